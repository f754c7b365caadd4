"""Build libmipnerf_hip.so (the drop-in library), libmipnerf_diag.so (measurement tooling), libmipnerf_preview.so (the baked-lattice
preview renderer), libmipnerf_preview_mip.so (the same renderer over a pyramid of lattices), libmipnerf_preview_sparse.so (the same
renderer over lattices that store only the rows next to an occupied cell) and libmipnerf_preview_tune.so (the gradient of that renderer
with respect to the lattice and an Adam step on it) and libmipnerf_preview_360.so (the renderer of the unbounded-scene model: a lattice over
the contracted space) and libmipnerf_preview_reg.so (the gradient of a total-variation term and an SH decay on the tuned lattice) and
libmipnerf_preview_tune_360.so (the gradient of the contracted-space renderer with respect to its lattice) and libmipnerf_proposal_360.so
(the proposal density of the unbounded-scene model from a pyramid of contracted lattices) and libmipnerf_fuse.so (rendered depth fused into a
truncated signed distance volume) for gfx950 in-tree (hipcc cross-compiles without a GPU).

    python -m mipnerf_pl_amd.build [--force]

Steps: (1) run the four generators of csrc/ (what they share lives in csrc/gen_common.py), one kernel per architecture variant <i> of
gen_mlp_bf16.VARIANTS (variant 0 of the first two without the suffix):
    gen_mlp_bf16.py   mlp_bf16_gen[_v<i>].hip, _gen_plan_tables[_v<i>].bin, mlp_plan_gen.hpp, mlp_variants_gen.hpp
    gen_mlp_train.py  mlp_bf16_trainfwd_gen[_v<i>].hip or mlp_bf16_trainfwd_pre_gen_v<i>.hip, mlp_bf16_dgrad_gen[_v<i>].hip,
                      _gen_train_tables[_v<i>].bin, mlp_train_variants_gen.hpp
    gen_mlp_f32r.py   mlp_f32r_gen_v<i>.hip, _gen_f32r_tables_v<i>.bin, mlp_f32r_variants_gen.hpp
    gen_pre_gemm.py   pre_gemm_gen_v<i>.hip, mlp_bf16_pre_gen_v<i>.hip, mlp_bf16_fused_gen_v<i>.hip, _gen_pre_tables_v<i>.bin,
                      mlp_pre_variants_gen.hpp
(2) compile each .hip translation unit to an object (the ray-math units with -ffp-contract=off, see
raymath.hpp), (3) link the shared library next to the sources.  No torch headers are used:
the library's only dependency is the HIP runtime.
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(CSRC, os.environ.get("MIPNERF_LIB_NAME", "libmipnerf_hip.so"))
ARCH = "gfx950"

# generated MFMA kernels: ReLU must be a single v_max_f32 that the COMPILER emits (no inline asm next to MFMAs, see
# gen_mlp_bf16.py relu1); without IEEE mode llvm.maxnum needs no canonicalising pre-instruction
NO_IEEE = ["-fno-honor-nans", "-mno-amdgpu-ieee"]

UNITS = [
    # (source, extra flags)
    ("kernels_ray.hip", ["-ffp-contract=off"]),
    ("kernels_train.hip", ["-ffp-contract=off"]),
    ("kernels_360.hip", ["-ffp-contract=off"]),
    ("kernels_resample_grad.hip", ["-ffp-contract=off"]),
    ("kernels_pack.hip", []),
    ("kernels_mlp_f32.hip", ["-ffp-contract=off"]),
    ("kernels_gemm_f32.hip", ["-ffp-contract=off"]),
    ("mlp_bf16_gen.hip", NO_IEEE + ["-ffp-contract=off"]),    # the fused IPE must round like kernels_ray.hip
    ("mlp_bf16_trainfwd_gen.hip", NO_IEEE + ["-ffp-contract=off"]),
    ("mlp_bf16_dgrad_gen.hip", NO_IEEE),
    ("kernels_wgrad.hip", []),
    ("kernels_eval.hip", ["-ffp-contract=off"]),
    ("kernels_vis.hip", ["-ffp-contract=off"]),
    ("kernels_pyramid.hip", ["-ffp-contract=off"]),     # q_rgb * q_a + (1 - q_a) rounds three times, as on the host
    ("kernels_downscale.hip", ["-ffp-contract=off"]),   # float(q) / 255.f stays one rounded division
    ("kernels_mesh.hip", ["-ffp-contract=off"]),        # lattice means lo + float(i) * h and the shared IPE round as stated in the header
    ("kernels_occupancy.hip", ["-ffp-contract=off"]),   # frustum end points o + t * d and floor((x - lo) / h) round as stated in the header
    ("kernels_bucket.hip", []),                         # integer ranks and copies only: no floating-point arithmetic to contract
    ("kernels_guided.hip", ["-ffp-contract=off"]),      # err + rate * (mean - err) and the float64 mixture round as stated in the header
    ("kernels_proposal.hip", ["-ffp-contract=off"]),    # the frustum mean and the trilinear blend round as stated in lattice_sample.hpp
    ("selftest.hip", ["-ffp-contract=off"]),
    ("capi.hip", []),
]
# the generated per-variant families: (unit stem, flags of its units, stem of its table blob, linker symbol of the blob); a unit is
# <stem>_v<i>.hip, a blob <stem>[_v<i>].bin linked in as <symbol>[_v<i>].  The fused IPE must round like kernels_ray.hip.
FAMILIES = [
    ("mlp_bf16_gen", NO_IEEE + ["-ffp-contract=off"], "_gen_plan_tables", "mip_plan_tables"),
    ("mlp_bf16_trainfwd_gen", NO_IEEE + ["-ffp-contract=off"], "_gen_train_tables", "mip_train_tables"),
    ("mlp_bf16_trainfwd_pre_gen", NO_IEEE + ["-ffp-contract=off"], None, None),
    ("mlp_bf16_dgrad_gen", NO_IEEE, None, None),
    ("mlp_f32r_gen", NO_IEEE + ["-ffp-contract=off"], "_gen_f32r_tables", "mip_f32r_tables"),     # the register-resident fp32 kernels
    ("pre_gemm_gen", NO_IEEE + ["-ffp-contract=off"], "_gen_pre_tables", "mip_pre_tables"),       # two- and one-kernel bf16 forms of wide encodings
    ("mlp_bf16_pre_gen", NO_IEEE + ["-ffp-contract=off"], None, None),
    ("mlp_bf16_fused_gen", NO_IEEE + ["-ffp-contract=off"], None, None),
]


def _family_files(col, ext):
    """sorted (file name, family row, variant suffix) of the files <stem>[_v<i>].<ext> in csrc/, stem = column `col` of the family rows"""
    out = []
    for f in sorted(os.listdir(CSRC)):
        for fam in FAMILIES:
            m = fam[col] and re.fullmatch(re.escape(fam[col]) + r"((?:_v\d+)?)\.(?:" + ext + ")", f)
            if m:
                out.append((f, fam, m.group(1)))
    return out


# measurement tooling (in-process MFMA ceilings, CU -> CU hand-off probe): its own library, include/mipnerf_diag.h -- the drop-in
# library above is the hot path only
DIAG_LIB = os.path.join(CSRC, "libmipnerf_diag.so")
DIAG_UNITS = [("kernels_diag.hip", []), ("diag_capi.hip", [])]
# the baked-lattice preview renderer (include/mipnerf_preview.h): a third library, so the drop-in library keeps its entry points
PREVIEW_LIB = os.path.join(CSRC, "libmipnerf_preview.so")
PREVIEW_UNITS = [("kernels_preview.hip", ["-ffp-contract=off"]),      # the slab test, o + t * d and the row blend round as stated in preview_march.hpp
                 ("preview_capi.hip", ["-ffp-contract=off"])]          # the world step step_scale * min(h) is formed on the host
# the preview over a cone-radius pyramid of lattices (include/mipnerf_preview_mip.h): a fourth library, so the preview library keeps its
# entry points as well
PREVIEW_MIP_LIB = os.path.join(CSRC, "libmipnerf_preview_mip.so")
PREVIEW_MIP_UNITS = [("kernels_preview_mip.hip", ["-ffp-contract=off"]),   # P7: the same roundings as kernels_preview.hip, bit for bit
                     ("preview_mip_capi.hip", ["-ffp-contract=off"])]       # the spacings s_l and the world step are formed on the host
# the preview over lattices that store only the rows the march reads (include/mipnerf_preview_sparse.h): a fifth library, so the other
# two preview libraries keep their entry points
PREVIEW_SPARSE_LIB = os.path.join(CSRC, "libmipnerf_preview_sparse.so")
PREVIEW_SPARSE_UNITS = [("kernels_preview_sparse.hip", ["-ffp-contract=off"]),   # the march of kernels_preview_mip.hip, bit for bit
                        ("preview_sparse_capi.hip", ["-ffp-contract=off"])]       # the spacings s_l and the world step are formed on the host
# fine-tuning the lattice through the renderer (include/mipnerf_preview_tune.h): a sixth library, so the three preview libraries keep their
# entry points
PREVIEW_TUNE_LIB = os.path.join(CSRC, "libmipnerf_preview_tune.so")
PREVIEW_TUNE_UNITS = [("kernels_preview_tune.hip", ["-ffp-contract=off"]),   # sweep A is the march of kernels_preview.hip, bit for bit
                      ("preview_tune_capi.hip", ["-ffp-contract=off"])]       # the world step step_scale * min(h) is formed on the host
# the preview of the unbounded-scene model, a lattice over the contracted space (include/mipnerf_preview_360.h): a seventh library, so the
# four preview libraries keep their entry points
PREVIEW_360_LIB = os.path.join(CSRC, "libmipnerf_preview_360.so")
PREVIEW_360_UNITS = [("kernels_preview_360.hip", ["-ffp-contract=off"]),   # the warp, the contraction and the row blend round as stated in preview_march_360.hpp
                     ("preview_360_capi.hip", ["-ffp-contract=off"])]       # the contracted step step_scale * min(h) is formed on the host
# regularising the tuning (include/mipnerf_preview_reg.h): an eighth library, so the five preview libraries keep their entry points
PREVIEW_REG_LIB = os.path.join(CSRC, "libmipnerf_preview_reg.so")
PREVIEW_REG_UNITS = [("kernels_preview_reg.hip", ["-ffp-contract=off"]),   # the differences, the norm and its quotients round as stated in preview_reg.hpp
                     ("preview_reg_capi.hip", ["-ffp-contract=off"])]       # no arithmetic of its own; compiled like the kernels for one rule
# tuning a contracted lattice through its own march (include/mipnerf_preview_tune_360.h): a ninth library, so the other eight keep their
# entry points and their bytes
PREVIEW_TUNE_360_LIB = os.path.join(CSRC, "libmipnerf_preview_tune_360.so")
PREVIEW_TUNE_360_UNITS = [("kernels_preview_tune_360.hip", ["-ffp-contract=off"]),   # sweep A is the march of kernels_preview_360.hip, bit for bit
                          ("preview_tune_360_capi.hip", ["-ffp-contract=off"])]       # the contracted step step_scale * min(h) is formed on the host
# the proposal density of the unbounded-scene model from a pyramid of contracted density lattices (include/mipnerf_proposal_360.h): a
# tenth library, so the other nine keep their entry points and their bytes
PROPOSAL_360_LIB = os.path.join(CSRC, "libmipnerf_proposal_360.so")
PROPOSAL_360_UNITS = [("kernels_proposal_360.hip", ["-ffp-contract=off"]),   # the Gaussian rounds as in k_cast_ipe_360, the blends as stated in lattice_sample_360.hpp
                      ("proposal_360_capi.hip", ["-ffp-contract=off"])]       # the spacings and inv_h are formed on the host
# rendered depth fused into a truncated signed distance volume (include/mipnerf_fuse.h): an eleventh library, so the other ten keep their
# entry points and their bytes
FUSE_LIB = os.path.join(CSRC, "libmipnerf_fuse.so")
FUSE_UNITS = [("kernels_fuse.hip", ["-ffp-contract=off"]),   # the projection rows, D - t and s / trunc round as stated in fuse_rules.hpp
              ("fuse_capi.hip", ["-ffp-contract=off"])]       # the spacing is formed on the host; the host build of rules T rounds like the kernel
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-fno-gpu-rdc", "-Wall",
          "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-value", "-Wno-unused-result"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build the gfx950 kernels)")


def _digest(paths, flags) -> str:
    h = hashlib.sha256()
    for p in sorted(paths):
        with open(p, "rb") as f:
            h.update(os.path.basename(p).encode())
            h.update(f.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def generate() -> None:
    """Run the four generators.  Every architecture of gen_mlp_bf16.VARIANTS gets its own inference kernel (mlp_bf16_gen_v<i>.hip),
    its training kernels + table blob when mlp_train_plan covers it, and a row in the generated dispatch headers; files of
    variants that no longer exist are removed first, so adding / removing a shape is an edit of VARIANTS and a rebuild."""
    for f, _, sfx in _family_files(0, "hip|o") + _family_files(2, "bin"):
        if sfx or f.endswith(".bin"):          # (the unsuffixed units of variant 0 are listed in UNITS)
            os.remove(os.path.join(CSRC, f))
    for gen in ("gen_mlp_bf16.py", "gen_mlp_train.py", "gen_mlp_f32r.py", "gen_pre_gemm.py"):
        subprocess.check_call([sys.executable, os.path.join(CSRC, gen), CSRC])


def variant_units():
    """(source, flags) of the generated per-variant kernels present after generate()."""
    return [(f, fam[1]) for f, fam, sfx in _family_files(0, "hip") if sfx]


def tables_object() -> str:
    """Link the binary tables the generators write (one blob per variant and family that has one) into the library: a
    one-object file made with the assembler's .incbin, so the plan modules stay the only definition of those tables."""
    src = os.path.join(CSRC, "_gen_train_tables.c")
    obj = os.path.join(CSRC, "train_tables.o")
    blobs = _family_files(2, "bin")
    with open(src, "w") as f:
        f.write("/* generated by build.py */\n")
        for fam in FAMILIES:                       # family by family, as the dispatch headers declare them
            for name, _, sfx in [b for b in blobs if b[1] is fam]:
                f.write('__asm__(".section .rodata\\n.global %s%s\\n.balign 16\\n'
                        '%s%s:\\n.incbin \\"%s\\"\\n.previous\\n");\n' % (fam[3], sfx, fam[3], sfx, os.path.join(CSRC, name)))
    subprocess.check_call(["gcc", "-c", "-fPIC", src, "-o", obj])
    return obj


def build(force: bool = False, verbose: bool = True) -> str:
    generate()
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp", ".bin"))]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_hip.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_diag.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_mip.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_sparse.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_tune.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_360.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_reg.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_preview_tune_360.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_proposal_360.h"))
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mipnerf_fuse.h"))
    stamp = os.path.join(CSRC, ".build_stamp_" + os.path.basename(LIB))
    units = UNITS[:-1] + variant_units() + UNITS[-1:]          # capi.hip last
    dig = _digest(deps, COMMON + sum((f for _, f in units + PREVIEW_UNITS + PREVIEW_MIP_UNITS + PREVIEW_SPARSE_UNITS + PREVIEW_TUNE_UNITS + PREVIEW_360_UNITS + PREVIEW_REG_UNITS + PREVIEW_TUNE_360_UNITS + PROPOSAL_360_UNITS + FUSE_UNITS), []))
    if not force and os.path.exists(LIB) and os.path.exists(DIAG_LIB) and os.path.exists(PREVIEW_LIB) and os.path.exists(PREVIEW_MIP_LIB) and \
            os.path.exists(PREVIEW_SPARSE_LIB) and os.path.exists(PREVIEW_TUNE_LIB) and os.path.exists(PREVIEW_360_LIB) and os.path.exists(PREVIEW_REG_LIB) and \
            os.path.exists(PREVIEW_TUNE_360_LIB) and os.path.exists(PROPOSAL_360_LIB) and os.path.exists(FUSE_LIB) and os.path.exists(stamp) and open(stamp).read() == dig:
        if verbose:
            print(f"[build] {LIB} is up to date")
        return LIB
    cc = hipcc()
    objs = []
    procs = []
    for src, extra in units + DIAG_UNITS + PREVIEW_UNITS + PREVIEW_MIP_UNITS + PREVIEW_SPARSE_UNITS + PREVIEW_TUNE_UNITS + PREVIEW_360_UNITS + PREVIEW_REG_UNITS + PREVIEW_TUNE_360_UNITS + PROPOSAL_360_UNITS + FUSE_UNITS:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        cmd = [cc] + COMMON + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print("[build]", " ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    failed = False
    for src, p in procs:
        out, _ = p.communicate()
        if out and verbose:
            sys.stdout.write(out.decode(errors="replace"))
        if p.returncode != 0:
            failed = True
            print(f"[build] FAILED: {src}")
    if failed:
        raise RuntimeError("hipcc failed")
    fuse_objs = objs[len(objs) - len(FUSE_UNITS):]
    objs = objs[:len(objs) - len(FUSE_UNITS)]
    prop360_objs = objs[len(objs) - len(PROPOSAL_360_UNITS):]
    objs = objs[:len(objs) - len(PROPOSAL_360_UNITS)]
    tune360_objs = objs[len(objs) - len(PREVIEW_TUNE_360_UNITS):]
    objs = objs[:len(objs) - len(PREVIEW_TUNE_360_UNITS)]
    reg_objs = objs[len(objs) - len(PREVIEW_REG_UNITS):]
    objs = objs[:len(objs) - len(PREVIEW_REG_UNITS)]
    p360_objs = objs[len(objs) - len(PREVIEW_360_UNITS):]
    objs = objs[:len(objs) - len(PREVIEW_360_UNITS)]
    tune_objs = objs[len(objs) - len(PREVIEW_TUNE_UNITS):]
    objs = objs[:len(objs) - len(PREVIEW_TUNE_UNITS)]
    sparse_objs = objs[len(objs) - len(PREVIEW_SPARSE_UNITS):]
    mip_objs = objs[len(units) + len(DIAG_UNITS) + len(PREVIEW_UNITS):len(objs) - len(PREVIEW_SPARSE_UNITS)]
    preview_objs = objs[len(units) + len(DIAG_UNITS):len(units) + len(DIAG_UNITS) + len(PREVIEW_UNITS)]
    diag_objs = objs[len(units):len(units) + len(DIAG_UNITS)]
    objs = objs[:len(units)]
    objs.append(tables_object())
    # Link by hand (not through hipcc) against an EMPTY stub named libamdhip64.so with no SONAME, so the
    # library's DT_NEEDED entry is exactly "libamdhip64.so".  PyTorch-ROCm wheels bundle their own HIP
    # runtime under that soname-less name; a DT_NEEDED of "libamdhip64.so.7" (what hipcc's link step
    # records from /opt/rocm) would pull a SECOND HIP runtime into the process, whose streams, events and
    # synchronisation are invisible to torch.  With the un-versioned name the loader reuses whichever
    # runtime is already mapped (torch's), and falls back to /opt/rocm/lib (RUNPATH) in a torch-free host.
    stub_dir = os.path.join(CSRC, "_stub")
    os.makedirs(stub_dir, exist_ok=True)
    stub_c = os.path.join(stub_dir, "stub.c")
    with open(stub_c, "w") as f:
        f.write("/* empty: only provides the DT_NEEDED name libamdhip64.so */\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", os.path.join(stub_dir, "libamdhip64.so"), stub_c])
    rocm_lib = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    # The dynamic symbol table is the C ABI and nothing else: a linker version script keeps `mipnerf_*` (the entry points
    # include/mipnerf_hip.h / mipnerf_diag.h / mipnerf_preview.h / mipnerf_preview_mip.h / mipnerf_preview_sparse.h / mipnerf_preview_tune.h / mipnerf_preview_360.h / mipnerf_preview_reg.h / mipnerf_preview_tune_360.h / mipnerf_proposal_360.h / mipnerf_fuse.h declare) and makes every C++ launcher, kernel handle and table blob local.
    vers = os.path.join(stub_dir, "exports.map")
    with open(vers, "w") as f:
        f.write("{ global: mipnerf_*; local: *; };\n")
    cmd = ["g++", "-shared", "-fPIC", "-o", LIB] + objs + [
        "-Wl,--version-script=" + vers, "-Wl,--no-as-needed", "-L" + stub_dir, "-lamdhip64", "-Wl,--as-needed", "-Wl,--allow-shlib-undefined",
        "-Wl,-rpath," + rocm_lib, "-Wl,--enable-new-dtags", "-lstdc++", "-lm"]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", DIAG_LIB] + diag_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_LIB] + preview_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_MIP_LIB] + mip_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_SPARSE_LIB] + sparse_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_TUNE_LIB] + tune_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_360_LIB] + p360_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_REG_LIB] + reg_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PREVIEW_TUNE_360_LIB] + tune360_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", PROPOSAL_360_LIB] + prop360_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    cmd = ["g++", "-shared", "-fPIC", "-o", FUSE_LIB] + fuse_objs + cmd[cmd.index("-Wl,--version-script=" + vers):]
    if verbose:
        print("[build]", " ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    with open(stamp, "w") as f:
        f.write(dig)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
