"""What the four kernel generators (gen_mlp_bf16.py, gen_mlp_train.py, gen_mlp_f32r.py, gen_pre_gemm.py) share: the import path set-up, the
constants of the bf16 kernels, the launcher signatures, the host-side launcher body, the dispatch-header layout and the pieces of kernel text
that more than one kernel contains.  Plain functions that return C++ lines; every piece of generated text that exists in more than one
kernel is written here once."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(os.path.dirname(HERE))):      # the generators import each other and the plan modules of the package
    if _p not in sys.path:
        sys.path.insert(0, _p)

WAVES = 8             # wavefronts per workgroup (32 samples each); the 512-wide trunk: 4 (gen_mlp_bf16.waves_of), k_mlp_f32r: 4
CHUNK_BYTES = 1024
PREFETCH = 4          # A-fragment prefetch distance in chunks (registers A0..)
NE = 3                # rotating registers for LDS-resident B operands (E0..E2)


# ---- launcher signatures: the one definition of every generated launcher's parameter list ---------------------------------------
# (the variant-0 declarations in kernels.hpp are hand-written; tests/test_cabi_cpu.py compares them with these)
_HEAD = [("const void*", "stream_w"), ("const float*", "bias_tab")]
_OUT = [("float*", "rgb_sigma"), ("float*", "raw_out")]
_SAVE = [("void*", "HT"), ("void*", "masks")]
_PRE_IN = [("const void*", "pre_x"), ("const void*", "pre_acc"), ("const void*", "viewenc")]
_SHAPE = [("int64_t", "M"), ("int", "num_samples"), ("float", "density_bias"), ("float", "rgb_padding"), ("int", "grid_limit")]
_NOISE = [("const float*", "dnoise"), ("float", "dnoise_scale"), ("hipStream_t", "st")]
SIGNATURES = {
    "bf16": _HEAD + [("const void*", "enc"), ("const void*", "viewenc")] + _OUT + _SHAPE + [("bool", "dma"), ("const RayInputs*", "rays")] + _NOISE,
    "bf16_pre": _HEAD + _PRE_IN + _OUT + _SHAPE + _NOISE,       # the trunk of the two-kernel form and the one-kernel (fused) form
    "trainfwd": _HEAD + [("const void*", "enc"), ("const void*", "viewenc")] + _OUT + _SAVE + _SHAPE + [("const RayInputs*", "rays")] + _NOISE,
    "trainfwd_pre": _HEAD + _PRE_IN + _OUT + _SAVE + _SHAPE + _NOISE,
    "dgrad": [("const void*", "stream_wT"), ("const float*", "d_raw"), ("const void*", "masks"), ("void*", "GT"), ("int64_t", "M"),
              ("int", "grid_limit"), ("hipStream_t", "st")],
    "f32r": [("const void*", "stream_w"), ("const float*", "aux"), ("const float*", "enc"), ("const float*", "viewenc")] + _OUT + _SHAPE + _NOISE,
    "pre_gemm": _HEAD + [("const void*", "enc"), ("int", "frag"), ("void*", "pre_x"), ("void*", "pre_acc"), ("int64_t", "M"),
                         ("int", "grid_limit"), ("hipStream_t", "st")],
}


def _wrap(head, items, tail, width=150):
    """head + the comma-separated items + tail, filled to `width` columns with the continuation lines aligned behind head"""
    lines, cur = [], head
    for i, it in enumerate(items):
        piece = it + (", " if i + 1 < len(items) else tail)
        if i and len(cur) + len(piece.rstrip()) > width:
            lines.append(cur.rstrip())
            cur = " " * len(head)
        cur += piece
    return lines + [cur]


def signature(name, kind):
    """first line(s) of a launcher's definition, up to and including the opening brace"""
    return _wrap(f"hipError_t {name}(", [f"{t} {n}" for t, n in SIGNATURES[kind]], ") {")


def fn_typedef(tname, kind):
    return _wrap(f"typedef hipError_t (*{tname})(", [f"{t} {n}" for t, n in SIGNATURES[kind]], ");")


def prototype(name, kind):
    return _wrap(f"hipError_t {name}(", [t for t, _ in SIGNATURES[kind]], ");")


def launcher(name, kind, kernels, launch, namespace=None, wg_per_cu=None, lds_bytes=None, rayin=None, range_check=None, attr_first=False):
    """Lines of one host-side launcher: the grid from the tile count and grid_limit, the per-device cache around the dynamic-LDS attribute
    of every kernel instantiation in `kernels`, the `launch` statement(s), hipGetLastError().
    wg_per_cu / lds_bytes: the standard bf16 kernel scales grid_limit (CUs) by its workgroups per CU.
    rayin: None, "null" (a constant empty RayIn) or "rays" (filled from the `rays` argument when there is one).
    range_check: condition on the 64-bit tile count nt64 that rejects the call; None narrows it to int unchecked.
    attr_first: the attribute block in front of the grid computation instead of behind it."""
    if range_check:
        grid = ["    const int64_t nt64 = (M + kTileSamples - 1) / kTileSamples;",
                f"    if ({range_check}) return hipErrorInvalidValue;",
                "    const int ntiles = (int)nt64;"]
    else:
        grid = ["    const int ntiles = (int)((M + kTileSamples - 1) / kTileSamples);"]
    if wg_per_cu is not None:
        grid.append(f"    grid_limit *= {wg_per_cu};      // workgroups per CU (LDS: {lds_bytes} B each)")
    grid += ["    int grid = ntiles < grid_limit ? ntiles : grid_limit;",
             "    if (grid < 1) grid = 1;"]
    attr = ["    static int attr_done[64] = {};",
            "    int dev = 0;",
            "    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return hipErrorInvalidDevice;",
            "    if (!attr_done[dev]) {"]
    for i, k in enumerate(kernels):
        attr.append(f"        {'er' if i else 'hipError_t er'} = hipFuncSetAttribute((const void*){k}, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);")
        attr.append("        if (er != hipSuccess) return er;")
    attr += ["        attr_done[dev] = 1;",
             "    }"]
    L = signature(name, kind)
    if namespace:
        L.append(f"    using namespace {namespace};")
    L += attr + grid if attr_first else grid + attr
    if rayin == "null":
        L.append("    const RayIn rin = {nullptr, nullptr, nullptr, nullptr, 0, 0};")
    elif rayin == "rays":
        L.append("    RayIn rin = {nullptr, nullptr, nullptr, nullptr, 0, 0};")
        L.append("    if (rays) rin = RayIn{rays->t, rays->origins, rays->dirs, rays->radii, rays->min_deg, rays->disable_integration};")
    return L + list(launch) + ["    return hipGetLastError();", "}"]


def dispatch_header(banner, body, rows, n, before_namespace=()):
    """A *_variants_gen.hpp: `body` (typedefs, per-variant prototypes and blob declarations, comment lines), then one table of n entries
    per row (table type, table name, {variant: entry}); a variant without an entry gets nullptr.  A row may also be a comment line."""
    L = [banner, "#pragma once", '#include "kernels.hpp"'] + list(before_namespace) + ["namespace mip {"] + list(body)
    for row in rows:
        if isinstance(row, str):
            L.append(row)
            continue
        ttype, tname, entries = row
        L.append(f"static const {ttype} {tname}[{n}] = {{{', '.join(entries.get(vi, 'nullptr') for vi in range(n))}}};")
    L.append("}  // namespace mip")
    return "\n".join(L) + "\n"


# ---- kernel text ------------------------------------------------------------------------------------------------------------------
SELECTORS = [
    "bf16x8 P1, P2;   // selection matrices of the transposing MFMAs: P1[k][n] = (n == k), P2[k][n] = (n == 16 + k)",
    "#pragma unroll",
    "for (int j = 0; j < 8; ++j) {",
    "    P1[j] = (__bf16)((n == hi * 8 + j) ? 1.0f : 0.0f);",
    "    P2[j] = (__bf16)((n == 16 + hi * 8 + j) ? 1.0f : 0.0f);",
    "}",
]


def thread_prologue(priv, priv_note="", bias=True, selectors=False, setprio_note="as the inference kernel (gen_mlp_bf16.py)", first_group=True):
    """Lines of a bf16 kernel from the LDS declaration to the tile loop: lane / wave indices, the ring and wave-private LDS pointers
    (priv = (base name, lane pointer name, offset constant, per-wave size constant)), the selection matrices of the training kernels,
    the bias table's copy to LDS, the static priority of the second half of the workgroup, ring group 0 of the first tile."""
    base, lane_ptr, off, size = priv
    L = ["    extern __shared__ __attribute__((aligned(16))) char smem[];",
         "    const int tid = threadIdx.x;",
         "    const int lane = tid & 63;",
         "    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);",
         "    const int hi = lane >> 5, n = lane & 31;",
         "    const unsigned lane16 = (unsigned)lane * 16u;",
         "    const char* ring_lane = smem + lane16;"]
    if bias:
        L.append("    const char* bias_lane = smem + kRingBytes + hi * 64;")
    L += [f"    char* {base} = smem + {off} + wave * {size};{priv_note}",
          f"    const char* {lane_ptr} = {base} + lane16;"]
    if selectors:
        L += ["    " + ln for ln in SELECTORS]
    if bias:
        L += ["    for (int i = tid; i < kBiasBytes / 16; i += blockDim.x)",
              "        reinterpret_cast<float4*>(smem + kRingBytes)[i] = reinterpret_cast<const float4*>(bias_tab)[i];",
              "    __syncthreads();"]
    L.append(f"    if (wave >= 4) __builtin_amdgcn_s_setprio(1);     // {setprio_note}")
    if first_group:
        L.append("    if ((int)blockIdx.x < ntiles) issue_group<DMA>(stream, smem, 0, 0, wave, lane16);")
    return L


def lda(c, group, slots):
    """load of the A fragment of chunk c from an LDS ring of `slots` groups of `group` chunks, into its rotating register"""
    return f"A{c % PREFETCH} = LDA({((c // group) % slots) * group * CHUNK_BYTES + (c % group) * CHUNK_BYTES});"


def activation_store(training):
    """Lines of the bf16 kernels' last step of a tile: density noise, the two activations, the stores (training: raw_out is not optional)"""
    note = "mip_nerf.py:232-233"
    L = ["if (hi == 0 && s < M) {"]
    if not training:
        L.append(f"    // {note}: raw_density += density_noise * randn (randomized training only), BEFORE the activation")
    return L + [
        "    const float noisy_density = dnoise ? raw_density + dnoise_scale * dnoise[s] : raw_density;" + (f"   // {note}" if training else ""),
        "    rgb_sigma[s] = make_float4(rgb_activation(raw_r, rgb_padding), rgb_activation(raw_g, rgb_padding),",
        "                               rgb_activation(raw_b, rgb_padding), density_activation(noisy_density, density_bias));",
        ("    " if training else "    if (raw_out) ") + "raw_out[s] = make_float4(raw_r, raw_g, raw_b, raw_density);",
        "}",
    ]
