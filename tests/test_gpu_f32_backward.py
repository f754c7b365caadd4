"""The fp32 ("parity") MLP backward -- mlp_backward_f32_impl over kernels_gemm_f32.hip -- against a float64 restatement of
models/mip_nerf.py:75-111 and its autograd gradients, at the ragged sizes where each of its routes guards a tail by hand.

Inputs (gpu_util.f32_backward_case): oracle make_params(seed, density_gain=10), encodings / view encodings uniform in [-1, 1],
d_raw standard normal with the boundary rows (0, M-1, and 15, 16, 63, 64, 255, 256, 511, 512, 2047, 2048, 2079, 2080 where they
exist) multiplied by 4.  Mask agreement: a sample with a float64 pre-activation within tau = 32 * delta of zero (delta = the
largest |float64 - torch fp32| pre-activation difference of that layer) gets a fresh encoding row, so float64, torch fp32 and the
kernels take the same ReLU branches and the gradient is the same linear map of d_raw in all three.

Bound, per tensor, err(x) = max |x - g64| / max |g64|:   err(native) <= max(4 * err(torch fp32 on the CPU), FLOOR).
Both are fp32 sums of the same products in another order, hence the margin of 4.  FLOOR = 8 * 2^-23 = 9.5e-7 (8 ulp of the
tensor's maximum) covers a tensor whose fp32 restatement happens to be exact or nearly so -- a bias gradient of a single sample
is d_raw itself, and the one or three sums of a head's bias gradient can come out right by luck.  A correct fp32 result still
takes half an ulp when it is stored and half an ulp of a PARTIAL sum in each of the up to three additions that combine the
split-K or slice partials (four group sums, then their fixed-order combination); partial sums of terms with both signs run up
to a few times the final value, taken as 4 x: (1 + 3) * 1/2 ulp * 4 = 8 ulp.  Nothing in the bound comes from the kernels.
Unused parameters (use_viewdirs=False) must be exactly zero.

err(torch fp32) of the worst tensor of a case is 5.0e-7 (130/90, M = 65) to 1.1e-6 (default, M = 1: raw_rgb) -- reference only,
computed on the CPU.  err(native) per case is recorded by every run (gpu_util.record, tags "f32_bwd ..."); it has NOT yet been
measured on an MI355X: no figures are quoted here until a run has produced them.
delta per hidden layer of the default architecture, largest over its eight shapes (tau = 32 x that): trunk layers 0..7
2.3e-6, 9.2e-7, 6.9e-7, 6.4e-7, 4.1e-7, 1.0e-6, 6.3e-7, 5.5e-7, view layer 6.1e-7; over every case and layer delta <= 2.8e-6,
tau <= 9.0e-5, and the loop ends after at most 8 of its 20 rounds.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 8.0 * 2.0 ** -23
MARGIN = 4.0

# (B, N): M = B * N samples, rowdiv = N in the view-feature product
SHAPES = [(1, 1),       # every wide product on the 64 x 64 fallback; one k per split, 255 empty splits; b_ones bias sums
          (3, 21),      # 63: last M below the big-kernel gate; k_relu_mask and the separate rank-1 launch
          (1, 64),      # first M on the big kernels: four full K blocks, 252 empty splits
          (5, 13),      # 65: K tail of one row after full 16-blocks; a 256-row dgrad tile with 65 live rows
          (3, 67),      # 201: odd rowdiv in k_thin_wgrad<32>
          (7, 37),      # 259: three rows past a 256-row dgrad tile
          (33, 65),     # 2145: second thin slice (2080 with rowdiv 65) of 65 rows; five 512-sample v4 slices, the last partial
          (17, 241)]    # 4097: split chunk rounded 17 -> 32: 129 live splits, the last holding one row, 127 empty
VARIANT_SHAPES = [(5, 13), (33, 65)]
# name -> (oracle make_params keywords, use_viewdirs)
ARCHS = {"default": ({}, True),
         "w128": (dict(net_width=128, net_width_condition=128), True),      # two rows share a sign-bit word; odd M: half-filled last word
         "noview": (dict(net_width_condition=256), False),
         "d6s3": (dict(net_depth=6, skip_index=3), True),
         "dc2": (dict(net_depth_condition=2), True),                        # odd number of inner view layers: the g1 -> g0 copy-back
         "w512": (dict(net_width=512, net_width_condition=256), True),
         "w200c72": (dict(net_width=200, net_width_condition=72), True),    # zero-padded on 256 / 128
         "w130c90dc2": (dict(net_width=130, net_width_condition=90, net_depth_condition=2), True)}
CASES = [("default", B, N) for B, N in SHAPES] + [(a, B, N) for a in ARCHS if a != "default" for B, N in VARIANT_SHAPES]


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def _model_kw(name):
    arch, views = ARCHS[name]
    kw = {"mlp_" + k: v for k, v in arch.items()}
    if not views:
        kw["use_viewdirs"] = False
    return kw


@functools.lru_cache(maxsize=None)
def reference(name, B, N):
    """The case's inputs, its float64 gradients g64 and err(torch fp32) per tensor -- computed once, shared, never modified."""
    import gpu_util as G
    arch, views = ARCHS[name]
    case = G.f32_backward_case(arch, B, N, seed=1000 * B + N, use_viewdirs=views)
    venc = case["venc"] if views else None
    raw64, g64, e64 = G.mlp_grads(case["params"], case["enc"], venc, case["d_raw"], case["skip_index"], torch.float64, True)
    raw32, g32, e32 = G.mlp_grads(case["params"], case["enc"], venc, case["d_raw"], case["skip_index"], torch.float32, True)
    ref = {k: v for k, v in g64.items() if v is not None}
    ref.update(d_enc=e64, raw_rgb=raw64[..., :3], raw_density=raw64[..., 3:])
    got32 = dict(g32, d_enc=e32, raw_rgb=raw32[..., :3], raw_density=raw32[..., 3:])
    err32 = {k: G.rel_err(got32[k], v) for k, v in ref.items()}
    return dict(case, ref=ref, err32=err32, bound={k: max(MARGIN * e, FLOOR) for k, e in err32.items()},
                unused=[k for k, v in g64.items() if v is None])


def _device_inputs(ref, enc_grad=False):
    B = ref["venc"].shape[0]
    enc = torch.from_numpy(ref["enc"]).to(DEV).requires_grad_(enc_grad)
    v32 = torch.zeros(B, 32, device=DEV)
    if ref["use_viewdirs"]:
        v32[:, :27] = torch.from_numpy(ref["venc"]).to(DEV)
    return enc, v32, torch.from_numpy(ref["d_raw"]).to(DEV)


def _check(G, tag, ref, got):
    """record err(native) and err(torch fp32) of every tensor in `got`, then assert the bound on each"""
    errs = {k: G.rel_err(v, ref["ref"][k]) for k, v in got.items()}
    rec = {}
    for k, e in errs.items():
        rec[k + ":native"], rec[k + ":torch"] = e, ref["err32"][k]
    worst = max(errs, key=lambda k: errs[k] / ref["bound"][k])
    G.record(tag, worst_native=max(errs.values()), worst_torch=max(ref["err32"][k] for k in errs), **rec)
    print(f"{tag}: worst native {max(errs.values()):.3e} torch {max(ref['err32'][k] for k in errs):.3e}; closest to its bound: "
          f"{worst} {errs[worst]:.3e} <= {ref['bound'][worst]:.3e}")
    for k, e in errs.items():
        assert e <= ref["bound"][k], (tag, k, e, ref["err32"][k], ref["bound"][k])


def _autograd_run(G, name, B, N, enc_grad):
    from mipnerf_pl_amd.autograd import mlp_native_f32
    ref = reference(name, B, N)
    model = G.make_model(ref["params"], N, "fp32", **_model_kw(name))
    enc, v32, d_raw = _device_inputs(ref, enc_grad)
    raw = mlp_native_f32(model.mlp, enc, v32)
    (raw * d_raw).sum().backward()
    raw = raw.detach()
    got = dict(raw_rgb=raw[..., :3], raw_density=raw[..., 3:])
    for k, p in model.mlp.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        if k in ref["unused"]:
            assert torch.count_nonzero(p.grad) == 0, (k, "unused parameter with a non-zero gradient")
        else:
            got[k] = p.grad
    if enc_grad:
        got["d_enc"] = enc.grad
    return ref, got


@pytest.mark.parametrize("name,B,N", CASES)
def test_parameter_gradients_match_float64(G, name, B, N):
    ref, got = _autograd_run(G, name, B, N, False)
    _check(G, f"f32_bwd {name} {B}x{N}", ref, got)


@pytest.mark.parametrize("B,N", [(5, 13), (7, 37)])
@pytest.mark.parametrize("name", ["default", "d6s3"])
def test_encoding_gradient_matches_float64(G, name, B, N):
    """mipnerf_mlp_backward_f32_enc: the two accumulating big-GEMM launches (layer 0 and the skip layer) at ragged M"""
    ref, got = _autograd_run(G, name, B, N, True)
    _check(G, f"f32_bwd_enc {name} {B}x{N}", ref, got)


def test_reference_notices_one_boundary_row():
    """The test's own guard, reference only: without ONE boundary row (the last one, and row 2048) the float64 gradients of the
    largest default shape move by at least 20 x the bound asserted on that tensor."""
    import gpu_util as G
    B, N = SHAPES[-1]
    ref = reference("default", B, N)
    M = B * N
    for row in (M - 1, 2048):
        d = ref["d_raw"].copy()
        d.reshape(M, 4)[row] = 0.0
        _, g, _ = G.mlp_grads(ref["params"], ref["enc"], ref["venc"], d, ref["skip_index"], torch.float64)
        for k, v in g.items():
            moved = G.rel_err(v, ref["ref"][k])
            assert moved >= 20.0 * ref["bound"][k], (row, k, moved, ref["bound"][k])


# ---- the C ABI itself: accumulate, determinism, bounds of writes -------------------------------------------------------------
CANARY, POISON = 0xA5, 0xFF          # POISON: four of them are a NaN, so a result that read memory nobody wrote shows


class Guarded:
    """`nbytes` device bytes with a 256-byte canary before and after"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((256 + self.n + 256,), CANARY, dtype=torch.uint8, device=DEV)
        self.bytes = self.buf[256:256 + self.n]
        self.bytes.fill_(POISON)
        assert self.bytes.data_ptr() % 256 == 0

    def floats(self):
        return self.bytes.view(torch.float32)

    def intact(self):
        return bool((self.buf[:256] == CANARY).all()) and bool((self.buf[256 + self.n:] == CANARY).all())


def _direct(model, ref, N, accumulate=0, prefill=None, enc_grad=False):
    """forward-with-save + backward through the C ABI, the way _MLPNativeF32 calls it, on canaried buffers: (grad_flat, raw,
    d_enc or None) as clones"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    nctx = model.mlp.native(torch.device(DEV))
    enc, v32, d_raw = _device_inputs(ref)
    M = enc.shape[0] * N
    sb, wb = C.c_size_t(), C.c_size_t()
    L.lib().mipnerf_mlp_train_f32_bytes(nctx.handle, M, C.byref(sb), C.byref(wb))
    save, ws = Guarded(sb.value), Guarded(wb.value)
    grad = Guarded(4 * nctx.grad_numel([p.shape for p in model.mlp.ordered_params()]))
    if prefill is not None:
        grad.floats().copy_(prefill)
    raw, rgb_sigma = torch.empty(M, 4, device=DEV), torch.empty(M, 4, device=DEV)
    L.check(L.lib().mipnerf_mlp_forward_train_f32(nctx.handle, M, N, enc.data_ptr(), v32.data_ptr(), rgb_sigma.data_ptr(),
                                                  raw.data_ptr(), save.bytes.data_ptr(), ops._stream()), "mlp_forward_train_f32")
    d_enc = None
    if enc_grad:
        d_enc = torch.full_like(enc, float("nan"))
        L.check(L.lib().mipnerf_mlp_backward_f32_enc(nctx.handle, M, N, d_raw.data_ptr(), enc.data_ptr(), v32.data_ptr(),
                                                     save.bytes.data_ptr(), ws.bytes.data_ptr(), grad.bytes.data_ptr(), accumulate,
                                                     d_enc.data_ptr(), ops._stream()), "mlp_backward_f32_enc")
    else:
        L.check(L.lib().mipnerf_mlp_backward_f32(nctx.handle, M, N, d_raw.data_ptr(), enc.data_ptr(), v32.data_ptr(),
                                                 save.bytes.data_ptr(), ws.bytes.data_ptr(), grad.bytes.data_ptr(), accumulate,
                                                 ops._stream()), "mlp_backward_f32")
    torch.cuda.synchronize()
    assert save.intact() and ws.intact() and grad.intact(), "a write outside the stated buffer sizes"
    return grad.floats().clone(), raw, d_enc


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _prefill(n):
    return torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)


def _param_slices(model):
    out, off = {}, 0
    for k, p in model.mlp.named_parameters():
        out[k] = slice(off, off + p.numel())
        off += p.numel()
    return out


@pytest.mark.parametrize("B,N", [(3, 21), (5, 13), (33, 65)])
@pytest.mark.parametrize("name", ["default", "noview"])
def test_accumulate_adds_with_one_ieee_add(G, name, B, N):
    """accumulate=1 on a prefilled gradient buffer R gives R + g0 bit for bit (g0 = the accumulate=0 result of the same call):
    every route adds its finished, deterministic sum to the destination once.  Unused parameters: 0 without, R with accumulate."""
    ref = reference(name, B, N)
    model = G.make_model(ref["params"], N, "fp32", **_model_kw(name))
    g0, _, _ = _direct(model, ref, N)
    assert torch.isfinite(g0).all(), "an element of grad_flat was never written"
    R = _prefill(g0.numel())
    g1, _, _ = _direct(model, ref, N, accumulate=1, prefill=R)
    sl = _param_slices(model)
    bad = [k for k, s in sl.items() if not _same_bits(g1[s], R[s] + g0[s])]
    assert not bad, bad
    for k in ref["unused"]:
        assert torch.count_nonzero(g0[sl[k]]) == 0 and _same_bits(g1[sl[k]], R[sl[k]]), k
    assert (len(ref["unused"]) == 4) == (name == "noview")


@pytest.mark.parametrize("B,N", VARIANT_SHAPES)
@pytest.mark.parametrize("name", list(ARCHS))
def test_deterministic_and_inside_its_buffers(G, name, B, N):
    """Every call of this module twice: identical bits, canaries around grad_flat and behind save / workspace intact (checked
    inside _direct), every element of the outputs written (the buffers start as NaN)."""
    ref = reference(name, B, N)
    model = G.make_model(ref["params"], N, "fp32", **_model_kw(name))
    runs = {}
    for mode, kw in (("plain", {}), ("enc", dict(enc_grad=True))):
        a, b = _direct(model, ref, N, **kw), _direct(model, ref, N, **kw)
        for x, y in zip(a, b):
            if x is not None:
                assert torch.isfinite(x).all() and _same_bits(x, y), mode
        runs[mode] = a
    assert _same_bits(runs["plain"][0], runs["enc"][0])        # the encoding gradient is two more launches, nothing else
    if name in ("default", "noview"):
        R = _prefill(runs["plain"][0].numel())
        a, b = _direct(model, ref, N, accumulate=1, prefill=R), _direct(model, ref, N, accumulate=1, prefill=R)
        assert _same_bits(a[0], b[0])
