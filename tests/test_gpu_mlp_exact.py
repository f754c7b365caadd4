"""The bf16 (and fp32) MLP kernels against float64 in EXACT integer arithmetic, at ragged sizes (tests/exact_mlp_fixture.py).

With small-integer weights, biases, encodings and upstream gradients every product, every partial sum in any order, every bf16
store of an activation or delta and the folded view matrix are exactly representable, so the kernels -- inference forward
(mlp_bf16_gen*.hip; pre_gemm / mlp_bf16_pre / mlp_bf16_fused for the 672-wide encoding), training forward-with-save, dgrad,
k_mlp_wgrad, k_wgrad_reduce, the device-side fold in the pack kernel -- must return the float64 result BIT FOR BIT whatever their
dataflow, tile shape, MFMA shape or reduction order.  Every comparison below is torch.equal against the float64 result cast to
float32; there is no tolerance.  The only exception is the activated output (sigmoid / softplus are not exact arithmetic), held
to test_mlp_fp32's settings against float64 sigmoid / softplus of the exact raw: rgb <= 5e-6, density <= 2e-5 relative to
1 + |density|.  The fixture's conditions are proven on the CPU by tests/test_exact_mlp_cpu.py, which also shows that the
one-element errors this module exists for change the float64 result.

Shapes (B, N), M = B * N; the workgroup tile is 256 samples = 8 wave tiles of 32 and the view row of sample s is row s // N:
(1, 1), (1, 31), (3, 11) = 33, (5, 13) = 65, (3, 85) = 255, (1, 257), (27, 19) = 513, (33, 65) = 2145, (17, 241) = 4097 for the
default architecture; (3, 11) and (33, 65) for w128, noview, d6s3, dc2, the unbounded 672-wide one (row-major encodings), w512
(inference only) and w200c72 (zero-padded on the 256 / 128 kernels).

What this cannot prove: rounding behaviour and accumulation accuracy on real-valued data, which stay with the emulation and
oracle tests and, stage by stage against float64 on the kernels' own saved operands, with tests/test_gpu_mlp_local.py.  Every run records, per case (gpu_util.record, tags "mlp_exact ..."), the number of mismatching entries per
tensor and the first one's index -- for raw also that sample's index modulo 32, modulo 256 and its ray s // N."""
import warnings

import numpy as np
import pytest
import torch

import exact_mlp_fixture as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAINABLE = [n for n in X.ARCHS if n != "w512"]          # the 512-wide trunk has a bf16 inference kernel only
FLAT = [n for n in TRAINABLE if n != "w200c72"]           # flat parameter mode needs a generated shape
TRAIN_CASES = [c for c in X.CASES if c[0] in TRAINABLE]
GRID_DEFAULT = 256


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def _model(name, params, N, precision):
    from mipnerf_pl_amd import MipNerf
    arch, views = X.ARCHS[name]
    kw = {"mlp_" + k: v for k, v in arch.items() if k != "xyz_dim"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MipNerf(num_samples=N, precision=precision, use_viewdirs=views, unbounded=name == "unbounded", **kw)
    missing, unexpected = m.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    assert not missing and not unexpected
    return m.to(DEV)


def _context(model):
    with warnings.catch_warnings():          # w200c72: "runs zero-padded on the 256 / 128 kernels"
        warnings.simplefilter("ignore")
        return model.mlp.native(torch.device(DEV))


def _inputs(c, dtype):
    """enc [B,N,xyz], view encoding [B,32] (columns 27-31 zero; all zero without view directions), d_raw on the device"""
    B = c["enc"].shape[0]
    v32 = torch.zeros(B, 32)
    if c["use_viewdirs"]:
        v32[:, :27] = torch.from_numpy(c["venc"])
    return torch.from_numpy(c["enc"]).to(DEV).to(dtype), v32.to(DEV).to(dtype), torch.from_numpy(c["d_raw"]).to(DEV)


def _diff(rec, key, got, want, N=None):
    """mismatches of `got` against the float64 `want` cast to float32 into rec: count and first flat index; for raw [B,N,4]
    (N given) the first mismatching sample's index modulo 32 and 256 and its ray.  Returns the count."""
    got = got.detach().float().cpu()
    want = want.float()
    assert got.shape == want.shape, (key, got.shape, want.shape)
    ne = got.reshape(-1) != want.reshape(-1)
    n = int(ne.sum())
    rec[key + ":mismatches"] = n
    rec[key + ":first"] = int(torch.nonzero(ne)[0]) if n else -1
    if n and N is not None:
        s = rec[key + ":first"] // 4
        rec[key + ":sample_mod32"], rec[key + ":sample_mod256"], rec[key + ":ray"] = s % 32, s % 256, s // N
    return n


def _assert_clean(G, tag, rec):
    """record every figure first, then assert that no tensor has a mismatching entry"""
    G.record(tag, **rec)
    bad = {k.rsplit(":", 1)[0] for k, v in rec.items() if k.endswith(":mismatches") and v}
    assert not bad, (tag, {k: v for k, v in rec.items() if k.rsplit(":", 1)[0] in bad})


def _forward(model, c, prec):
    enc, v32, _ = _inputs(c, torch.float32)
    with torch.no_grad():
        rgb, den, act = model.mlp(enc, v32[:, :27] if c["use_viewdirs"] else None, precision=prec, return_activated=True)
    return torch.cat([rgb, den], -1).clone(), act.clone()


def _check_activated(model, c, act, tag):
    """sigmoid / softplus (mip_nerf.py:236-238) of the EXACT raw in float64; test_mlp_fp32's bounds"""
    pad, bias = float(np.float32(model.rgb_padding)), float(np.float32(model.density_bias))
    rgb = torch.sigmoid(c["raw"][..., :3]) * (1 + 2 * pad) - pad
    den = torch.nn.functional.softplus(c["raw"][..., 3:] + bias, beta=1, threshold=20)
    act = act.double().cpu()
    ea = float((act[..., :3] - rgb).abs().max())
    es = float(((act[..., 3:] - den).abs() / (1 + den.abs())).max())
    print(f"{tag}: activated rgb {ea:.3e} (<= 5e-6), density {es:.3e} relative (<= 2e-5)")
    assert ea <= 5e-6 and es <= 2e-5, (tag, ea, es)


# ---- a. bf16 inference forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,N", X.CASES)
def test_bf16_inference_forward_is_exact(G, name, B, N):
    """DMA ring / register ring (option 0), one-kernel / two-kernel form of the wide encoding (option 6), and 256 / 1 / 3 persistent
    workgroups (option 1: with 1 and 3 a workgroup walks several tiles and the ring phase crosses tile ends)"""
    from mipnerf_pl_amd import _lib as L
    c = X.case(name, B, N)
    model = _model(name, c["params"], N, "bf16")
    ctx = _context(model)
    rec, act0 = {}, None
    try:
        for form in ((1, 0) if name == "unbounded" else (None,)):
            if form is not None:
                ctx.set_option(6, form)
            for dma in (1, 0):
                ctx.set_option(0, dma)
                for grid in (GRID_DEFAULT, 1, 3):
                    ctx.set_option(1, grid)
                    raw, act = _forward(model, c, L.PREC_BF16)
                    _diff(rec, f"raw form={form} dma={dma} grid={grid}", raw, c["raw"], N)
                    act0 = act if act0 is None else act0
                    assert torch.equal(act, act0), ("activated output depends on the route", form, dma, grid)
    finally:
        ctx.set_option(0, 1)
        ctx.set_option(1, GRID_DEFAULT)
        if name == "unbounded":
            ctx.set_option(6, 1)
    _assert_clean(G, f"mlp_exact bf16_fwd {name} {B}x{N}", rec)
    _check_activated(model, c, act0, f"mlp_exact bf16_fwd {name} {B}x{N}")


# ---- b. fp32 inference forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,N", X.CASES)
def test_fp32_inference_forward_is_exact(G, name, B, N):
    """register-resident and LDS-resident fp32 kernels (option 5)"""
    from mipnerf_pl_amd import _lib as L
    c = X.case(name, B, N)
    model = _model(name, c["params"], N, "fp32")
    ctx = _context(model)
    rec, acts = {}, []
    try:
        for resident in (1, 0):
            ctx.set_option(5, resident)
            raw, act = _forward(model, c, L.PREC_FP32)
            _diff(rec, f"raw resident={resident}", raw, c["raw"], N)
            acts.append(act)
    finally:
        ctx.set_option(5, 1)
    _assert_clean(G, f"mlp_exact fp32_fwd {name} {B}x{N}", rec)
    for act in acts:
        _check_activated(model, c, act, f"mlp_exact fp32_fwd {name} {B}x{N}")


# ---- c. training kernels through autograd.mlp_native --------------------------------------------------------------------------------
def _train_once(model, c):
    """forward-with-save + backward of sum(raw * d_raw): raw (detached)"""
    from mipnerf_pl_amd.autograd import mlp_native
    enc, v32, d_raw = _inputs(c, torch.bfloat16)
    raw = mlp_native(model.mlp, enc, v32)
    (raw * d_raw).sum().backward()
    return raw.detach()


def _diff_grads(rec, model, c, scale=1.0, prefix=""):
    for k, p in model.mlp.named_parameters():
        assert p.grad is not None and p.grad.shape == p.shape, k
        want = c["grads"][k]
        _diff(rec, prefix + k, p.grad, torch.zeros(p.shape, dtype=torch.float64) if want is None else scale * want)


@pytest.mark.parametrize("name,B,N", TRAIN_CASES)
def test_training_kernels_are_exact_with_per_tensor_gradients(G, name, B, N):
    c = X.case(name, B, N)
    model = _model(name, c["params"], N, "bf16")
    _context(model)
    rec = {}
    _diff(rec, "raw", _train_once(model, c), c["raw"], N)
    _diff_grads(rec, model, c)
    _assert_clean(G, f"mlp_exact train {name} {B}x{N}", rec)


@pytest.mark.parametrize("name,B,N", [c for c in TRAIN_CASES if c[0] in FLAT])
def test_training_kernels_are_exact_in_flat_mode_and_accumulate(G, name, B, N):
    """flatten_parameters(): the split reduction writes into the buffer the .grad tensors alias; a second forward + backward adds
    (accumulate = 1) and must give exactly twice the gradient; after _flat_grad_valid is reset the gradient is exact again"""
    c = X.case(name, B, N)
    model = _model(name, c["params"], N, "bf16")
    model.mlp.flatten_parameters()
    assert model.mlp.grads_are_flat()
    rec = {}
    _diff(rec, "raw", _train_once(model, c), c["raw"], N)
    assert model.mlp._flat_grad_valid and model.mlp.grads_are_flat()
    _diff_grads(rec, model, c)
    _diff(rec, "second raw", _train_once(model, c), c["raw"], N)
    _diff_grads(rec, model, c, scale=2.0, prefix="accumulated ")
    model.mlp._flat_grad_valid = False
    _train_once(model, c)
    _diff_grads(rec, model, c, prefix="after reset ")
    _assert_clean(G, f"mlp_exact train_flat {name} {B}x{N}", rec)


# ---- d. stale scratch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "unbounded"])
def test_small_case_after_a_large_one_on_the_same_context_is_exact(G, name):
    """one model, one context: (17, 241) through forward + backward, then (3, 11) -- nothing of the larger run may be left over in
    delta / partials / act"""
    big, small = X.case(name, 17, 241), X.case(name, 3, 11)
    model = _model(name, big["params"], 241, "bf16")
    ctx = _context(model)
    rec = {}
    _diff(rec, "large raw", _train_once(model, big), big["raw"], 241)
    _diff_grads(rec, model, big, prefix="large ")
    model.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in small["params"].items()}, strict=True)
    for p in model.mlp.parameters():
        p.grad = None
    assert _context(model) is ctx
    _diff(rec, "small raw", _train_once(model, small), small["raw"], 11)
    _diff_grads(rec, model, small, prefix="small ")
    _assert_clean(G, f"mlp_exact stale_scratch {name}", rec)


# ---- e. training forward against inference forward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TRAINABLE)
def test_training_forward_gives_the_inference_forwards_bits(G, name):
    """implied by (a) and (c); asserted directly for the diagnostic"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd.autograd import mlp_native
    B, N = 33, 65
    c = X.case(name, B, N)
    model = _model(name, c["params"], N, "bf16")
    _context(model)
    enc, v32, _ = _inputs(c, torch.bfloat16)
    train = mlp_native(model.mlp, enc, v32).detach()
    infer, _ = _forward(model, c, L.PREC_BF16)
    ne = (train != infer).reshape(-1, 4).any(1)
    first = int(torch.nonzero(ne)[0]) if bool(ne.any()) else -1
    G.record(f"mlp_exact train_vs_inference {name}", mismatching_samples=int(ne.sum()), first=first, first_mod32=first % 32,
             first_mod256=first % 256, first_ray=first // N)
    assert torch.equal(train, infer), (name, int(ne.sum()), first)
