"""Every stage of the bf16 MLP training kernels against float64 ON ITS OWN SAVED OPERANDS (tests/saved_operands.py; the instrument is
proven on the CPU by tests/test_saved_operands_cpu.py).

mipnerf_mlp_forward_train, mipnerf_mlp_dgrad and mipnerf_mlp_wgrad run once per case through the context of model.mlp.native(), on
real-valued data: orc.make_params(density_gain=20), the oracle's integrated positional encoding of synthetic rays rounded to bf16,
d_raw ~ N(0, 1e-2) colour / N(0, 1e-3) density.  The act, mask and delta buffers are read back and decoded; every saved activation,
every saved delta, both raw heads and every parameter gradient must lie inside the admissible interval of the float64 result of ITS
stage computed from the inputs the kernel itself stored -- gamma = (n + 2) 2^-23 sum |terms|, derived, not measured.  Nothing
propagates from layer to layer, so this is the criterion for rounding and accumulation that the exact-integer suite
(test_gpu_mlp_exact.py) cannot be and the cascade bounds ("2 x measured") only approximate.  Exact beside it: every mask bit equals
(saved activation > 0), the saved raw delta is RNE_bf16(d_raw), rows of padded samples are zero in every delta block, gradients of
unused parameters are zero; and the share of elements whose interval holds two bf16 values stays under the caps (25 %; 50 % where an
unsaved intermediate stands between), so that the check cannot hide a failure behind indecision.

Cases (B, N): default at (3, 11) -- the ray changes inside a wave tile --, (5, 13) -- one row past two wave tiles -- and (33, 65)
-- nine workgroup tiles, the last ragged; w128, noview, d6s3, dc2 and the 672-wide two-kernel form (row-major bf16 encodings) at
(5, 13) and (33, 65).  Every case records its figures per stage (gpu_util.record, tags "mlp_local ..."): violations, undecided
share, elements that differ from RNE(z), and for fp32 outputs the worst |error| / gamma."""
import warnings

import numpy as np
import pytest
import torch

import exact_mlp_fixture as X
import saved_operands as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANTS = ["w128", "noview", "d6s3", "dc2", "unbounded"]
CASES = [("default", 3, 11), ("default", 5, 13), ("default", 33, 65)] + [(a, B, N) for a in VARIANTS for B, N in ((5, 13), (33, 65))]
EXACT_CASES = [(a, B, N) for a in ("default", "unbounded") for B, N in ((3, 11), (33, 65))]


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def _model(name, params, N):
    from mipnerf_pl_amd import MipNerf
    arch, views = X.ARCHS[name]
    kw = {"mlp_" + k: v for k, v in arch.items() if k != "xyz_dim"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = MipNerf(num_samples=N, precision="bf16", use_viewdirs=views, unbounded=name == "unbounded", **kw)
    missing, unexpected = m.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    assert not missing and not unexpected
    return m.to(DEV)


def _run(name, params, enc, view32, d_raw):
    """the three kernels once on enc [B, N, xyz], view32 [B, 32], d_raw [B, N, 4] (float32 arrays holding bf16 values where the
    kernels take bf16) -> (Saved, model, raw tensor of the forward-with-save)"""
    from mipnerf_pl_amd import _lib as L, ops
    arch, views = X.ARCHS[name]
    tp, spec = S.plan_of(arch, views)
    B, N = enc.shape[:2]
    M = B * N
    model = _model(name, params, N)
    nctx = model.mlp.native(torch.device(DEV))
    e16 = torch.from_numpy(enc).to(DEV).to(torch.bfloat16).contiguous()
    v16 = torch.from_numpy(view32).to(DEV).to(torch.bfloat16).contiguous()
    assert torch.equal(e16.float().cpu(), torch.from_numpy(enc)) and torch.equal(v16.float().cpu(), torch.from_numpy(view32))
    dr = torch.from_numpy(d_raw).to(DEV).contiguous()
    sz = nctx.train_sizes(M)
    n_wt = (M + 255) // 256 * 8
    assert sz[1] == n_wt * tp.NMASK * 1024 and sz[2] == n_wt * tp.NG * 2048 and sz[0] >= n_wt * tp.NH * 2048, (sz, n_wt, tp.NH, tp.NG)
    act, masks, delta, partials = (torch.zeros(s, dtype=torch.uint8, device=DEV) for s in sz)
    raw = torch.empty(B, N, 4, device=DEV)
    rs = torch.empty_like(raw)
    shapes = [p.shape for p in model.mlp.ordered_params()]
    assert [tuple(s) for s in shapes] == [tuple(s) for s in spec.shapes.values()]
    grad = torch.zeros(nctx.grad_numel(shapes), device=DEV)
    lib, st = L.lib(), ops._stream()
    L.check(lib.mipnerf_mlp_forward_train(nctx.handle, M, N, e16.data_ptr(), v16.data_ptr(), rs.data_ptr(), raw.data_ptr(), act.data_ptr(),
                                          masks.data_ptr(), st), "mlp_forward_train")
    L.check(lib.mipnerf_mlp_dgrad(nctx.handle, M, dr.data_ptr(), masks.data_ptr(), delta.data_ptr(), st), "mlp_dgrad")
    L.check(lib.mipnerf_mlp_wgrad(nctx.handle, M, act.data_ptr(), delta.data_ptr(), partials.data_ptr(), grad.data_ptr(), 0, st), "mlp_wgrad")
    torch.cuda.synchronize()
    HT = act[:n_wt * tp.NH * 2048].view(torch.bfloat16).float().cpu().numpy().reshape(n_wt, tp.NH, 2, 64, 8)
    GT = delta.view(torch.bfloat16).float().cpu().numpy().reshape(n_wt, tp.NG, 2, 64, 8)
    MK = masks.cpu().numpy().view(np.uint32).reshape(n_wt, tp.NMASK, 64, 4)
    sv = S.decode(tp, M, HT, MK, GT, enc=e16.float().cpu().numpy() if tp.pre_gemm else None, raw=raw.cpu().numpy(),
                  grad_flat=grad.cpu().numpy(), shapes=spec.shapes)
    return sv, spec, model, raw


@pytest.mark.parametrize("name,B,N", CASES)
def test_every_stage_is_inside_its_float64_interval(G, name, B, N):
    arch, views = X.ARCHS[name]
    c = S.real_case(arch, views, B, N, seed=1000 * B + N)
    sv, spec, model, raw = _run(name, c["params"], c["enc"], c["view"], c["d_raw"])
    fails, report = S.check_all(spec, c["params"], sv, c["d_raw"], record=G.record, tag=f"{name} {B}x{N}")
    for k, r in report.items():
        print(f"mlp_local {name} {B}x{N} {k}: {r}")
    assert np.array_equal(sv.acts["enc"][:sv.M], c["enc"].reshape(sv.M, -1))            # the saved encoding is the one passed in
    if views:
        assert np.array_equal(sv.acts["view"][:sv.M], np.repeat(c["view"], N, axis=0))   # the view row of sample s is row s // N
    assert not fails, fails
    if name == "default":
        # the link to the headline kernel: the inference forward returns the forward-with-save's raw output bit for bit
        from mipnerf_pl_amd import _lib as L
        with torch.no_grad():
            rgb, den, _ = model.mlp(torch.from_numpy(c["enc"]).to(DEV), torch.from_numpy(c["view"][:, :27]).to(DEV), precision=L.PREC_BF16,
                                    return_activated=True)
        infer = torch.cat([rgb, den], -1).reshape(raw.shape)
        G.record(f"mlp_local inference_vs_train {name} {B}x{N}", mismatches=int((infer != raw).sum()))
        assert torch.equal(infer, raw)


@pytest.mark.parametrize("name,B,N", EXACT_CASES)
def test_exact_cases_decode_to_the_float64_activations_and_deltas(G, name, B, N):
    """the decoder against the device, and the exact pin extended from outputs to intermediates: on the exact-integer cases every saved
    activation, mask and delta equals the fixture's float64 pass bit for bit"""
    c = X.case(name, B, N)
    views = c["use_viewdirs"]
    M = B * N
    view32 = np.zeros((B, 32), np.float32)
    view32[:, :27] = c["venc"]
    sv, spec, _, _ = _run(name, c["params"], c["enc"], view32, c["d_raw"])
    _, _, acts, deltas = X.float64_pass(c["params"], c["enc"], c["venc"], c["d_raw"], c["skip_index"], views)
    names = [f"x{i + 1}" for i in range(spec.D)] + [None] + [spec.hv(i) for i in range(spec.nV)]
    gnames = [f"g{i + 1}" for i in range(spec.D)] + [None] + [spec.gv(i) for i in range(spec.nV)]
    assert len(names) == len(acts)
    rec = {}
    for n, g, a, d in zip(names, gnames, acts, deltas):
        if n is None:
            continue                          # the bottleneck is never stored
        a, d = a.reshape(M, -1).numpy(), (d * (a > 0)).reshape(M, -1).numpy()      # the kernels store delta behind the ReLU gate
        rec[n] = int((sv.acts[n][:M] != a).sum())
        rec[g] = int((sv.deltas[g][:M] != d).sum())
    rec.update({"mask " + k: v for k, v in S.mask_mismatches(spec, sv).items()})
    rec.update({"padded " + k: v for k, v in S.padded_nonzeros(sv).items()})
    rec["raw_delta"] = S.raw_delta_mismatches(sv, c["d_raw"])
    G.record(f"mlp_local exact_intermediates {name} {B}x{N}", **rec)
    assert not any(rec.values()), {k: v for k, v in rec.items() if v}
