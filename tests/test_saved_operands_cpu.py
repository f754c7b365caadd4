"""CPU: the instrument of tests/test_gpu_mlp_local.py (tests/saved_operands.py) proven without a GPU.  The plan's numpy emulation
(mlp_train_plan.emulate_train_tile / emulate_wgrad / post_process) stands in for the kernels: its blocks go through the same decoder
and the same float64 stage references as the device buffers do.

* the decoder returns the per-sample values that went in, for both plan forms;
* on the exact-integer cases of tests/exact_mlp_fixture.py the decoded emulation IS the fixture's float64 activations and deltas;
* the emulation with bf16 operand rounding has no violation in any stage of any architecture, and the share of elements the check
  cannot decide (interval holds two bf16 values) stays under the caps -- a condition on the inputs, not a measurement;
* every defect the exact-integer suite cannot see leaves the admissible interval: a truncating store, a bias added after the
  rounding, an accumulator narrowed to bf16 between k-steps, a dropped k-step, a padded sample's delta left nonzero, weight-gradient
  partial sums kept in bf16.  Each mutant is the stage's own recipe run in fp32 k-steps with ONE defect; with the defect switched
  off (mode "none") the same model has no violation, which is asserted beside every mutant."""
import numpy as np
import pytest

import exact_mlp_fixture as X
import saved_operands as S
from mipnerf_pl_amd.mlp_train_plan import emulate_train_tile, emulate_wgrad, post_process

NAMES = ["default", "w128", "noview", "d6s3", "dc2", "unbounded"]
B, N = 5, 13                      # M = 65: one row past two wave tiles
_CACHE = {}


def emulate(tp, spec, params, enc, view32, d_raw, wgrad=True):
    """the three kernels on [M, .] inputs (view32 per sample), wave tile by wave tile like emulate_train -> Saved"""
    M = enc.shape[0]
    flat = np.concatenate([params[k].ravel() for k in spec.shapes])
    HT, GT, MK, ET, raw = [], [], [], [], []
    for t in range((M + 31) // 32):
        idx = np.minimum(np.arange(t * 32, t * 32 + 32), M - 1)
        valid = np.arange(t * 32, t * 32 + 32) < M
        h, g, r, e, m = emulate_train_tile(tp, flat, enc[idx], view32[idx], d_raw[idx], valid, True, return_masks=True)
        HT.append(h), GT.append(g), MK.append(m), ET.append(e), raw.append(r)
    HT, GT, MK = np.stack(HT), np.stack(GT), np.stack(MK)
    ET = np.stack(ET) if tp.pre_gemm else None
    grad = None
    if wgrad:
        part, _ = emulate_wgrad(tp, HT, GT, ET)
        grad = post_process(tp, flat, part)
    sv = S.decode(tp, M, HT, MK, GT, enc_blocks=ET, raw=np.concatenate(raw)[:M], grad_flat=grad, shapes=spec.shapes)
    return sv, dict(HT=HT, GT=GT, MK=MK, ET=ET)


def real(name):
    """the real-valued case of an architecture at M = 65 and its emulation: computed once, shared, never modified"""
    if name not in _CACHE:
        kw, views = X.ARCHS[name]
        tp, spec = S.plan_of(kw, views)
        c = S.real_case(kw, views, B, N, seed=300 + NAMES.index(name))
        M = B * N
        enc, view32, d_raw = c["enc"].reshape(M, -1), np.repeat(c["view"], N, axis=0), c["d_raw"].reshape(M, 4)
        sv, blocks = emulate(tp, spec, c["params"], enc, view32, d_raw)
        _CACHE[name] = dict(tp=tp, spec=spec, params=c["params"], enc=enc, view32=view32, d_raw=d_raw, sv=sv, blocks=blocks)
    return _CACHE[name]


# ---- decoder -----------------------------------------------------------------------------------------------------------------------------
def test_number_formats():
    import torch
    x = np.random.default_rng(0).normal(0, 1, 4096) * 2.0 ** np.random.default_rng(1).integers(-20, 20, 4096)
    x32 = x.astype(np.float32)
    want = torch.from_numpy(x32).to(torch.bfloat16).float().numpy().astype(np.float64)
    assert np.array_equal(S.rne_bf16(x32.astype(np.float64)), want)
    assert np.array_equal(S.rne_bf16(np.array([1.00390625, 1.01171875, -1.00390625, 0.0])), np.array([1.0, 1.015625, -1.0, 0.0]))   # ties to even
    assert np.array_equal(S.trunc_bf16(np.array([1.0078, -1.0078, 1.9999])), np.array([1.0, -1.0, 1.9921875]))
    # one step, not through float32: 1 + 2^-8 + 2^-30 lies above the tie; float32 would land on it and round to even (down)
    assert S.rne_bf16(np.array([1 + 2.0 ** -8 + 2.0 ** -30]))[0] == 1 + 2.0 ** -7
    assert S.ulp_bf16(1.5) == 2.0 ** -7 and S.ulp_fp32(1.5) == 2.0 ** -23 and S.ulp_fp32(0.0) > 0


@pytest.mark.parametrize("name", ["default", "unbounded", "dc2", "noview"])
def test_decoder_returns_the_values_that_went_in(name):
    c = real(name)
    sv, M = c["sv"], B * N
    assert np.array_equal(sv.acts["enc"][:M], c["enc"])
    if c["spec"].views:
        assert np.array_equal(sv.acts["view"][:M], c["view32"])
    want = np.zeros((M, 32))
    want[:, :4] = S.rne_bf16(c["d_raw"].astype(np.float64))
    assert np.array_equal(sv.deltas["raw"][:M], want)
    assert np.array_equal(sv.raw.shape, (M, 4))
    for kind in (0, 1):
        blocks = np.random.default_rng(kind).normal(size=(3, 5, 2, 64, 8)).astype(np.float32)
        assert np.array_equal(S.encode_blocks(S.decode_blocks(blocks, kind), kind), blocks)


@pytest.mark.parametrize("name", NAMES)
def test_exact_cases_decode_to_the_float64_activations_and_deltas(name):
    """the DLAYOUT blocks and the mask bits, against numbers that owe nothing to the plan"""
    c = X.case(name, 3, 11)
    kw, views = X.ARCHS[name]
    tp, spec = S.plan_of(kw, views)
    M = 33
    view32 = np.zeros((M, 32), np.float32)
    if views:
        view32[:, :27] = np.repeat(c["venc"], 11, axis=0)
    sv, _ = emulate(tp, spec, c["params"], c["enc"].reshape(M, -1), view32, c["d_raw"].reshape(M, 4))
    _, _, acts, deltas = X.float64_pass(c["params"], c["enc"], c["venc"], c["d_raw"], c["skip_index"], views)
    names = [f"x{i + 1}" for i in range(spec.D)] + ([None] + [spec.hv(i) for i in range(spec.nV)] if views else [])
    gnames = [f"g{i + 1}" for i in range(spec.D)] + ([None] + [spec.gv(i) for i in range(spec.nV)] if views else [])
    assert len(names) == len(acts)
    for n, g, a, d in zip(names, gnames, acts, deltas):
        if n is None:
            continue                          # the bottleneck is never stored
        assert np.array_equal(sv.acts[n][:M], a.reshape(M, -1).numpy()), n
        # the fixture's delta is the gradient of the ACTIVATION; the kernels store it behind the ReLU gate
        assert np.array_equal(sv.deltas[g][:M], (d * (a > 0)).reshape(M, -1).numpy()), g
    fails, report = S.check_all(spec, c["params"], sv, c["d_raw"])
    assert not fails, fails
    assert all(r.get("differs", 0) == 0 for r in report.values()), report
    for k, g in c["grads"].items():
        want = np.zeros(spec.shapes[k]) if g is None else g.numpy()
        assert np.array_equal(sv.grads[k], want.reshape(spec.shapes[k])), k


# ---- no false alarms, and a check that can decide ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_emulation_has_no_violation_and_few_undecided_elements(name):
    c = real(name)
    fails, report = S.check_all(c["spec"], c["params"], c["sv"], c["d_raw"])
    for k, r in report.items():
        print(name, k, r)
    assert not fails, fails
    bf16 = {k: r for k, r in report.items() if "undecided" in r}
    assert len(bf16) == 2 * c["spec"].D + 2 * c["spec"].nV          # every saved activation and every saved delta was judged
    # sharp: where no unsaved intermediate stands between, next to no element differs from RNE(z) at all
    weak = {f"g{c['spec'].D}"} | ({c["spec"].hv(0)} if not c["spec"].folded else set())
    assert all(r["differs"] <= 4 for k, r in bf16.items() if k not in weak), bf16


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------------
def _model(st, mode):
    """the stage's recipe as the kernels run it -- fp32 accumulator started from the bias, one k-step of 16 products at a time, gate,
    one RNE store -- with ONE defect: "trunc" the store truncates; "bias_after" the bias is added to the rounded sum; "acc_bf16" the
    accumulator is rounded to bf16 after every k-step; "drop" the second k-step is left out of the first 32 x 32 tile; "none"."""
    store = S.trunc_bf16 if mode == "trunc" else S.rne_bf16

    def run(terms, bias, gate):
        rows, out = terms[0][0].shape[0], terms[0][1].shape[0]
        acc = np.zeros((rows, out), np.float32)
        if bias is not None and mode != "bias_after":
            acc += bias.astype(np.float32)
        step = 0
        for a, w in terms:
            for k0 in range(0, a.shape[1], 16):
                p = a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T
                if mode == "drop" and step == 1:
                    p[:32, :32] = 0.0
                acc = (acc + p.astype(np.float32)).astype(np.float32)
                if mode == "acc_bf16":
                    acc = S.rne_bf16(acc.astype(np.float64)).astype(np.float32)
                step += 1
        x = acc.astype(np.float64)
        if bias is not None and mode == "bias_after":
            x = (S.rne_bf16(x) + bias).astype(np.float32).astype(np.float64)
        if isinstance(gate, str):
            x = np.maximum(x, 0.0)
        elif gate is not None:
            x = np.where(gate, x, 0.0)
        return store(x), step
    terms = list(st.terms)
    if st.inner is not None:
        a0, w0, b0 = st.inner
        terms[0] = (run([(a0, w0)], b0, None)[0], terms[0][1])
    return run(terms, st.bias, st.gate)


def _bf16_stages(c):
    fwd, _ = S.forward_stages(c["spec"], c["params"], c["sv"])
    return [(st, "forward") for st in fwd if st.kind == "bf16"] + [(st, "dgrad") for st in S.dgrad_stages(c["spec"], c["params"], c["sv"])]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", ["trunc", "bias_after", "acc_bf16"])
def test_rounding_and_accumulation_defects_leave_the_interval(name, mode):
    """at least 5 % of the elements of every stage the defect touches (3 % where an unsaved intermediate weakens the check)"""
    c = real(name)
    touched = 0
    for st, group in _bf16_stages(c):
        v0, steps = _model(st, "none")
        assert S.judge(st, v0)["violations"] == 0, (st.name, "the model without a defect must pass")
        if (mode == "bias_after" and group != "forward") or (mode == "acc_bf16" and steps < 2):
            continue                # dgrad has no bias; one k-step has nothing between k-steps
        r = S.judge(st, _model(st, mode)[0])
        share = r["violations"] / r["elements"]
        print(name, mode, st.name, f"{share:.3f}")
        assert share >= (0.03 if st.weak and st.name == f"g{c['spec'].D}" else 0.05), (name, mode, st.name, share)
        touched += 1
    assert touched >= c["spec"].D


@pytest.mark.parametrize("name", NAMES)
def test_a_dropped_k_step_leaves_the_interval(name):
    c = real(name)
    seen = 0
    for st, _ in _bf16_stages(c):
        v, steps = _model(st, "drop")
        if steps < 2:
            continue
        r = S.judge(st, v)
        assert r["violations"] > 0, (name, st.name)
        seen += 1
    assert seen >= 2 * c["spec"].D - 1


@pytest.mark.parametrize("name", ["default", "unbounded"])
def test_a_padded_samples_delta_left_nonzero_is_reported(name):
    c = real(name)
    tp, spec, M = c["tp"], c["spec"], B * N
    assert not any(S.padded_nonzeros(c["sv"]).values())
    b0, n, kind = tp.g_blocks["g3"]
    nat = S.decode_blocks(c["blocks"]["GT"][:, b0:b0 + n], kind)
    nat[M, 17] = 2.0 ** -9                     # the first padded row
    GT = c["blocks"]["GT"].copy()
    GT[:, b0:b0 + n] = S.encode_blocks(nat, kind)
    assert np.count_nonzero(GT != c["blocks"]["GT"]) == 1
    sv = S.decode(tp, M, c["blocks"]["HT"], c["blocks"]["MK"], GT, enc_blocks=c["blocks"]["ET"])
    fails, report = S.check_all(spec, c["params"], sv, c["d_raw"])
    assert report["exact"]["padded g3"] == 1 and fails == ["padded g3: 1 entries differ"], fails


@pytest.mark.parametrize("name", NAMES)
def test_weight_gradient_partials_kept_in_bf16_leave_the_bound(name):
    """per wave tile partial sums of delta^T a rounded to bf16 before the reduction, against the same sums kept in fp32"""
    c = real(name)
    stages, _ = S.wgrad_stages(c["spec"], c["params"], c["sv"])
    direct = [st for st in stages if st.terms]
    assert len(direct) >= 2 * c["spec"].D + 4
    for st in direct:
        d, a = st.terms[0]                     # [out, M], [in, M]
        for narrow in (False, True):
            total = np.zeros((d.shape[0], a.shape[0]), np.float32)
            for r0 in range(0, d.shape[1], 32):
                p = (d[:, r0:r0 + 32] @ a[:, r0:r0 + 32].T).astype(np.float32)
                total = total + (S.rne_bf16(p.astype(np.float64)).astype(np.float32) if narrow else p)
            r = S.judge(st, total.astype(np.float64))
            assert (r["violations"] > 0) == narrow, (name, st.name, narrow, r)
