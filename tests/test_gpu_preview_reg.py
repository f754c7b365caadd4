"""GPU: mipnerf_preview_reg_grad byte for byte against the host build of csrc/preview_reg.hpp (tests/hostmath/preview_reg.cpp, which
test_preview_reg_cpu.py pins bit for bit to the float32 restatement of tests/preview_reg_fixture.py), and the regulariser end to end through
`TuneState.step` against the numbers the fixtures alone give for the same recipe (preview_reg_fixture.RECORDED)."""
import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_reg_fixture as rf
import preview_tune_fixture as tf
import test_preview_reg_cpu as cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
WHITE = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def hm():
    return cpu.host()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_grad(master, mask, dims, lo, hi, degree, grad, w_sigma, w_colour, w_view, eps):
    """`grad` plus the regulariser's gradient by the library, as a new numpy array (n_points = 1: the weights reach the kernel as given)"""
    from mipnerf_pl_amd import preview
    out = _dev(grad)
    preview.tune_regularise(_dev(master), _dev(mask), dims, lo, hi, degree, out, w_sigma, w_colour, w_view, eps, 1)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_the_kernel_is_the_host_build_byte_for_byte(hm, degree):
    """three lattices (r_a != 1; x-lines of 2 and of 67 points), no mask / holes / one point, into a random grad with sentinel pads"""
    for dims, lo, hi in rf.LATTICES:
        scale = rf.axis_scale(dims, lo, hi)
        master = rf.master_rows(dims, degree)
        before = cpu.grad_before(master.shape, degree)
        for name, mask in cpu.masks_of(dims, degree).items():
            want = cpu.host_grad(hm, master, mask, dims, degree, scale, before, *rf.WEIGHTS, rf.EPS)
            got = gpu_grad(master, mask, dims, lo, hi, degree, before, *rf.WEIGHTS, rf.EPS)
            assert got.tobytes() == want.tobytes(), (degree, dims, name)
            on = np.ones(master.shape[:3], bool) if mask is None else mask != 0
            assert got[~on].tobytes() == before[~on].tobytes() and (got[..., rf.USED[degree]:] == F(-555.0)).all()      # added into, pads kept
            if name != "single":                                       # (a point without neighbours has a zero total-variation gradient)
                assert (got[on][:, :rf.USED[degree]] != before[on][:, :rf.USED[degree]]).mean() > 0.9


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_each_weight_alone_and_none(hm, degree):
    dims, lo, hi = rf.LATTICES[0]
    scale = rf.axis_scale(dims, lo, hi)
    master = rf.master_rows(dims, degree)
    before = cpu.grad_before(master.shape, degree)
    mask = cpu.masks_of(dims, degree)["holes"]
    for w in ((rf.WEIGHTS[0], 0.0, 0.0), (0.0, rf.WEIGHTS[1], 0.0), (0.0, 0.0, rf.WEIGHTS[2])):
        want = cpu.host_grad(hm, master, mask, dims, degree, scale, before, *w, rf.EPS)
        got = gpu_grad(master, mask, dims, lo, hi, degree, before, *w, rf.EPS)
        assert got.tobytes() == want.tobytes(), (degree, w)
        if degree > 0 or w[2] == 0.0:
            assert got.tobytes() != before.tobytes()
    # all weights zero: grad keeps its bytes (negative zeros and a NaN among them)
    odd = before.copy()
    odd[0, 0, 0, 0], odd[1, 1, 1, 1] = F(-0.0), F(np.nan)
    got = gpu_grad(master, mask, dims, lo, hi, degree, odd, 0.0, 0.0, 0.0, rf.EPS)
    assert got.tobytes() == odd.tobytes()


def test_two_launches_give_equal_bytes():
    dims, lo, hi = rf.LATTICES[0]
    master = rf.master_rows(dims, 2)
    before = cpu.grad_before(master.shape, 2)
    mask = cpu.masks_of(dims, 2)["holes"]
    runs = [gpu_grad(master, mask, dims, lo, hi, 2, before, *rf.WEIGHTS, rf.EPS) for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_a_nan_master_entry_spoils_exactly_its_stencils(hm, degree):
    dims, lo, hi = rf.LATTICES[0]
    scale = rf.axis_scale(dims, lo, hi)
    for name, mask in cpu.masks_of(dims, degree).items():
        master, q, e = cpu.nan_case(dims, degree, mask)
        on = np.ones(master.shape[:3], bool) if mask is None else mask != 0
        zero = np.zeros(master.shape, F)
        got = gpu_grad(master, mask, dims, lo, hi, degree, zero, *rf.WEIGHTS, rf.EPS)
        assert cpu.same_bits(got, cpu.host_grad(hm, master, mask, dims, degree, scale, zero, *rf.WEIGHTS, rf.EPS)), (degree, name)
        spoiled = {(int(i), int(j), int(k), int(en)) for k, j, i, en in np.argwhere(np.isnan(got))}
        assert spoiled == {p + (e,) for p in rf.stencil_points(q, dims, on, e >= 4)}, (degree, name)
        assert len(spoiled) == 13 if mask is None else len(spoiled) <= 13


def test_the_regulariser_through_tune_state_against_the_recorded_recipe():
    """The recipe of preview_reg_fixture.recipe through `TuneState.step`, with and without the weights.  The yardstick is what the
    fixtures alone give (RECORDED; test_preview_reg_cpu.py replays it): batch loss 1.518e-3 -> 1.86e-5 and a final total variation of
    (703, 4470) with the regulariser, (4195, 9061) without.  Required, with a margin of 2 over the recorded values for the fp32 gradients
    of the march and their arrival order: the regularised run's total variation is at most twice the recorded one and below the
    unregularised run's, its final batch loss at most twice the recorded one and below the first."""
    from mipnerf_pl_amd import preview
    import test_gpu_preview_tune as gt
    rays = pf.scene_rays()
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, WHITE)
    ok = np.flatnonzero(~want[4])
    target = _dev(want[0].astype(F)[ok])
    student = tf.student_rows(teacher, 1)
    batch = gt._rays_of(rays, ok)
    scale = rf.axis_scale(pf.DIMS, pf.LO, pf.HI)
    R = rf.RECIPE
    result = {}
    for reg in (False, True):
        baked = gt._baked(student, 1, tf.occupancy_of(np.ones_like(student)))          # every cell occupied: the mask keeps every point
        kw = dict(tv_sigma=R["tv_sigma"], tv_colour=R["tv_colour"], sh_decay=R["sh_decay"], tv_eps=R["tv_eps"]) if reg else {}
        state, losses = preview.tune_field(baked, lambda k: (batch, target), R["steps"], WHITE, lr_sigma=R["lr_sigma"], lr_colour=R["lr_colour"],
                                           t_min=1e-3, **kw)
        tv = rf.total_variation(state.master.cpu().numpy(), None, 1, scale, R["tv_eps"])
        last = float(state.step(batch, target, WHITE))                                    # the loss after the last of the steps
        first = float(losses[0])
        print(f"regularised {reg}: loss {first:.4e} -> {last:.4e}, tv sigma {tv[0]:.4e} colour {tv[1]:.4e} "
              f"(recorded {rf.RECORDED[reg]['loss']:.4e}, {rf.RECORDED[reg]['tv']})")
        assert state.regularised == reg and (state.n_points == 720 if reg else state._n_points is None)
        assert abs(first - rf.RECORDED[reg]["loss0"]) < 2e-5
        result[reg] = (first, last, tv)
    first, last, tv = result[True]
    assert last <= 2.0 * rf.RECORDED[True]["loss"] and last < first
    for got, recorded, plain in zip(tv, rf.RECORDED[True]["tv"], result[False][2]):
        assert got <= 2.0 * recorded and got < plain
