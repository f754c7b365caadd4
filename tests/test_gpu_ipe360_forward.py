"""GPU: the unbounded-scene forward path entry by entry against float64 -- k_sample_along_rays_360, k_cast_ipe_360 and
k_cast_ipe_360_tile (fp32 rows, bf16 rows and bf16 fragments), k_gauss_360 and k_lattice_ipe_360_tile behind
mipnerf_sample_along_rays_360, mipnerf_cast_ipe_360, mipnerf_gauss_360 and mipnerf_lattice_ipe_360 -- on seven classes of rays, five
ragged shapes (1 to 258 samples: below, at and one past a workgroup's 64, one past a fragment tile's 256), five ranges of degrees (the
shipped 16 among them) and both values of `contracted`, on a hand-made table of Gaussians and on a small lattice.

tests/ipe360_forward.py has the operands, the float64 truths, the budget of every entry and the constants, which come from the host
build of csrc/raymath360.hpp and never from a kernel; tests/test_ipe360_forward_cpu.py checks that fixture without a GPU.  Nothing
here is normalised by a batch maximum and no entry is left out.  Every output lies in front of a canary tail that must come back
untouched; every route that promises "the same bits" is held to them; the share of each budget the device reaches is recorded.

Each stage gets the fixture's operands (the cast stages the host build's fence posts, not the sampler kernel's), so that what the CPU
test asserts about them holds here too."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ipe360_forward as f3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_VALUE = -7.25           # exact in bf16
F = np.float32


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Out:
    """a device buffer of `shape` followed by a canary tail"""

    def __init__(self, shape, bf16=False):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.full((self.n + f3.CANARY,), CANARY_VALUE, device=DEV, dtype=torch.bfloat16 if bf16 else torch.float32)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, what):
        out = self.buf.float().cpu().numpy()               # the widening of bf16 is exact
        assert np.all(out[self.n:] == F(CANARY_VALUE)), f"{what} wrote behind its output"
        return out[:self.n].reshape(self.shape)


def _lib():
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    return L, L.lib(), ops._stream()


def sample(near, far, t_rand, N):
    L, lib, st = _lib()
    B = near.shape[0]
    t_inv, t = Out((B, N + 1)), Out((B, N + 1))
    dn, df, dr = T(near), T(far), (None if t_rand is None else T(t_rand))
    L.check(lib.mipnerf_sample_along_rays_360(B, N, dn.data_ptr(), df.data_ptr(), None if dr is None else dr.data_ptr(), t_inv.ptr, t.ptr, st),
            "sample_along_rays_360")
    return t_inv.get("t_inv"), t.get("t_samples")


def cast(dev, B, N, deg, contracted, out_dtype, gaussians):
    """mipnerf_cast_ipe_360: rows [B*N, 42 L] (fragments: the flat buffer of whole 256-sample tiles) and, with `gaussians`, (mean, cov)"""
    L, lib, st = _lib()
    t, o, d, r = dev
    M, width = B * N, 2 * f3.NB * (deg[1] - deg[0])
    frag = out_dtype == L.OUT_BF16_FRAGMENTS
    enc = Out((-(-M // 256) * 256 * width,) if frag else (M, width), bf16=out_dtype != L.PREC_FP32)
    mean, cov = (Out((B, N, 3)), Out((B, N, 3, 3))) if gaussians else (None, None)
    L.check(lib.mipnerf_cast_ipe_360(B, N, deg[0], deg[1], contracted, t.data_ptr(), o.data_ptr(), d.data_ptr(), r.data_ptr(), enc.ptr, out_dtype,
                                     mean.ptr if gaussians else None, cov.ptr if gaussians else None, st), "cast_ipe_360")
    rows = enc.get("cast_ipe_360 enc")
    return (rows, mean.get("cast_ipe_360 means"), cov.get("cast_ipe_360 covs")) if gaussians else rows


def gauss(means, covs, deg, contracted, bf16):
    """mipnerf_gauss_360: (rows [M, 42 L], mean [M,3], cov [M,3,3])"""
    L, lib, st = _lib()
    M = means.shape[0]
    dm, dc = T(means), T(covs)
    enc, mo, co = Out((M, 2 * f3.NB * (deg[1] - deg[0])), bf16), Out((M, 3)), Out((M, 3, 3))
    L.check(lib.mipnerf_gauss_360(M, deg[0], deg[1], contracted, dm.data_ptr(), dc.data_ptr(), enc.ptr, L.PREC_BF16 if bf16 else L.PREC_FP32,
                                  mo.ptr, co.ptr, st), "gauss_360")
    return enc.get("gauss_360 enc"), mo.get("gauss_360 means"), co.get("gauss_360 covs")


def lattice(space, deg, out_dtype):
    L, lib, st = _lib()
    la = f3.LATTICE
    width = 2 * f3.NB * (deg[1] - deg[0])
    frag = out_dtype == L.OUT_BF16_FRAGMENTS
    enc = Out((-(-la["count"] // 256) * 256 * width,) if frag else (la["count"], width), bf16=out_dtype != L.PREC_FP32)
    dims, lo, hi = (C.c_int32 * 3)(*la["dims"]), (C.c_float * 3)(*la["lo"]), (C.c_float * 3)(*la["hi"])
    L.check(lib.mipnerf_lattice_ipe_360(dims, lo, hi, la["first"], la["count"], la["cov_scale"], L.SPACES[space], deg[0], deg[1], enc.ptr, out_dtype,
                                        st), "lattice_ipe_360")
    return enc.get("lattice_ipe_360 enc")


class Worst:
    def __init__(self):
        self.worst, self.fails = {}, []

    def check(self, key, got, truth, budget):
        v = f3.worst(got, truth, budget)
        self.worst[key] = max(self.worst.get(key, 0.0), v)
        if not v <= 1.0:
            self.fails.append((key, v))

    def done(self, G, tag):
        print(f"ipe360_forward {tag}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in self.worst.items()))
        G.record(f"ipe360_forward {tag}", **self.worst)
        assert not self.fails, self.fails


def _fragments(flat, M, width, rows, what):
    """a fragment buffer read back through enc360_index's rule: the rows' bits in front, the last sample's row in every padding row"""
    got = f3.rows_of_fragments(flat, M, width)
    assert _same_bits(got[:M], rows), f"{what}: fragments differ from the rows"
    assert np.array_equal(_bits(got[M:]), np.broadcast_to(_bits(rows[M - 1]), got[M:].shape)), f"{what}: padding rows"


@functools.lru_cache(maxsize=None)
def _operands(cls, B, N):
    c = f3.make(cls, B, N)
    _, t = f3.host_sample(c["near"], c["far"], c["t_rand"], N)
    return c, t, f3.frustum_truth(t, c["o"], c["d"], c["r"])


@pytest.mark.parametrize("shape", f3.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cls", f3.CLASSES)
def test_fence_posts(G, cls, shape):
    """stage 1: t_inv against float64 with and without t_rand (which holds 0 and nextafter(1, 0)), a ray with near = far among them;
    t = 1 / t_inv of the kernel's own t_inv to 1 u"""
    B, N = shape
    near, far, t_rand = f3.sampler_operands(_operands(cls, B, N)[0])
    w = Worst()
    for name, tr in (("plain", None), ("jittered", t_rand)):
        t_inv, t = sample(near, far, tr, N)
        pt = f3.posts_truth(near, far, tr, N)
        w.check(f"t_inv {name}", t_inv, pt["t_inv"], f3.posts_budget(pt))
        w.check(f"t {name}", t, 1.0 / t_inv.astype(np.float64), f3.U / np.abs(t_inv.astype(np.float64)) + f3.FLOOR)
    w.done(G, f"posts {cls} {B}x{N}")


@pytest.mark.parametrize("shape", f3.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cls", f3.CLASSES)
def test_gaussians_and_rows_within_their_budgets(G, cls, shape):
    """stages 2, 3 and 5 on the per-direction kernel (fp32 and bf16, with means and covs), then the tiled kernel's fp32 rows, bf16 rows and
    fragments against the same truths and, bit for bit, against the per-direction rows"""
    from mipnerf_pl_amd import _lib as L
    B, N = shape
    M = B * N
    c, t, fr = _operands(cls, B, N)
    dev = (T(t), T(c["o"]), T(c["d"]), T(c["r"]))
    w = Worst()
    gaussians = {}
    for contracted in (0, 1):
        for deg in f3.DEGREES:
            k, width = f"c{contracted} {f3.deg_id(deg)}", 2 * f3.NB * (deg[1] - deg[0])
            rows, mean, cov = cast(dev, B, N, deg, contracted, L.PREC_FP32, True)
            rows16, mean16, cov16 = cast(dev, B, N, deg, contracted, L.PREC_BF16, True)
            assert _same_bits(mean, mean16) and _same_bits(cov, cov16), k
            if contracted not in gaussians:
                gaussians[contracted] = (mean, cov)
                assert _same_bits(cov, cov.swapaxes(-1, -2)), "covariances must be symmetric bit for bit"
                if contracted == 0:
                    a, b = f3.gauss_ratios(mean, cov, fr, f3.C_M, f3.C_V)
                    w.worst["mean"], w.worst["cov"] = a, b
                else:
                    m0, c0 = gaussians[0]
                    fu = f3.fused_truth(m0, fr, f3.MARGIN_N2 / 2)          # from the device's own uncontracted mean
                    out = fu["out"]
                    assert _same_bits(mean[~out], m0[~out]) and _same_bits(cov[~out], c0[~out]), "inside the unit ball nothing changes"
                    a = f3.worst(mean[out], fu["mean"][out], f3.C_MC * f3.U * fu["mag_mean"][out] + f3.FLOOR)
                    b = f3.worst(cov[out], fu["cov"][out], f3.C_VF * f3.U * fu["mag_cov"][out] + f3.FLOOR)
                    w.worst["mean'"], w.worst["fused cov'"] = a, b
                w.fails += [(n, v) for n, v in ((f"{k} mean", a), (f"{k} cov", b)) if not v <= 1.0]
            gm, gc = gaussians[contracted]
            assert _same_bits(mean, gm) and _same_bits(cov, gc), f"{k}: the Gaussians depend on the degrees"
            ft = f3.feature_truth(mean, cov, deg)
            w.check(f"f32 {k}", rows.reshape(B, N, width), ft["f32"], ft["bud_f32"])
            w.check(f"bf16 {k}", rows16.reshape(B, N, width), ft["bf16"], ft["bud_bf16"])
            dead = ft["damp"].reshape(M, width) == 0
            assert np.all(rows[dead] == 0) and np.all(rows16[dead] == 0), k                 # float64's exp underflowed: exactly +-0
            # only the encoding: the tiled kernel where 21 L is a multiple of 8 (the per-direction kernel again where it is not)
            assert _same_bits(cast(dev, B, N, deg, contracted, L.PREC_FP32, False), rows), f"{k}: fp32 rows of the encoding-only route"
            assert _same_bits(cast(dev, B, N, deg, contracted, L.PREC_BF16, False), rows16), f"{k}: bf16 rows of the encoding-only route"
            if f3.tiled(deg):
                _fragments(cast(dev, B, N, deg, contracted, L.OUT_BF16_FRAGMENTS, False), M, width, rows16, k)
    w.done(G, f"{cls} {B}x{N}")


def test_gauss_360_on_the_table(G):
    """stage 4 on the hand-made table (means inside, exactly on and one step outside the unit sphere, out to 400; covariances 0, a
    denormal, 1e-12, 1 and 1e-6 : 1) and on the `far` frusta; its encoding against stage 5"""
    mm, cc = f3.table()
    m0, c0 = f3.host_cast(_operands("far", 2, 129)[1], *[_operands("far", 2, 129)[0][k] for k in ("o", "d", "r")], 0, (0, 1))[:2]
    w = Worst()
    for name, (means, covs) in (("table", (mm, cc)), ("far", (m0.reshape(-1, 3), c0.reshape(-1, 3, 3)))):
        tr = f3.generic_truth(means, covs)
        for deg in ((0, 16), (0, 6)):
            rows, mo, co = gauss(means, covs, deg, 1, False)
            rows16, mo16, co16 = gauss(means, covs, deg, 1, True)
            assert _same_bits(mo, mo16) and _same_bits(co, co16) and _same_bits(co, co.swapaxes(-1, -2))
            keep = ~tr["out"]
            assert _same_bits(mo[keep], means[keep]) and _same_bits(co[keep], covs[keep]), "fp32 n2 <= 1: bit for bit"
            a, b = f3.gauss_ratios(mo, co, tr, f3.C_MC, f3.C_VG)
            w.worst[f"{name} mean'"], w.worst[f"{name} generic cov'"] = a, b
            w.fails += [(n, v) for n, v in ((f"{name} mean'", a), (f"{name} cov'", b)) if not v <= 1.0]
            ft = f3.feature_truth(mo, co, deg)
            w.check(f"{name} f32 {f3.deg_id(deg)}", rows, ft["f32"], ft["bud_f32"])
            w.check(f"{name} bf16 {f3.deg_id(deg)}", rows16, ft["bf16"], ft["bud_bf16"])
            r0, m1, c1 = gauss(means, covs, deg, 0, False)
            assert _same_bits(m1, means) and _same_bits(c1, covs), "contracted = 0 hands the Gaussians through"
            f0 = f3.feature_truth(means, covs, deg)
            w.check(f"{name} f32 uncontracted {f3.deg_id(deg)}", r0, f0["f32"], f0["bud_f32"])
    n2 = f3.n2_fp32(mm)
    exact = np.all(mm == np.array([1, 0, 0], F), -1) | np.all(mm == np.array([0.6, 0.8, 0], F), -1)
    assert exact.sum() == 12 and np.all(n2[exact] == 1) and not f3.generic_truth(mm, cc)["out"][exact].any()
    above = (n2 > 1) & (n2 < 1 + 2.0 ** -20) & np.all(cc == np.eye(3, dtype=F), (1, 2))
    co = gauss(mm, cc, (0, 16), 1, False)[2]
    assert above.sum() == 3 and np.all(np.any(_bits(co[above]) != _bits(cc[above]), (1, 2))), "one step outside: contracted"
    w.done(G, "gauss_360")


@pytest.mark.parametrize("space", ["world", "contracted"])
def test_lattice_rows_and_fragments(G, space):
    """k_lattice_ipe_360_tile on a 5 x 4 x 3 lattice that straddles |z| = 1, a ragged range of it: its Gaussian (lo + i h,
    diag(cov_scale h^2 / 12)) is the host build's (held to float64 here), its rows the bits of mipnerf_gauss_360 on those Gaussians and
    within the budgets of stages 4 and 5, its fragments the rows"""
    from mipnerf_pl_amd import _lib as L
    la = f3.LATTICE
    lm, lc = f3.host_lattice(**la)
    lt = f3.lattice_truth(**la)
    w = Worst()
    w.check("mean", lm, lt["mean"], f3.C_M * f3.U * lt["mag_mean"] + f3.FLOOR)
    w.check("var", np.diagonal(lc, axis1=1, axis2=2), lt["var"], f3.C_V * f3.U * lt["var"] + f3.FLOOR)
    contracted = int(space == "world")
    for deg in ((0, 16), (0, 8)):
        width = 2 * f3.NB * (deg[1] - deg[0])
        want, mo, co = gauss(lm, lc, deg, contracted, False)
        want16 = gauss(lm, lc, deg, contracted, True)[0]
        rows, rows16 = lattice(space, deg, L.PREC_FP32), lattice(space, deg, L.PREC_BF16)
        assert _same_bits(rows, want) and _same_bits(rows16, want16), f"{space} {deg}: not the bits of gauss_360 on the same Gaussians"
        _fragments(lattice(space, deg, L.OUT_BF16_FRAGMENTS), la["count"], width, rows16, f"lattice {space} {deg}")
        if contracted:
            a, b = f3.gauss_ratios(mo, co, f3.generic_truth(lm, lc), f3.C_MC, f3.C_VG)
            w.worst["mean'"], w.worst["generic cov'"] = a, b
            assert a <= 1.0 and b <= 1.0
        ft = f3.feature_truth(mo, co, deg)
        w.check(f"f32 {f3.deg_id(deg)}", rows, ft["f32"], ft["bud_f32"])
        w.check(f"bf16 {f3.deg_id(deg)}", rows16, ft["bf16"], ft["bud_bf16"])
    w.done(G, f"lattice {space}")
