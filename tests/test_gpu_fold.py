"""The bf16 forward kernels run the folded plan (Plan.build(fold_view=True)): inference and training forward-with-save share one packed
stream, whose folded view layer the pack kernel computes from the parameters."""
import numpy as np
import pytest
import torch

from mipnerf_pl_amd.mlp_plan import Arch, Plan, bf16_round, emulate_wave
from oracle import mipnerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


# trainable variants with view directions (gen_mlp_bf16.VARIANTS 0, 1, 3, 5): MipNerf keyword arguments
CASES = [dict(), dict(mlp_net_width=128, mlp_net_width_condition=128), dict(mlp_net_depth=6, mlp_skip_index=3),
         dict(mlp_net_depth_condition=2)]


def _arch(kw):
    return Arch(net_width=kw.get("mlp_net_width", 256), net_width_condition=kw.get("mlp_net_width_condition", 128),
                net_depth=kw.get("mlp_net_depth", 8), skip_index=kw.get("mlp_skip_index", 4),
                net_depth_condition=kw.get("mlp_net_depth_condition", 1))


def _case(arch, B, N, seed):
    rng = np.random.default_rng(seed)
    params = orc.make_params(seed=seed, density_gain=40.0, net_width=arch.net_width, net_width_condition=arch.net_width_condition,
                             net_depth=arch.net_depth, skip_index=arch.skip_index, net_depth_condition=arch.net_depth_condition)
    enc = (rng.uniform(-1, 1, (B, N, 96)) * rng.uniform(0, 1, (1, 1, 96)) ** 2).astype(np.float32)
    vdir = rng.normal(0, 1, (B, 3)).astype(np.float32)
    vdir /= np.linalg.norm(vdir, axis=-1, keepdims=True)
    venc = orc.pos_enc(vdir, 0, 4, True).astype(np.float32)
    return params, enc, venc


@pytest.mark.parametrize("kw", CASES, ids=["v0", "v1", "v3", "v5"])
def test_inference_and_training_forward_agree_bit_for_bit(G, kw):
    """k_mlp_bf16 (no autograd) and k_mlp_bf16_trainfwd (autograd) read the same stream in the same order: same rgb and density bits."""
    arch = _arch(kw)
    params, enc, venc = _case(arch, 6, 64, seed=41)
    model = G.make_model(params, 64, "bf16", **kw)
    e, v = torch.from_numpy(enc).to(DEV), torch.from_numpy(venc).to(DEV)
    rgb, den = model.mlp(e, v)
    assert rgb.requires_grad
    with torch.no_grad():
        rgb2, den2 = model.mlp(e, v)
    assert torch.equal(rgb.detach(), rgb2) and torch.equal(den.detach(), den2)


@pytest.mark.parametrize("kw", CASES, ids=["v0", "v1", "v3", "v5"])
def test_device_forward_equals_folded_emulation(G, kw):
    """The packed folded stream, seen through the kernel: the device forward against the numpy emulation of the folded plan with bf16
    operand rounding (fp32 accumulation order and rare bf16 tie flips are the only differences).  Density never touches the fold.  rgb
    must sit much closer to the folded emulation than to the unfolded one (~2e-3 apart): a device fold off by more than its own
    rounding would not."""
    arch = _arch(kw)
    B, N = 2, 64
    params, enc, venc = _case(arch, B, N, seed=43)
    model = G.make_model(params, N, "bf16", **kw)
    with torch.no_grad():
        rgb, den = model.mlp(torch.from_numpy(enc).to(DEV), torch.from_numpy(venc).to(DEV))
    rgb, den = rgb.cpu().numpy().reshape(B, N, 3), den.cpu().numpy().reshape(B, N)
    flat = np.concatenate([p.ravel() for p in params.values()])
    em = {}
    for fold in (True, False):
        plan = Plan.build(arch, fold_view=fold)
        r_all, d_all = np.zeros_like(rgb), np.zeros_like(den)
        for b in range(B):
            view = np.zeros((32, 32), np.float32)
            view[:, :27] = bf16_round(venc[b])[None]
            for t in range(N // 32):
                r_all[b, 32 * t:32 * t + 32], d_all[b, 32 * t:32 * t + 32] = emulate_wave(plan, flat, bf16_round(enc[b, 32 * t:32 * t + 32]),
                                                                                          view, round_bf16=True)
        em[fold] = (r_all, d_all)
    rms = {f: float(np.sqrt(((rgb - em[f][0]).astype(np.float64) ** 2).mean())) for f in em}
    e_den = float(np.abs(den - em[True][1]).max())
    G.record(f"fold_device_vs_emulation {kw}", rgb_rms_folded=rms[True], rgb_rms_unfolded=rms[False], density_max=e_den)
    assert e_den <= 1e-3 * max(1.0, float(np.abs(den).max()))
    assert rms[True] <= 0.25 * rms[False], rms


def test_fold_is_deterministic_and_graph_equals_eager(G):
    """Re-packing the same parameters gives the same bits, and the captured forward computes what the eager one does."""
    from mipnerf_pl_amd import Rays
    from mipnerf_pl_amd.model import GraphedForward
    import synthetic_inputs as syn
    params = syn.make_params(seed=0, density_gain=40.0)
    m = G.make_model(params, 64, "bf16")
    R = Rays(*[torch.from_numpy(x).to(DEV) for x in syn.synthetic_rays(256, seed=7)])
    with torch.no_grad():
        a = [t.clone() for lvl in m(R, False, True) for t in lvl]
        m.mlp.load_state_dict(m.mlp.state_dict())            # a fresh pack of the same parameters
        b = [t.clone() for lvl in m(R, False, True) for t in lvl]
        gf = GraphedForward(m, 256, True)
        c = [t.clone() for lvl in gf(R) for t in lvl]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(a, c))
