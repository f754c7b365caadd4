"""bench.py contract on the GPU box: `python bench.py --gpus N` starts N ranks ITSELF (no launcher), the JSON line carries
n_gpus = N; a plain run times the headline alone and can write its outputs; with --full the line carries the headline plus the
train / render sub-records, each with a roofline.  A 1-GPU box cannot run two RCCL
ranks (RCCL refuses two ranks per device), so the plumbing test puts both ranks on cuda:0 over gloo
(MIPNERF_BENCH_SHARE_GPU / MIPNERF_BENCH_BACKEND: test-only knobs)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=timeout,
                          env=env, cwd=REPO)


def test_bench_refuses_world_size_mismatch():
    """A launcher environment that disagrees with --gpus is an error, not a silent 1-rank run."""
    out = _run(["--gpus", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0 and "WORLD_SIZE=2 but --gpus 1" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_bench_self_launches_two_ranks():
    out = _run(["--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--rays", "512", "--samples", "32", "--sustain-seconds", "0", "--preheat-seconds", "0.1"],
               {"MIPNERF_BENCH_SHARE_GPU": "1", "MIPNERF_BENCH_BACKEND": "gloo"})
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1
    assert line["config"]["mode"] == "inference" and line["roofline"]["frac"] > 0
    assert line["per_gpu"] * 2 == pytest.approx(line["value"], rel=1e-6)
    for k in ("train", "render"):
        assert line[k]["n_gpus"] == 2 and line[k]["value"] > 0 and line[k]["roofline"]["frac"] > 0, k
    assert line["render"]["scaling"] == "strong" and line["train"]["scaling"] == "weak"
    assert line["cpu_baseline"] is None          # N = 1 only
    # round 6: the line says who ran -- one entry per rank with its device; here both ranks share cuda:0 and the line says so
    who = line["ranks"]
    assert who["world_size"] == 2 and [r["rank"] for r in who["ranks"]] == [0, 1] and who["backend"] == "gloo"
    assert who["shared_gpu_plumbing_test"] is True and who["distinct_devices"] == 1 and all(r["name"] for r in who["ranks"])
    assert who["train_allreduce_ms"] is not None and who["train_allreduce_ms"] > 0
    assert line["train"]["lightning_route"] is None and "reference_frame" not in line["render"]      # N = 1 only


@pytest.mark.gpu
def test_bench_self_launches_eight_ranks_on_the_shared_gpu():
    """the driver's SCALE run goes to N = 8 and no box with more than one GPU was ever available to the builder.  The
    rank-count-specific host logic -- self-launch under torch.distributed.run with 8 ranks, the eight contiguous ray shards of the
    640,000-ray frame (80,000 each) and their gather, eight flat-gradient all-reduces per training step with 1 / 8 folded into Adam, max over
    ranks of the timed regions -- runs here with all eight ranks on cuda:0 over gloo (RCCL refuses two ranks per device)."""
    out = _run(["--full", "--gpus", "8", "--steps", "2", "--warmup", "1", "--rays", "256", "--samples", "32", "--sustain-seconds", "0", "--preheat-seconds", "0.05"],
               {"MIPNERF_BENCH_SHARE_GPU": "1", "MIPNERF_BENCH_BACKEND": "gloo"}, timeout=1500)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 8 and line["steps"] == 2
    assert line["per_gpu"] * 8 == pytest.approx(line["value"], rel=1e-6)
    for k in ("train", "render"):
        assert line[k]["n_gpus"] == 8 and line[k]["value"] > 0 and line[k]["roofline"]["frac"] > 0, k
    assert line["train"]["scaling"] == "weak" and line["render"]["scaling"] == "strong"
    assert line["train"]["config"]["global_batch_rays"] == 8 * 256, line["train"]["config"]
    assert line["render"]["config"]["rays_per_gpu_max"] == 80000 and line["render"]["config"]["frame_rays"] == 640000, line["render"]["config"]
    assert line["cpu_baseline"] is None and "scale_model" not in line          # N = 1 only


@pytest.mark.gpu
def test_bench_single_gpu_line():
    out = _run(["--full", "--steps", "3", "--warmup", "1", "--rays", "512", "--samples", "32", "--sustain-seconds", "0.2", "--ceiling-seconds", "0.4", "--preheat-seconds", "0.2"], {})
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["metric"] == "ray-samples/sec" and line["dtype"] == "bf16"
    assert line["cpu_baseline"]["kind"] in ("reference", "port") and line["cpu_baseline"]["value"] > 0
    assert line["sustained"]["value"] > 0 and "train" in line and "render" in line
    assert line["train"]["config"]["hip_graph"] is True and line["train"]["config"]["hip_graph_capture_error"] is None
    assert line["train"]["ranks"]["ms_per_step_min"] > 0
    # round 6: who ran; the step an unmodified train.py executes (Lightning's automatic optimisation), routed onto the one-call native step;
    # the render record is not rendered for N = 32 against the reference's frame (its golden is N = 128)
    assert line["ranks"]["world_size"] == 1 and line["ranks"]["distinct_devices"] == 1 and line["ranks"]["ranks"][0]["compute_units"] == 256
    lr = line["train"]["lightning_route"]
    assert lr["routed_onto_native_step"] is True and 0 < lr["ms_per_step"] <= lr["per_stage_autograd_ms_per_step"] * 1.05, lr
    # round 3: the MFMA ceiling of THIS chip and the fp32 configs[3] forward travel in the same line
    assert 0.3 < line["ceiling"]["lds_fed"] <= line["ceiling"]["register_fed"] * 1.05 < 1.1, line["ceiling"]
    assert 0.3 < line["ceiling"]["lds_and_dma_fed"] <= line["ceiling"]["lds_fed"] * 1.05, line["ceiling"]   # + the L2 -> LDS weight stream
    assert 0.2 < line["ceiling"]["lds_dma_and_store_fed"] <= line["ceiling"]["lds_and_dma_fed"] * 1.05, line["ceiling"]   # + the T-block stores
    assert line["fp32"]["dtype"] == "fp32" and line["fp32"]["roofline"]["kernel"].startswith("k_mlp_f32r") and line["fp32"]["roofline"]["frac"] > 0.3
    # round 4: the stated expectation for the 1 / 2 / 4 / 8 curve, from this run's 1-GPU numbers + a 1-rank RCCL all-reduce measured here
    sm = line["scale_model"]
    assert sm["measured"] is False                                # a written-down expectation, never to be read as a measurement
    assert sm["measured_inputs"]["train_ms_per_step_1gpu"] == line["train"]["ms_per_step"]
    assert sm["measured_inputs"]["allreduce_1rank_rccl_ms"] is not None and 0 < sm["measured_inputs"]["allreduce_1rank_rccl_ms"] < 5, sm
    assert sm["predicted"]["1"]["train_allreduce_ms"] == 0 and sm["predicted"]["8"]["train_allreduce_ms"] > sm["predicted"]["2"]["train_allreduce_ms"] > 0
    assert 0.5 < sm["predicted"]["8"]["train_weak_efficiency"] < 1 and 0.5 < sm["predicted"]["8"]["render_strong_efficiency"] <= 1
    # ... and the same batch through the unbounded-scene model (configs[3] says "360 unbounded")
    assert line["fp32"]["unbounded"].get("finite") is True and line["fp32"]["unbounded"]["frac"] > 0.3, line["fp32"]["unbounded"]
    # round 4: ... and in bf16 (k_pre_gemm + trunk kernel): several times faster than its fp32 forward, close to its frame
    ub = line["fp32"]["unbounded"]["bf16"]
    assert ub.get("finite") is True and ub["frac"] > 0.25 and ub["psnr_vs_fp32_frame_db"] > 45, ub
    assert ub["ms_per_step"] < 0.4 * line["fp32"]["unbounded"]["ms_per_step"], (ub, line["fp32"]["unbounded"])


@pytest.mark.gpu
def test_bench_plain_line_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """Without --full: the headline alone (no sub-record, no roofline re-run, no ceiling, no CPU baseline), exactly --steps timed steps, and
    --dump-outputs writes the last timed step's per-level outputs -- the same bits on a second run with the same arguments."""
    import numpy as np
    B, N = 512, 32
    lines = []
    for run in ("a", "b"):
        out = _run(["--gpus", "1", "--steps", "4", "--warmup", "1", "--rays", str(B), "--samples", str(N), "--preheat-seconds", "0.1",
                    "--dump-outputs", str(tmp_path / run)], {}, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    line = lines[0]
    assert line["metric"] == "ray-samples/sec" and line["unit"] == "ray-samples/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 4 and line["warmup"] == 1 and line["config"]["mode"] == "inference" and line["config"]["hip_graph"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(B * N * 2 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["roofline"] is None and line["cpu_baseline"] is None and "sustained" not in line and "ceiling" not in line
    assert not {"train", "render", "fp32", "trained_field", "variants", "scale_model"} & set(line)
    shapes = {"rgb": (B, 3), "distance": (B,), "acc": (B,), "weights": (B, N), "t_samples": (B, N + 1)}
    want = sorted(f"level{lvl}_{k}.npy" for lvl in range(2) for k in shapes)
    assert sorted(os.listdir(tmp_path / "a")) == want and sorted(os.listdir(tmp_path / "b")) == want
    for name in want:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and a.shape == shapes[name[7:-4]] and np.isfinite(a).all(), name
        assert np.array_equal(a, b), name


@pytest.mark.gpu
def test_train_step_collective_path_on_a_one_rank_rccl_communicator():
    """the data-parallel form of the training step (graph A = forward + backward, gradient all-reduce on the
    process group's RCCL communicator, graph B = Adam + re-pack) had only ever run over gloo.  A 1-rank RCCL communicator is
    legal: MIPNERF_FORCE_COLLECTIVE_PATH=1 drives exactly that sequence on the 1-GPU box, and the run must agree with the
    single-graph form (the all-reduce of one rank is the identity, grad_scale = 1)."""
    code = r'''
import json, os, sys, torch
sys.path.insert(0, os.getcwd())
import torch.distributed as dist
import synthetic_inputs as syn
from mipnerf_pl_amd import Rays
from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
from mipnerf_pl_amd.train_graph import GraphedTrainStep
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
forced = os.environ.get("MIPNERF_FORCE_COLLECTIVE_PATH") == "1"
if forced:
    dist.init_process_group("nccl", rank=0, world_size=1)
B, N = 512, 64
rays = syn.synthetic_rays(B, seed=3, multiscale=True)
params = syn.make_params(seed=0, density_gain=40.0)
hp = dict(DEFAULT_HPARAMS); hp.update({"nerf.num_samples": N, "train.randomized": False, "optimizer.lr_init": 1e-3,
                                       "optimizer.lr_delay_steps": 0})
system = MipNeRFSystem(hp, precision="bf16")
system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()})
system = system.to(dev)
system.fused_adam = True
(opt,), (sch,) = system.configure_optimizers()
g = GraphedTrainStep(system, opt, B, dev, use_graph=True)
g.time_allreduce = True
for dst, src in zip(g.rays, rays):
    dst.copy_(torch.from_numpy(src))
g.gt.copy_(torch.rand(B, 3, generator=torch.Generator().manual_seed(1)))
losses = []
for it in range(7):
    losses.append(float(g()[0]))
    sch["scheduler"].step()
    if it == 0:
        torch.cuda.synchronize()
        g.allreduce_stats()          # the first all-reduce creates the RCCL communicator (hundreds of ms): not a step cost
torch.cuda.synchronize()
ar = g.allreduce_stats()
p = torch.cat([q.detach().reshape(-1) for q in system.mip_nerf.parameters()])
print(json.dumps({"losses": losses, "collective": g.collective, "use_graph": g.use_graph, "graphs": len(g._graphs or ()),
                  "allreduce_ms": ar[0], "allreduce_n": ar[1], "psum": float(p.double().sum()), "pabs": float(p.double().abs().sum()),
                  "backend": dist.get_backend() if forced else None}))
if forced:
    dist.destroy_process_group()
'''
    res = {}
    for forced in ("0", "1"):
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
        import socket
        with socket.socket() as sk:          # a free port for the 1-rank rendezvous
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env.update({"MIPNERF_FORCE_COLLECTIVE_PATH": forced, "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
        assert out.returncode == 0, out.stderr[-3000:]
        res[forced] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    a, b = res["0"], res["1"]
    assert a["collective"] is False and a["graphs"] == 1 and a["use_graph"]
    assert b["collective"] is True and b["graphs"] == 2 and b["use_graph"] and b["backend"] == "nccl"
    assert b["allreduce_n"] == 6 and b["allreduce_ms"] is not None and 0 < b["allreduce_ms"] < 50, b
    assert a["losses"] == b["losses"], (a["losses"], b["losses"])          # same kernels, identity all-reduce: bit-identical trajectories
    assert a["psum"] == b["psum"] and a["pabs"] == b["pabs"]
    assert a["losses"][-1] < a["losses"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("same_xcd,flavour", [(1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (0, 0), (0, 1), (0, 3)])
def test_handoff_probe_protocols_deliver_every_word(same_xcd, flavour):
    """mipnerf_handoff_probe (milestone 1 of the layer pipeline): every CU -> CU protocol hands all 128 pairs' tiles over
    with no wrong 16-byte word and no timed-out poll, with and without MFMA work beside the transfer; the fence-free protocols (2, 4)
    are only defined between workgroups of one XCD."""
    import ctypes as C
    import torch
    from mipnerf_pl_amd import _lib as L
    torch.cuda.init()
    st = torch.cuda.current_stream().cuda_stream
    for mfma in (0, 64):
        out = (C.c_double * 6)()
        rc = L.diag_lib().mipnerf_handoff_probe(same_xcd, flavour, 48, 2, 131072, mfma, 1, out, st)
        assert rc == 0, L.diag_lib().mipnerf_diag_last_error()
        assert out[4] == 0 and out[5] == 0, (list(out), mfma)      # wrong words, timed-out polls
        assert out[0] > 50.0                                      # GB/s aggregate: it moved


@pytest.mark.gpu
def test_collective_paths_hold_up_over_200_steps_on_a_one_rank_rccl_communicator():
    """VERDICT r03 #5b / 5c: the data-parallel training step (graph A -> RCCL all-reduce -> graph B) replayed 200 times on a 1-rank
    RCCL communicator: device memory flat after the first steps (no event / graph / work-handle leak), the all-reduce event list bounded
    and its mean sane; and the multi-GPU rendering gather (parallel.gather_rendered) through the same communicator equals the local
    tensor -- also for an empty shard."""
    code = r'''
import json, os, sys, torch
sys.path.insert(0, os.getcwd())
import torch.distributed as dist
import synthetic_inputs as syn
from mipnerf_pl_amd.parallel import gather_rendered, shard_bounds
from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
from mipnerf_pl_amd.train_graph import GraphedTrainStep
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
B, N = 256, 32
rays = syn.synthetic_rays(B, seed=3, multiscale=True)
params = syn.make_params(seed=0, density_gain=40.0)
hp = dict(DEFAULT_HPARAMS); hp.update({"nerf.num_samples": N, "train.randomized": True, "optimizer.lr_init": 1e-3, "optimizer.lr_delay_steps": 0})
system = MipNeRFSystem(hp, precision="bf16")
system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()})
system = system.to(dev)
system.fused_adam = True
(opt,), (sch,) = system.configure_optimizers()
g = GraphedTrainStep(system, opt, B, dev, use_graph=True)
g.time_allreduce = True
for dst, src in zip(g.rays, rays):
    dst.copy_(torch.from_numpy(src))
g.gt.copy_(torch.rand(B, 3, generator=torch.Generator().manual_seed(1)))
mem, losses = [], []
for it in range(200):
    losses.append(float(g()[0]))
    sch["scheduler"].step()
    if it in (19, 99, 199):
        torch.cuda.synchronize()
        mem.append((torch.cuda.memory_allocated(), torch.cuda.memory_reserved()))
n_events = len(g._ar_events)
ar = g.allreduce_stats()
# rendering: the gather of per-ray outputs through the 1-rank communicator
x = torch.rand(1000, 3, device=dev)
y = gather_rendered(x, 1000, force_collective=True)
z = gather_rendered(x[:0], 0, force_collective=True)
print(json.dumps({"mem": mem, "n_events": n_events, "allreduce_ms": ar[0], "allreduce_n": ar[1], "events_after": len(g._ar_events),
                  "collective": g.collective, "graphs": len(g._graphs or ()), "finite": bool(torch.isfinite(torch.tensor(losses)).all()),
                  "loss0": losses[0], "loss199": losses[-1], "gather_equal": bool(torch.equal(x, y)) and y.data_ptr() != x.data_ptr(),
                  "gather_empty": list(z.shape), "bounds": shard_bounds(1000, 0, 1)}))
dist.destroy_process_group()
'''
    import socket
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env.update({"MIPNERF_FORCE_COLLECTIVE_PATH": "1", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert r["collective"] is True and r["graphs"] == 2 and r["finite"] and r["loss199"] < r["loss0"]
    assert r["mem"][0] == r["mem"][1] == r["mem"][2], r["mem"]                 # flat from step 20 to step 200
    assert r["n_events"] == 200 and r["allreduce_n"] == 200 and r["events_after"] == 0 and 0 < r["allreduce_ms"] < 50, r
    assert r["gather_equal"] and r["gather_empty"] == [0, 3] and r["bounds"] == [0, 1000]
