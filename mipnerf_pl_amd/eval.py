"""Command line of the test-set evaluation, the reference's eval.py (flags as there, plus --precision and --no-graph):

    python -m mipnerf_pl_amd.eval --ckpt CKPT --data DATA_DIR --out_dir OUT --scale 1|4 [--save_image] [--summa_only]

For a checkpoint of a captured scene (`dataset_name` llff / realdata360; `--scale 1`) the defaults follow the checkpoint and the data:
`--factor` its `factor`, `--white_bkgd` its `val.white_bkgd`, `--base_size` the data set's own (w, h), so the images land in `1/`.

Loads the checkpoint with MipNeRFSystem.load_from_checkpoint, reads the test split of hparams['dataset_name'] through
datasets.dataset_dict, runs evaluate.evaluate and prints evaluate.summarize_results."""
from __future__ import annotations

import argparse

import torch

from .evaluate import distorted_frames, evaluate, summarize_results
from .render_video import (add_common_args, cli_ladder, cli_occupancy, cli_proposal, cli_span_samples, flag_given, is_scene360, load_system,
                           refuse_adaptive_without_cull, refuse_proposal_without_grid, refuse_scene360_proposal, refuse_tighten_without_cull,
                           refuse_unbounded_cull)


def build_parser():
    p = add_common_args(argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.eval"))
    p.add_argument("--data", help="Path to data.")
    p.add_argument("--save_image", help="whether save predicted image", action="store_true")
    p.add_argument("--summa_only", help="Only summarize results", action="store_true")
    p.add_argument("--scale", help="eval scale", type=int, required=True, choices=[1, 4])
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    refuse_tighten_without_cull(args)
    refuse_adaptive_without_cull(args)
    refuse_proposal_without_grid(args)
    system = load_system(args)
    refuse_unbounded_cull(args, system)
    refuse_scene360_proposal(args, system)
    ladder = cli_ladder(args, system)
    hp = system.hparams
    exp_name = hp["exp_name"]
    if not args.summa_only:
        from .datasets import dataset_dict
        dev = torch.device("cuda", torch.cuda.current_device())
        system = system.to(dev).eval()
        scene360 = is_scene360(hp)
        kw = {"factor": args.factor if args.factor is not None else int(hp.get("factor", 4))} if scene360 else {}
        dataset = dataset_dict[hp["dataset_name"]](data_dir=args.data, split="test", white_bkgd=hp["val.white_bkgd"],
                                                  batch_type=hp["val.batch_type"], device=dev, **kw)
        white_bkgd, base_size = args.white_bkgd, args.base_size
        if scene360 and not flag_given(argv, "--white_bkgd"):
            white_bkgd = bool(hp["val.white_bkgd"])
        if scene360 and not flag_given(argv, "--base_size"):
            base_size = (dataset.w, dataset.h)
        occupancy = cli_occupancy(args, system, (dataset[i][0] for i in range(len(dataset))), distorted=distorted_frames(dataset))
        proposal = cli_proposal(args, system, (dataset[i][0] for i in range(len(dataset))), distorted=distorted_frames(dataset))
        evaluate(system, dataset, args.out_dir, exp_name, scale=args.scale, save_image=args.save_image, chunk_size=args.chunk_size,
                 white_bkgd=white_bkgd, use_graph=args.use_graph, base_size=base_size, occupancy=occupancy, tighten=args.cull_tighten,
                 span_samples=cli_span_samples(args, system) if args.cull else None, adaptive=args.cull_adaptive, ladder=ladder,
                 proposal=proposal)
    summary = summarize_results(args.out_dir, [exp_name], args.scale)
    print("PSNR | SSIM | Average")
    print(summary)
    return summary


if __name__ == "__main__":
    main()
