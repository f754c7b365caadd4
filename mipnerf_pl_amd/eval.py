"""Command line of the test-set evaluation, the reference's eval.py (flags as there, plus --precision and --no-graph):

    python -m mipnerf_pl_amd.eval --ckpt CKPT --data DATA_DIR --out_dir OUT --scale 1|4 [--save_image] [--summa_only]

Loads the checkpoint with MipNeRFSystem.load_from_checkpoint, reads the test split of hparams['dataset_name'] through
datasets.dataset_dict, runs evaluate.evaluate and prints evaluate.summarize_results."""
from __future__ import annotations

import argparse

import torch

from .evaluate import evaluate, summarize_results
from .render_video import add_common_args, load_system


def build_parser():
    p = add_common_args(argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.eval"))
    p.add_argument("--data", help="Path to data.")
    p.add_argument("--save_image", help="whether save predicted image", action="store_true")
    p.add_argument("--summa_only", help="Only summarize results", action="store_true")
    p.add_argument("--scale", help="eval scale", type=int, required=True, choices=[1, 4])
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    system = load_system(args)
    hp = system.hparams
    exp_name = hp["exp_name"]
    if not args.summa_only:
        from .datasets import dataset_dict
        dev = torch.device("cuda", torch.cuda.current_device())
        system = system.to(dev).eval()
        dataset = dataset_dict[hp["dataset_name"]](data_dir=args.data, split="test", white_bkgd=hp["val.white_bkgd"],
                                                  batch_type=hp["val.batch_type"], device=dev)
        evaluate(system, dataset, args.out_dir, exp_name, scale=args.scale, save_image=args.save_image, chunk_size=args.chunk_size,
                 white_bkgd=args.white_bkgd, use_graph=args.use_graph, base_size=args.base_size)
    summary = summarize_results(args.out_dir, [exp_name], args.scale)
    print("PSNR | SSIM | Average")
    print(summary)
    return summary


if __name__ == "__main__":
    main()
