"""k_preview_reg_grad on a synthetic 256^3 lattice (random master rows, degree from argv, default 1), three calls without a mask and three
with a ball-shaped mask of about 17 % of the points: the target of rocprofv3 --kernel-trace --pmc (counters in runs of their own), for the
question of DESIGN 4.20 whether the y / z neighbours' lines come from cache.  Prints the bytes the kernel must move."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mipnerf_pl_amd import preview  # noqa: E402

degree = int(sys.argv[1]) if len(sys.argv) > 1 else 1
n, W, used = 256, preview.ROW_HALVES[degree], 1 + 3 * (degree + 1) ** 2
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev)
gen.manual_seed(0)
master = torch.randn(n, n, n, W, device=dev, generator=gen)
grad = torch.zeros_like(master)
x = torch.linspace(-1, 1, n, device=dev)
mask = ((x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) < 0.6857 ** 2).to(torch.uint8).contiguous()
count = int(mask.sum())
lo, hi = (-1.0,) * 3, (1.0,) * 3
for m, c in ((None, n ** 3), (mask, count)):
    for _ in range(3):
        preview.tune_regularise(master, m, (n, n, n), lo, hi, degree, grad, 0.1, 0.1, 0.01, 1e-4, c)
    torch.cuda.synchronize()
    print(f"mask {'none' if m is None else 'ball'}: {c} points, master {n ** 3 * used * 4} B (whole lattice) / {c * used * 4} B (these points), "
          f"grad read + written {2 * c * used * 4} B")
