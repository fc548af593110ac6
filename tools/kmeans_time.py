#!/usr/bin/env python
"""usage (GPU box): python tools/kmeans_time.py [N K] -- milliseconds of one k-means assignment (compress.assign) and of one full
iteration (compress.kmeans(iters=1): two assignments, two distortions, one update, the counts) at N = 1M rows, K = 4096 codes,
D in {7, 12, 48}, INTERLEAVED inside one process (as tools/ab_interleaved.py does: both settings see the same host) with a chunked
torch assignment of the same problem on the same device: argmax of x @ c.T - |c|^2 / 2 in blocks of 65536 rows.  Median and best
round per setting, the achieved share of the 157 TF f32 matrix peak (2 N K D flops per assignment, the padding not counted), the
ratio to torch, and the share of rows on which the two disagree."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import compress            # noqa: E402

N, K = (int(v) for v in sys.argv[1:3]) if len(sys.argv) >= 3 else (1_000_000, 4096)
PEAK = 157.3e12
BLOCK = 65536
dev = torch.device("cuda:0")


def torch_assign(x, c):
    h = 0.5 * (c.double() ** 2).sum(1).float()
    ct = c.t().contiguous()
    return torch.cat([torch.argmax(x[i:i + BLOCK] @ ct - h, dim=1) for i in range(0, x.shape[0], BLOCK)])


for D in (7, 12, 48):
    gen = torch.Generator(device=dev).manual_seed(D)
    x = torch.randn(N, D, device=dev, generator=gen)
    c = x[torch.randperm(N, device=dev, generator=gen)[:K]].contiguous()
    settings = {"hip assign": lambda: compress.assign(x, c), "torch assign": lambda: torch_assign(x, c),
                "hip iteration": lambda: compress.kmeans(x, K, None, iters=1, init=c)}
    with torch.no_grad():
        got = {k: f() for k, f in settings.items()}       # warm-up
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in settings}
        for _ in range(7):
            for k, f in settings.items():
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(dev)
                ms[k].append(1e3 * (time.perf_counter() - t0))
    differ = float((got["hip assign"].long() != got["torch assign"]).double().mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    share = 2.0 * N * K * D / (med["hip assign"] * 1e-3) / PEAK
    print(f"N {N} K {K} D {D}: " + " | ".join(f"{k}: median {med[k]:.2f} best {min(v):.2f} ms" for k, v in ms.items())
          + f" | share of the f32 matrix peak {100 * share:.1f} % | torch / hip {med['torch assign'] / med['hip assign']:.2f}"
          + f" | rows that differ {differ:.2e}")
