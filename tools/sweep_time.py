#!/usr/bin/env python
"""usage (GPU box): python tools/sweep_time.py -- the plane-sweep matcher at the working size of an LLFF scene (504x378, 3 views,
stride 2, D = 128), on synthetic images of the generator of tests/sweep_ref.py:
  fused   one b3gs_sweep_match_pair call per view pair (five launches, both directions, no host read)
  ref     a reference-shaped version of the same statements in torch on the same device: the host loops over the hypotheses,
          warps the other view's gray with grid_sample, forms the ZNCC of every 7x7 window with avg_pool2d and keeps the running
          best, runner-up-outside-k+-1 candidates and neighbour scores as image-sized tensors (score only: no parabola, no
          left/right check, no compaction -- it does LESS than the fused call)
Both run in ALTERNATING blocks inside one process, as tools/cloud_time.py does; median and best block per side.  Prints one
JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sweep_ref as sr                                    # noqa: E402
from binocular3dgs_amd import sweep_matcher as sm         # noqa: E402

dev = torch.device("cuda")
W, H, D, STRIDE = 504, 378, 128, 2
sc = sr.make_scene(W=W, H=H, baseline=2.4, toe_in=True)
images = [torch.from_numpy(sr.render(sc, v)).to(dev) for v in range(3)]
params = sm.SweepParams(stride=STRIDE, hypotheses=D)
PAIRS = ((0, 1), (0, 2), (1, 2))
plans = {p: sm.pair_plan(sc.K, sc.c2ws[p[0]], sc.c2ws[p[1]], sc.near, sc.far, D) for p in PAIRS}
dev_plans = {p: (torch.from_numpy(pl.homographies).to(dev), torch.from_numpy(pl.proj).to(dev)) for p, pl in plans.items()}


def fused():
    return [sm.launch_pair(images[a], images[b], *dev_plans[(a, b)], plans[(a, b)], sc.near, sc.far, params) for a, b in PAIRS]


def gray(img):
    c = img.to(torch.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).float()


ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
pix = torch.stack([xs, ys, torch.ones_like(xs)], -1)


def ref_direction(ga, gb, hs):
    pool = lambda t: F.avg_pool2d(t[None, None], 7, stride=1)[0, 0][::STRIDE, ::STRIDE]  # noqa: E731
    ma, maa = pool(ga), pool(ga * ga)
    best = torch.full_like(ma, -2.0)
    best_k = torch.zeros_like(ma, dtype=torch.int64)
    vol = []
    for k in range(D):
        q = pix @ hs[k].T
        uv = q[..., :2] / q[..., 2:]
        grid = torch.stack([uv[..., 0] / (W - 1) * 2 - 1, uv[..., 1] / (H - 1) * 2 - 1], -1)
        wb = F.grid_sample(gb[None, None], grid[None], align_corners=True, padding_mode="zeros")[0, 0]
        inside = ((grid.abs() <= 1).all(-1) & (q[..., 2] > 0)).float()
        mb, mbb, mab, ok = pool(wb), pool(wb * wb), pool(ga * wb), pool(inside) > 0.999
        s = (mab - ma * mb) / torch.sqrt(((maa - ma * ma) * (mbb - mb * mb)).clamp_min(1e-6))
        s = torch.where(ok, s, torch.full_like(s, -2.0))
        vol.append(s)
        better = s > best
        best, best_k = torch.where(better, s, best), torch.where(better, torch.full_like(best_k, k), best_k)
    vol = torch.stack(vol)
    away = (torch.arange(D, device=dev)[:, None, None] - best_k[None]).abs() > 1
    second = torch.where(away, vol, torch.full_like(vol, -2.0)).amax(0)
    return (best >= params.min_score) & ~(second > best - params.margin), best_k


def ref():
    out = []
    for a, b in PAIRS:
        ga, gb = gray(images[a]), gray(images[b])
        hs = dev_plans[(a, b)][0]
        out.append((ref_direction(ga, gb, hs[0]), ref_direction(gb, ga, hs[1])))
    return out


BLOCKS = 5
times = {"fused": [], "ref": []}
for blk in range(BLOCKS + 1):                                                          # block 0 warms both sides up
    for side, fn in (("fused", fused), ("ref", ref)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        if blk:
            times[side].append((time.perf_counter() - t0) * 1e3)
matches = int(sum(int(r[3].sum()) for r in fused()))
print(json.dumps({"size": [W, H], "views": 3, "stride": STRIDE, "hypotheses": D, "nodes_per_view": sm.node_count(W, H, STRIDE),
                  "fused_ms_median": statistics.median(times["fused"]), "fused_ms_best": min(times["fused"]),
                  "ref_shaped_ms_median": statistics.median(times["ref"]), "ref_shaped_ms_best": min(times["ref"]),
                  "matches_all_pairs": matches, "blocks": BLOCKS}))
