#!/usr/bin/env python
"""usage (GPU box): python tools/mesh_score_time.py [--points 400000] [--max_dist 0.05] -- the time of the nearest distances
between the points sampled on an analytic sphere mesh and a cloud sampled on the same sphere, about `points` per side:
  grid    mesh_tools.nearest_distances: bounding box, cell ids, radix sort, cell table, one thread per query walking shells
          of cells (csrc/meshtools.hip); the grid is rebuilt in every call
  cdist   chunked torch.cdist(a_chunk, b).min(1) capped at max_dist -- what a user would otherwise write
Both run in ALTERNATING blocks inside one process (block 0 warms both up); every block ends in a device synchronise inside the
host clock; median and best block per side.  The two results are compared before anything is timed (cdist computes the
distance by another formula, so the largest difference is reported, not asserted).  Prints one JSON line."""
import argparse
import json
import math
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import mesh_tools                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--points", type=int, default=400000)
ap.add_argument("--max_dist", type=float, default=0.05)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5, help="grid calls per timed block")
ap.add_argument("--chunk", type=int, default=1024, help="queries per cdist call (the temporary is chunk x points floats)")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("mesh_score_time.py measures on the HIP device: none found")
dev = torch.device("cuda")


def sphere_mesh(n_lat):
    """A latitude / longitude mesh of the unit sphere: (vertices float32 [V,3], faces int32 [F,3])."""
    n_lon = 2 * n_lat
    th = torch.linspace(0.0, math.pi, n_lat + 1, device=dev)[1:-1]
    ph = torch.arange(n_lon, device=dev) * (2.0 * math.pi / n_lon)
    ring = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                        torch.cos(th)[:, None].expand(-1, n_lon)], -1).reshape(-1, 3)
    v = torch.cat([ring, torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]], device=dev)]).float()
    i, j = torch.meshgrid(torch.arange(n_lat - 2, device=dev), torch.arange(n_lon, device=dev), indexing="ij")
    p00, p01 = i * n_lon + j, i * n_lon + (j + 1) % n_lon
    p10, p11 = p00 + n_lon, p01 + n_lon
    quads = torch.cat([torch.stack([p00, p10, p01], -1).reshape(-1, 3), torch.stack([p01, p10, p11], -1).reshape(-1, 3)])
    j = torch.arange(n_lon, device=dev)
    top = torch.stack([torch.full_like(j, len(ring)), j, (j + 1) % n_lon], -1)
    last = (n_lat - 2) * n_lon
    bottom = torch.stack([torch.full_like(j, len(ring) + 1), last + (j + 1) % n_lon, last + j], -1)
    return v, torch.cat([quads, top, bottom]).int()


# a mesh of about points / 4 vertices, sampled at a spacing that brings the cloud to about `points`
n_lat = max(8, int(math.sqrt(a.points / 8.0)))
vertices, faces = sphere_mesh(n_lat)
recon = mesh_tools.sample_surface(vertices, faces, 0.6 * math.pi / n_lat)
g = torch.Generator(device=dev).manual_seed(1)
gt = torch.nn.functional.normalize(torch.randn(a.points, 3, device=dev, generator=g), dim=1)


def grid():
    return mesh_tools.nearest_distances(recon, gt, a.max_dist)


def cdist():
    out = torch.empty(recon.shape[0], device=dev)
    for s in range(0, recon.shape[0], a.chunk):
        out[s:s + a.chunk] = torch.cdist(recon[s:s + a.chunk], gt).min(1).values
    return out.clamp_(max=a.max_dist)


d_grid, d_cdist = grid(), cdist()
torch.cuda.synchronize()
max_diff = float((d_grid - d_cdist).abs().max())

times = {"grid": [], "cdist": []}
for blk in range(a.blocks + 1):                                                       # block 0 warms both sides up
    for side in ("grid", "cdist"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if side == "grid":
            for _ in range(a.repeats):
                grid()
        else:
            cdist()
        torch.cuda.synchronize()
        if blk:
            times[side].append((time.perf_counter() - t0) * 1e3 / (a.repeats if side == "grid" else 1))
print(json.dumps({"recon_points": int(recon.shape[0]), "gt_points": int(gt.shape[0]), "max_dist": a.max_dist,
                  "grid": mesh_tools.NearestGrid(gt, a.max_dist).params(),
                  "grid_ms_median": statistics.median(times["grid"]), "grid_ms_best": min(times["grid"]),
                  "cdist_ms_median": statistics.median(times["cdist"]), "cdist_ms_best": min(times["cdist"]),
                  "max_abs_diff": max_diff, "mean_distance": float(d_grid.mean()), "blocks": a.blocks,
                  "grid_repeats_per_block": a.repeats, "cdist_chunk": a.chunk}))
