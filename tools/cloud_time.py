#!/usr/bin/env python
"""usage (GPU box): python tools/cloud_time.py -- the matcher cloud at the reference's sizes (504x378 images, 3 views, 100 x 200
candidates per round, a starting cloud of ~100k points):
  fused   one growth round of b3gs_cloud_grow_round (two launches, no host read), wall time per round over blocks of rounds
          closed by one synchronisation
  ref     the reference-shaped round: this project's own torch statements of the same round -- projection, two grid_sample
          patch stacks, the grouped 11x11 convolutions, two torch.unique(dim=0) over the whole cloud and the host reads the
          reference's `if` statements make -- on the same device
Both run in ALTERNATING blocks inside one process, in the manner of tools/ab_interleaved.py (the host is shared: separate runs
cannot resolve a small effect); median and best block per side.  Also: matches per second of triangulate_pair at 200k
matches.  The images are a smooth texture seen through a homography-free identity rig, so that candidates are accepted and the
cloud grows on both sides.  Prints one JSON line."""
import json
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from binocular3dgs_amd import matcher_cloud as mc       # noqa: E402

dev = torch.device("cuda")
W, H, V, SEEDS, SAMPLES, N0 = 504, 378, 3, 100, 200, 100_000
rng = np.random.default_rng(0)
K = np.array([[400.0, 0, 252.0], [0, 400.0, 189.0], [0, 0, 1.0]], np.float32)
c2ws = np.stack([np.eye(4, dtype=np.float32) for _ in range(V)])
c2ws[1, 0, 3], c2ws[2, 1, 3] = 8.0, 6.0
DEPTH = 400.0


def image(v):
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    X = (xs - K[0, 2]) / K[0, 0] * DEPTH + c2ws[v, 0, 3]
    Y = (ys - K[1, 2]) / K[1, 1] * DEPTH + c2ws[v, 1, 3]
    ch = [0.5 + 0.45 * np.sin(0.09 * X + 0.03 * Y + p) * np.cos(0.02 * X - 0.08 * Y) for p in (0.3, 1.1, 2.0)]
    return np.clip(np.round(np.stack(ch, -1) * 255), 0, 255).astype(np.uint8)


imgs_u8 = [torch.from_numpy(image(v)).to(dev) for v in range(V)]
uv0 = np.stack([rng.uniform(0, W - 1, N0), rng.uniform(0, H - 1, N0)], 1)
start = np.stack([(uv0[:, 0] - K[0, 2]) / K[0, 0] * DEPTH, (uv0[:, 1] - K[1, 2]) / K[1, 1] * DEPTH, np.full(N0, DEPTH)], 1).astype(np.float32)
points0 = torch.from_numpy(start).to(dev)
colors0 = torch.zeros((N0, 3), device=dev)
window = mc.ssim_window().to(dev)


# ---- the reference-shaped round, in torch ---------------------------------------------------------------------------------
def project(p, w2c, focal, center):
    q = torch.matmul(w2c[None, :3, :3], p[:, :, None])[..., 0] + w2c[None, :3, 3]
    return q[:, :2] / q[:, 2:] * focal + center


class TorchRound:
    def __init__(self):
        self.points, self.colors = points0.clone(), colors0.clone()
        self.images = torch.stack(imgs_u8).float()
        self.w2c = torch.from_numpy(np.stack([np.linalg.inv(c) for c in c2ws]).astype(np.float32)).to(dev)
        self.focal, self.center = torch.tensor([K[0, 0], K[1, 1]], device=dev), torch.tensor([K[0, 2], K[1, 2]], device=dev)
        r = torch.arange(-5, 6, device=dev)
        oy, ox = torch.meshgrid(r, r, indexing="ij")
        self.offset = torch.stack([ox, oy], -1).reshape(-1, 2).float()
        self.win = window.reshape(1, 1, 11, 11).expand(3, 1, 11, 11).contiguous()

    def patches(self, img, uv):
        grid = (uv.reshape(1, -1, 1, 2) + self.offset[None, None]) * 2 / torch.tensor([W, H], device=dev) - 1.0
        p = F.grid_sample(img.permute(2, 0, 1)[None], grid, align_corners=False)        # [1,3,N,121]
        return p[0].permute(1, 0, 2).reshape(-1, 3, 11, 11)

    def round(self, ref, src, seed_idx, noise):
        cand = (self.points[seed_idx][:, None, :] + noise * 10.0).reshape(-1, 3)
        ri, si = self.images[ref] / 255.0, self.images[src] / 255.0
        ur, us = project(cand, self.w2c[ref], self.focal, self.center), project(cand, self.w2c[src], self.focal, self.center)
        mask = (ur[:, 0] >= 0) & (ur[:, 0] < W) & (ur[:, 1] >= 0) & (ur[:, 1] < H) & (us[:, 0] >= 0) & (us[:, 0] < W) & (us[:, 1] >= 0) & (us[:, 1] < H)
        a, b = self.patches(si, us), self.patches(ri, ur)
        conv = lambda t: F.conv2d(t, self.win, groups=3).reshape(-1, 3)  # noqa: E731
        mu1, mu2 = conv(a), conv(b)
        s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
        ssim = (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))).mean(-1) * mask
        new = cand[ssim >= 0.95]
        if len(new) == 0:                                                              # (host read, as the reference's)
            return
        tmp = torch.cat([self.points, new])
        wh = torch.tensor([W - 1, H - 1], device=dev)
        ones = torch.ones((1, 1, H, W), device=dev)
        sel = []
        for v, img in ((ref, ri), (src, si)):
            uv = project(tmp, self.w2c[v], self.focal, self.center)
            normal = (uv[-len(new):] / wh) * 2 - 1.0
            pm = F.grid_sample(ones, normal.reshape(1, -1, 1, 2), align_corners=False).reshape(-1).bool()
            if pm.sum() == 0:                                                          # (host read)
                return
            _, inv, cnt = torch.unique(torch.round(uv), return_inverse=True, return_counts=True, dim=0)
            sel.append(pm & (cnt[inv][-len(new):] <= 2))
            if v == ref:
                col = F.grid_sample(img.permute(2, 0, 1)[None], normal.reshape(1, -1, 1, 2), align_corners=False)[0, :, :, 0].permute(1, 0)
        keep = sel[0] & sel[1]
        self.points = torch.cat([self.points, new[keep]])
        self.colors = torch.cat([self.colors, col[keep] * 255.0])


def draws(n, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        ref = int(torch.randperm(V, generator=gen)[0])
        src = [v for v in range(V) if v != ref][int(torch.randperm(V - 1, generator=gen)[0])]
        out.append((ref, src, torch.randperm(N0, generator=gen)[:SEEDS].to(dev), torch.randn((SEEDS, SAMPLES, 3), generator=gen).to(dev)))
    return out


BLOCK, BLOCKS = 10, 8
fused = mc.CloudGrower(points0, colors0, imgs_u8, K, c2ws, capacity=N0 + 400_000)
ref_side = TorchRound()
times = {"fused": [], "ref": []}
for blk in range(BLOCKS + 1):                                                          # block 0 warms both sides up
    ds = draws(BLOCK, blk)
    for side in ("fused", "ref"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for ref, src, si, nz in ds:
            if side == "fused":
                fused.round(ref, src, si.to(torch.int32), nz)
            else:
                ref_side.round(ref, src, si, nz)
        torch.cuda.synchronize()
        if blk:
            times[side].append((time.perf_counter() - t0) / BLOCK * 1e6)
n_fused = len(fused.result()[0])
out = {"round_fused_us_median": statistics.median(times["fused"]), "round_fused_us_best": min(times["fused"]),
       "round_ref_shaped_us_median": statistics.median(times["ref"]), "round_ref_shaped_us_best": min(times["ref"]),
       "cloud_after_fused": n_fused, "cloud_after_ref_shaped": len(ref_side.points), "rounds": BLOCK * (BLOCKS + 1)}

# ---- triangulation -----------------------------------------------------------------------------------------------------------
N = 200_000
X = np.stack([rng.uniform(-200, 200, N), rng.uniform(-150, 150, N), rng.uniform(300, 500, N)], 1)
proj = lambda c: (lambda q: (q[:, :2] / q[:, 2:]).astype(np.float32))((X - c[:3, 3]) @ K.T.astype(np.float64))  # noqa: E731
k0, k1 = torch.from_numpy(proj(c2ws[0])).to(dev), torch.from_numpy(proj(c2ws[1])).to(dev)
cams = mc.PinholeView(K, c2ws[0]), mc.PinholeView(K, c2ws[1])
ts = []
for i in range(8):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, _ = mc.triangulate_pair(cams[0], cams[1], k0, k1, imgs_u8[0])
    torch.cuda.synchronize()
    if i >= 2:
        ts.append(time.perf_counter() - t0)
out.update({"triangulate_matches": N, "triangulate_kept": len(p), "triangulate_ms_median": statistics.median(ts) * 1e3,
            "triangulate_matches_per_s": N / statistics.median(ts)})
print(json.dumps(out))
