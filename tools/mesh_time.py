#!/usr/bin/env python
"""usage (GPU box): python tools/mesh_time.py [--views 24] [--resolution 256] -- the time to fuse N views of 504x378 (the
working size of an LLFF scene) into a resolution^3 TSDF volume and to extract the mesh, on an analytic sphere seen from a
ring of cameras:
  fused   TsdfVolume.integrate: one b3gs_tsdf_integrate_batch launch per 8 views (csrc/mesh.hip), then TsdfVolume.extract
          (six launches and one host read of two words)
  torch   the same integration as device torch statements, view by view over the whole volume -- what a user would otherwise
          write (about thirty full-volume passes per view); it has no extraction
Both integrations run in ALTERNATING blocks inside one process (block 0 warms both up); every block ends in a device
synchronise inside the host clock; median and best block per side.  The two volumes are compared before anything is timed.
Prints one JSON line."""
import argparse
import json
import math
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import mesh                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=24)
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=10, help="fused fusions (and extractions) per timed block")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("mesh_time.py measures on the HIP device: none found")
dev = torch.device("cuda")
W, H, FOCAL, RADIUS, DIST = 504, 378, 420.0, 1.0, 4.0
RES, N = a.resolution, a.views
VOXEL = 3.0 / RES
TRUNC, NEAR, ALPHA_MIN = 4.0 * VOXEL, 0.2, 0.5


def scene():
    """N cameras on a ring of radius DIST around the unit sphere at the origin, looking at it: table [N,14] and per view
    the analytic z-depth * alpha, alpha (1 on the sphere, 0 elsewhere) and a colour image, on the device."""
    table = np.zeros((N, 14), np.float32)
    depths, alphas, colours = [], [], []
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    dc = torch.stack([(u - (0.5 * W - 0.5)) / FOCAL, (v - (0.5 * H - 0.5)) / FOCAL, torch.ones_like(u)], -1)
    for k in range(N):
        th = 2.0 * math.pi * k / N
        centre = np.array([DIST * math.sin(th), 0.3 * math.sin(3 * th), -DIST * math.cos(th)])
        zc = -centre / np.linalg.norm(centre)
        xc = np.cross([0.0, 1.0, 0.0], zc)
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])                  # world -> camera
        table[k, :9], table[k, 9:12], table[k, 12:] = R.reshape(9), -R @ centre, FOCAL
        dw = dc @ torch.from_numpy(R).to(dev)
        oc = torch.from_numpy(centre).to(dev)
        qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), float(centre @ centre) - RADIUS ** 2
        disc = qb * qb - 4 * qa * qc
        hit = disc > 0
        z = torch.where(hit, (-qb - torch.sqrt(disc.clamp_min(0))) / (2 * qa), torch.zeros_like(qa))
        alpha = hit.float()
        depths.append((z.float() * alpha).contiguous())
        alphas.append(alpha.contiguous())
        colours.append(torch.stack([alpha * 0.8, alpha * (0.2 + 0.6 * k / N), 1.0 - alpha * 0.5]).contiguous())
    return table, depths, alphas, colours


table, depths, alphas, colours = scene()
vol = mesh.TsdfVolume([-1.5] * 3, [1.5] * 3, VOXEL, TRUNC, device=dev)
assert vol.dims == (RES, RES, RES), vol.dims


def fused():
    vol.reset()
    vol.integrate(table, depths, alphas, colours, alpha_min=ALPHA_MIN, near=NEAR)


axis = vol.origin[0] + (torch.arange(RES, device=dev, dtype=torch.float32) + 0.5) * VOXEL
PX, PY, PZ = axis[None, None, :], axis[None, :, None], axis[:, None, None]
t_tsdf, t_w, t_rgb = torch.ones_like(vol.tsdf), torch.zeros_like(vol.weight), torch.zeros((3,) + tuple(vol.tsdf.shape), device=dev)


def torch_statements():
    """The statements of b3gs_tsdf_integrate_batch (include/b3gs_raster.h), each a device torch call over the whole volume."""
    t_tsdf.fill_(1.0)
    t_w.zero_()
    t_rgb.zero_()
    for k in range(N):
        c = table[k].tolist()
        x = c[0] * PX + c[1] * PY + c[2] * PZ + c[9]
        y = c[3] * PX + c[4] * PY + c[5] * PZ + c[10]
        z = c[6] * PX + c[7] * PY + c[8] * PZ + c[11]
        uf = torch.round(c[12] * (x / z) + (0.5 * W - 0.5))
        vf = torch.round(c[13] * (y / z) + (0.5 * H - 0.5))
        ok = (z > NEAR) & (uf >= 0) & (uf <= W - 1) & (vf >= 0) & (vf <= H - 1)
        pix = torch.where(ok, vf * W + uf, torch.zeros_like(uf)).long()
        al = alphas[k].reshape(-1)[pix]
        ok &= al >= ALPHA_MIN
        sdf = depths[k].reshape(-1)[pix] / al - z
        ok &= sdf >= -TRUNC
        val = torch.clamp(sdf / TRUNC, max=1.0)
        wn = t_w + 1.0
        t_tsdf.copy_(torch.where(ok, (t_tsdf * t_w + val) / wn, t_tsdf))
        for ch in range(3):
            t_rgb[ch].copy_(torch.where(ok, (t_rgb[ch] * t_w + colours[k][ch].reshape(-1)[pix]) / wn, t_rgb[ch]))
        t_w.copy_(torch.where(ok, wn, t_w))


# the two sides compute the same volume (torch fuses nothing here, but its division and rounding are the same IEEE operations)
fused()
torch_statements()
torch.cuda.synchronize()
same_weight = bool((vol.weight == t_w).all())
tsdf_diff = float((vol.tsdf - t_tsdf).abs().max())
rgb_diff = float((vol.rgb - t_rgb.permute(1, 2, 3, 0)).abs().max())

times = {"fused": [], "torch": [], "extract": []}
for blk in range(a.blocks + 1):                                                        # block 0 warms every side up
    for side in ("fused", "torch", "extract"):
        if side == "extract":
            fused()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if side == "fused":
            for _ in range(a.repeats):
                fused()
        elif side == "torch":
            torch_statements()
        else:
            for _ in range(a.repeats):
                out = vol.extract()
        torch.cuda.synchronize()
        if blk:
            times[side].append((time.perf_counter() - t0) * 1e3 / (1 if side == "torch" else a.repeats))
print(json.dumps({"volume": list(vol.dims), "views": N, "image": [W, H],
                  "fused_ms_median": statistics.median(times["fused"]), "fused_ms_best": min(times["fused"]),
                  "torch_statements_ms_median": statistics.median(times["torch"]), "torch_statements_ms_best": min(times["torch"]),
                  "extract_ms_median": statistics.median(times["extract"]), "extract_ms_best": min(times["extract"]),
                  "vertices": int(out[0].shape[0]), "triangles": int(out[2].shape[0]),
                  "same_weight": same_weight, "tsdf_max_abs_diff": tsdf_diff, "rgb_max_abs_diff": rgb_diff,
                  "blocks": a.blocks, "fused_repeats_per_block": a.repeats}))
