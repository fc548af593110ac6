#!/usr/bin/env python
"""usage (GPU box): python tools/texture_time.py [--resolution 256] -- the device time of the mesh texture calls
(csrc/texture.hip) on the sphere-and-slab mesh of tools/simplify_time.py simplified at 2 and at 4 voxels, 8 orbit views at
800 x 600, atlases that fit 2048^2 and 4096^2 (mesh_texture.atlas_for).  accumulate (b3gs_mesh_texture_accumulate_batch, the 8
views in one call, the rasterizer's outputs made once outside the window), finalize (b3gs_mesh_texture_finalize) and the
textured resolve (b3gs_mesh_resolve_textured_batch, 8 views) are timed separately with device events around `repeats` calls; the
sides run in ALTERNATING blocks in one process (block 0 warms all of them up); median and best block per side.  Beside each
time, the bytes the call must move at the least -- accumulate: the accumulator read and written, 32 bytes per texel; finalize:
the accumulator read and the texture written, 19; resolve: the visibility word read and the four outputs written, 28 per pixel --
divided by the median: a floor on the achieved rate, to hold against the copy rate of tools/stream_rates.py from the same
session.  Nothing is asserted about speed.  One JSON line."""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, mesh, mesh_texture, mesh_tools       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3, help="calls per timed block and stage")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("texture_time.py measures on the HIP device: none found")
dev = torch.device("cuda")
RES, W, H = a.resolution, 800, 600
VOXEL = 3.0 / RES
TRUNC = 4.0 * VOXEL

vol = mesh.TsdfVolume([-1.5] * 3, [1.5] * 3, VOXEL, TRUNC, device=dev)
axis = vol.origin[0] + (torch.arange(RES, device=dev, dtype=torch.float32) + 0.5) * VOXEL
px, py, pz = axis[None, None, :], axis[None, :, None], axis[:, None, None]
sphere = torch.sqrt(px * px + (py - 0.1) ** 2 + pz * pz) - 0.8
slab = torch.maximum((py + 0.9).abs() - 0.2, torch.maximum(px.abs(), pz.abs()) - 1.3)
vol.tsdf.copy_(torch.clamp(torch.minimum(sphere, slab) / TRUNC, -1.0, 1.0))
vol.weight.fill_(1.0)
vol.rgb.copy_(torch.stack(torch.broadcast_tensors(px / 3 + 0.5, py / 3 + 0.5, pz / 3 + 0.5), -1))
raw = vol.extract()
meshes = {2: mesh_tools.simplify(*raw, 2.0 * VOXEL), 4: mesh_tools.simplify(*raw, 4.0 * VOXEL)}


def orbit(n, radius, fx):
    rows = np.zeros((n, 14), np.float32)
    for k in range(n):
        t = 2.0 * np.pi * k / n + 0.3
        eye = np.array([radius * np.sin(t), -0.6 * radius, -radius * np.cos(t)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        rows[k, :9], rows[k, 9:12], rows[k, 12:] = R.reshape(9), -R @ eye, fx
    return torch.from_numpy(rows)


cams = orbit(8, 4.0, 700.0)
images = torch.rand(8, 3, H, W, device=dev)
sides = {}
for voxels, (v, c, f) in meshes.items():
    ws, _ = _C.mesh_raster(v, f, cams, W, H, False, -1, -1)
    tid, depth, _, _ = _C.mesh_resolve(v, None, f, cams, W, H, ws, None, 1, None, True)
    for side in (2048, 4096):
        cell, Wt = mesh_texture.atlas_for(f.shape[0], side)
        Ht = mesh_texture.atlas_size(f.shape[0], cell, Wt)[1]
        sides[f"simplified_{voxels}_atlas_{side}"] = {
            "mesh": (v, c, f), "ws": ws, "tid": tid, "depth": depth, "cell": cell, "Wt": Wt, "Ht": Ht, "slack": voxels * VOXEL,
            "accum": torch.zeros(Ht, Wt, 4, device=dev), "times": {"accumulate": [], "finalize": [], "resolve_textured": []}}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.repeats):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / a.repeats, out


for blk in range(a.blocks + 1):                                                        # block 0 warms every side up
    for s in sides.values():
        v, c, f = s["mesh"]
        s["accum"].zero_()
        ms_a, _ = timed(lambda: _C.mesh_texture_accumulate(v, f, cams, W, H, s["cell"], s["Wt"], s["tid"], s["depth"], images, s["slack"], False, s["accum"]))
        ms_f, (tex, cov) = timed(lambda: _C.mesh_texture_finalize(v.shape[0], c, f, s["cell"], s["Wt"], s["accum"]))
        ms_r, _ = timed(lambda: _C.mesh_resolve_textured(v, f, cams, W, H, s["ws"], None, tex, s["cell"], None))
        s["coverage"] = cov.tolist()
        if blk:
            for name, ms in (("accumulate", ms_a), ("finalize", ms_f), ("resolve_textured", ms_r)):
                s["times"][name].append(ms)
out = []
for name, s in sides.items():
    texels, pixels = s["Wt"] * s["Ht"], 8 * W * H
    least = {"accumulate": 32 * texels, "finalize": 19 * texels, "resolve_textured": 28 * pixels}
    row = {"side": name, "triangles": int(s["mesh"][2].shape[0]), "cell": s["cell"], "atlas": [s["Wt"], s["Ht"]], "views": 8,
           "texels_seen": s["coverage"][0], "texels_owned": s["coverage"][1]}
    for stage, t in s["times"].items():
        med = statistics.median(t)
        row[stage + "_ms_median"], row[stage + "_ms_best"] = med, min(t)
        row[stage + "_least_bytes"], row[stage + "_least_GBps"] = least[stage], least[stage] / med / 1e6
    out.append(row)
print(json.dumps({"image": [W, H], "blocks": a.blocks, "repeats_per_block": a.repeats, "sides": out}))
