#!/usr/bin/env python
"""usage (GPU box): python tools/mesh_render_time.py [--resolution 256] [--no-model] -- the device time of the mesh rasterizer
(csrc/meshraster.hip) on the sphere-and-slab mesh of tools/simplify_time.py (a resolution^3 volume, 1.55 M triangles at 256), on
its 2-voxel and 4-voxel simplifications, 8 orbit views at 800 x 600, and on ONE close camera for which a few triangles of the
4-voxel mesh cover most of the image -- the latter also with every triangle forced through the one-lane path (thresholds at
infinity): the factor is what the wave and workgroup paths buy.  raster (b3gs_mesh_raster_batch) and resolve
(b3gs_mesh_resolve_batch) are timed separately with device events around `repeats` calls; the sides run in ALTERNATING blocks
in one process (block 0 warms all of them up); median and best block per side.  As context only, evaluate.render_views of a
synthetic model of 1 M Gaussians at the same size, in the same process.  Nothing is asserted about speed.  One JSON line."""
import argparse
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, mesh, mesh_tools       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3, help="calls per timed block and stage")
ap.add_argument("--no-model", action="store_true", help="skip the 1 M Gaussian context render")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("mesh_render_time.py measures on the HIP device: none found")
dev = torch.device("cuda")
RES, W, H = a.resolution, 800, 600
VOXEL = 3.0 / RES
TRUNC = 4.0 * VOXEL
INT_MAX = 2 ** 31 - 1

vol = mesh.TsdfVolume([-1.5] * 3, [1.5] * 3, VOXEL, TRUNC, device=dev)
axis = vol.origin[0] + (torch.arange(RES, device=dev, dtype=torch.float32) + 0.5) * VOXEL
px, py, pz = axis[None, None, :], axis[None, :, None], axis[:, None, None]
sphere = torch.sqrt(px * px + (py - 0.1) ** 2 + pz * pz) - 0.8
slab = torch.maximum((py + 0.9).abs() - 0.2, torch.maximum(px.abs(), pz.abs()) - 1.3)
vol.tsdf.copy_(torch.clamp(torch.minimum(sphere, slab) / TRUNC, -1.0, 1.0))
vol.weight.fill_(1.0)
vol.rgb.copy_(torch.stack(torch.broadcast_tensors(px / 3 + 0.5, py / 3 + 0.5, pz / 3 + 0.5), -1))
raw = vol.extract()
meshes = {"raw": raw, "simplified_2": mesh_tools.simplify(*raw, 2.0 * VOXEL), "simplified_4": mesh_tools.simplify(*raw, 4.0 * VOXEL)}


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


far, close = orbit(8, 4.0, 700.0), orbit(1, 1.2, 9000.0)
sides = {name: {"mesh": m, "cams": far, "box": (-1, -1)} for name, m in meshes.items()}
sides["close_simplified_4"] = {"mesh": meshes["simplified_4"], "cams": close, "box": (-1, -1)}
sides["close_simplified_4_one_lane"] = {"mesh": meshes["simplified_4"], "cams": close, "box": (INT_MAX, INT_MAX)}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.repeats):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / a.repeats, out


for s in sides.values():
    s["times"] = {"raster": [], "resolve": []}
for blk in range(a.blocks + 1):                                                        # block 0 warms every side up
    for s in sides.values():
        v, c, f = s["mesh"]
        ms_r, (ws, _) = timed(lambda: _C.mesh_raster(v, f, s["cams"], W, H, False, s["box"][0], s["box"][1]))
        ms_s, out = timed(lambda: _C.mesh_resolve(v, c, f, s["cams"], W, H, ws, None, 0, None, True))
        s["covered"] = float(out[2].mean())
        if blk:
            s["times"]["raster"].append(ms_r)
            s["times"]["resolve"].append(ms_s)
result = {"image": [W, H], "blocks": a.blocks, "repeats_per_block": a.repeats,
          "sides": [{"side": name, "views": int(s["cams"].shape[0]), "triangles": int(s["mesh"][2].shape[0]), "covered": round(s["covered"], 4),
                     **{n + "_ms_median": statistics.median(t) for n, t in s["times"].items()},
                     **{n + "_ms_best": min(t) for n, t in s["times"].items()}} for name, s in sides.items()]}
if not a.no_model:
    from binocular3dgs_amd import evaluate, synth
    model = synth.synth_model(1_000_000, seed=1, device="cuda", width=W, height=H)
    cams = synth.synth_cameras(W, H, yaws=tuple(5.0 * k for k in range(8)), device="cuda")
    bg = torch.zeros(3, device=dev)
    evaluate.render_views(model, cams, bg)
    times = [timed(lambda: evaluate.render_views(model, cams, bg))[0] for _ in range(a.blocks)]
    result["context_render_views_1M_gaussians_8_views_ms"] = {"median": statistics.median(times), "best": min(times)}
print(json.dumps(result))
