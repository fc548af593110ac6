#!/usr/bin/env python
"""usage (GPU box): python tools/simplify_time.py [--resolution 256] -- the device time of mesh_tools.simplify on the mesh of a
resolution^3 volume that holds a sphere resting on a slab (an analytic signed distance written straight into the volume, then
TsdfVolume.extract), at cells of 2 and 4 voxels, stage by stage:
  count   b3gs_mesh_simplify_count: box, keys, the vertex sort, clusters, the three face sorts, the two ranks
  emit    b3gs_mesh_simplify_emit per placement: faces, (quadric: the incidence sort), one thread per cluster
The sides run in ALTERNATING blocks inside one process (block 0 warms all of them up); every stage is timed with device events
around `repeats` calls; median and best block per side.  Nothing is asserted about speed.  Prints one JSON line."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, mesh, mesh_tools       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--blocks", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5, help="calls per timed block and stage")
a = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("simplify_time.py measures on the HIP device: none found")
dev = torch.device("cuda")
RES = a.resolution
VOXEL = 3.0 / RES
TRUNC = 4.0 * VOXEL

vol = mesh.TsdfVolume([-1.5] * 3, [1.5] * 3, VOXEL, TRUNC, device=dev)
assert vol.dims == (RES, RES, RES), vol.dims
axis = vol.origin[0] + (torch.arange(RES, device=dev, dtype=torch.float32) + 0.5) * VOXEL
px, py, pz = axis[None, None, :], axis[None, :, None], axis[:, None, None]
sphere = torch.sqrt(px * px + (py - 0.1) ** 2 + pz * pz) - 0.8
slab = torch.maximum((py + 0.9).abs() - 0.2, torch.maximum(px.abs(), pz.abs()) - 1.3)
vol.tsdf.copy_(torch.clamp(torch.minimum(sphere, slab) / TRUNC, -1.0, 1.0))
vol.weight.fill_(1.0)
vol.rgb.copy_(torch.stack(torch.broadcast_tensors(px / 3 + 0.5, py / 3 + 0.5, pz / 3 + 0.5), -1))
vertices, colours, faces = vol.extract()


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(a.repeats):
        out = fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / a.repeats, out


sides = {}
for k in (2.0, 4.0):
    cell = k * VOXEL
    ws, totals = _C.mesh_simplify_count(vertices, faces, cell)
    t = totals.tolist()
    sides[k] = {"cell": cell, "ws": ws, "nverts": t[0], "ntris": t[1], "clusters": t[5],
                "times": {"count": [], "emit_quadric": [], "emit_mean": []}}
for blk in range(a.blocks + 1):                                                        # block 0 warms every side up
    for k, s in sides.items():
        ms, (s["ws"], _) = timed(lambda: _C.mesh_simplify_count(vertices, faces, s["cell"]))
        stage = {"count": ms}
        for name in ("quadric", "mean"):
            stage["emit_" + name], _ = timed(lambda: _C.mesh_simplify_emit(vertices, colours, faces, s["cell"], mesh_tools.PLACEMENTS[name],
                                                                           s["ws"], s["nverts"], s["ntris"]))
        if blk:
            for name, ms in stage.items():
                s["times"][name].append(ms)
print(json.dumps({"volume": list(vol.dims), "vertices_in": int(vertices.shape[0]), "triangles_in": int(faces.shape[0]),
                  "blocks": a.blocks, "repeats_per_block": a.repeats,
                  "sides": [{"cell_voxels": k, "clusters": s["clusters"], "vertices_out": s["nverts"], "triangles_out": s["ntris"],
                             **{n + "_ms_median": statistics.median(v) for n, v in s["times"].items()},
                             **{n + "_ms_best": min(v) for n, v in s["times"].items()}} for k, s in sides.items()]}))
