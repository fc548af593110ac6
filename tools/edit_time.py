#!/usr/bin/env python
"""usage (GPU box): python tools/edit_time.py -- the model editor at 1M Gaussians (events around the call, warm, median of 20):
  transform  b3gs_transform_gaussians at sh_degree 3, out of place: ms and bytes per second, counting xyz, rotation, scaling and
             features_rest once in and once out (220 bytes each way per Gaussian)
  select     b3gs_select_gaussians with a box, a sphere, both float tests and 8 masked views at 800 x 600: ms
  icp        one iteration of edit.register's device part at 1M points against 1M: transform_points, nearest_query_index and
             similarity_sums (the grid over dst is built once, outside), and the query alone
  copy       a device copy of the bytes the transform moves (torch's clone), the rate to hold it against, beside the streaming
             rate DESIGN.md records for this part (adam_kernel: 4.9-5.9 TB/s)
Prints one JSON line.  No bar is fixed."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, edit, synth                      # noqa: E402
from binocular3dgs_amd.mesh_tools import NearestGrid               # noqa: E402

dev = torch.device("cuda")
DESIGN_STREAM_TBPS = (4.9, 5.9)


def events(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


P = 1_000_000
model = synth.synth_model(P, seed=0, device=dev, K=16, requires_grad=False)
g = np.random.default_rng(0)
q = g.standard_normal(4)
w, x, y, z = q / np.linalg.norm(q)
R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
              [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
T = edit.Similarity(R, [0.3, -0.2, 0.1], 1.3)
words = T.device_words()
out = {"P": P}

ins = [model._xyz.detach(), model._rotation.detach(), model._scaling.detach(), model._features_rest.detach().contiguous()]
outs = [torch.empty_like(t) for t in ins]
med, best = events(lambda: _C.transform_gaussians(3, *ins, words, *outs))
nbytes = 2 * sum(t.numel() * 4 for t in ins)
flat = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
cmed, _ = events(lambda: flat.clone())
out["transform"] = {"ms": med, "best_ms": best, "bytes": nbytes, "GBps": nbytes / med / 1e6, "copy_ms": cmed, "copy_GBps": nbytes / cmed / 1e6}
print(f"transform, degree 3: {med:.3f} ms, {nbytes / med / 1e6:.0f} GB/s; a device copy of the same bytes: {nbytes / cmed / 1e6:.0f} GB/s; "
      f"DESIGN.md's streaming kernels: {DESIGN_STREAM_TBPS[0]}-{DESIGN_STREAM_TBPS[1]} TB/s")

cams = synth.synth_cameras(800, 600, yaws=synth.YAWS_8, device=dev)
cw = torch.from_numpy(edit.camera_words(cams)).to(dev)
masks = (torch.rand((8, 600, 800), device=dev) < 0.7).to(torch.uint8)
box = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, -6.0, 3.0, 2.0, 4.0]
med, best = events(lambda: _C.select_gaussians(ins[0], model._opacity.detach(), ins[2], box, [0.0, 0.0, 6.0, 25.0], -1.0, -2.0, cw, masks, 2))
sbytes = P * (12 + 4 + 12 + 1 + 4)
flat = torch.empty(sbytes // 2, dtype=torch.uint8, device=dev)
cmed, _ = events(lambda: flat.clone())
out["select_8_masked_views"] = {"ms": med, "best_ms": best, "bytes_without_masks": sbytes, "copy_ms": cmed}
print(f"select, every test, 8 masked views: {med:.3f} ms; a device copy of its {sbytes / 1e6:.0f} MB of rows: {cmed:.3f} ms")

src = ins[0].contiguous()
dst = edit.transform_points(src, edit.Similarity(edit._rotation_about([0.2, 1.0, -0.4], 2.0), [0.01, -0.02, 0.01], 1.0))
max_dist = 0.05
grid = NearestGrid(dst, max_dist)
cur = torch.empty_like(src)
sums = torch.empty(18, dtype=torch.float64, device=dev)
o = [0.0, 0.0, 6.0]
I = edit.Similarity().device_words()


def iteration():
    _C.transform_points(src, I, cur)
    dist, index = grid.query_index(cur)
    _C.similarity_sums(src, dst, index, dist, max_dist, None, o, o, sums)


med, best = events(iteration)
qmed, _ = events(lambda: grid.query_index(src))
gmed, _ = events(lambda: NearestGrid(dst, max_dist))
ibytes = P * (12 + 12 + 12 + 8 + (12 + 12 + 8))
flat = torch.empty(ibytes // 2, dtype=torch.uint8, device=dev)
cmed, _ = events(lambda: flat.clone())
out["icp_iteration_1M_vs_1M"] = {"ms": med, "best_ms": best, "query_index_ms": qmed, "grid_build_ms": gmed, "copy_ms": cmed, "bytes_streamed": ibytes,
                                 "grid": grid.params(), "pairs": int(sums[0].item())}
print(f"one ICP iteration, 1M against 1M: {med:.3f} ms (the query alone {qmed:.3f} ms; the grid, built once, {gmed:.3f} ms); a device copy of "
      f"the {ibytes / 1e6:.0f} MB it streams: {cmed:.3f} ms")
print(json.dumps(out))
