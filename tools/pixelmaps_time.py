#!/usr/bin/env python
"""usage (GPU box): python tools/pixelmaps_time.py [P W H VIEWS] -- the pixel-maps batch (b3gs_blend_pixel_maps_batch) against
the blend forward batch (b3gs_blend_forward_batch) of the same views, on the `synth` scene at the headline shape (1M Gaussians,
800x600, 8 views).  The views are rendered once by a FusedRasterizer; the two calls then ALTERNATE in blocks inside one process
(both see the same host and device state), each block timed with HIP events around REPS calls.  Prints one JSON line: medians
of both in microseconds per call and their ratio."""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _lib, synth                   # noqa: E402
from binocular3dgs_amd.fused import FusedRasterizer          # noqa: E402

P, W, H, NV = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (1_000_000, 800, 600, 8)
BLOCKS, REPS = 7, 5
dev = torch.device("cuda:0")
model = synth.synth_model(P, seed=0, device=dev, width=W, height=H, requires_grad=False)
cams = synth.synth_cameras(W, H, yaws=synth.YAWS_8[:NV], device=dev)
bg = torch.zeros(3, device=dev)
fr = FusedRasterizer(model, W, H, num_slots=NV, want_means2D=False, schedule="batched", seg1_fraction=0.0)
views = [(c, k) for k, c in enumerate(cams)]
fr.fit_capacity(views, bg)
with torch.no_grad():
    fr.render_batch(views, bg)
torch.cuda.synchronize(dev)
assert int(fr.overflow_flag.item()) & 1 == 0

L = _lib.lib()
stream = torch.cuda.current_stream(dev).cuda_stream
scenes = [_lib.B3gsScene() for _ in range(NV)]
blend = (_lib.B3gsBlendView * NV)()
maps = (_lib.B3gsPixelMapView * NV)()
planes = []
for k, (sc, s) in enumerate(zip(scenes, fr.slots)):
    sc.P, sc.W, sc.H, sc.background = P, W, H, bg.data_ptr()
    for t in (blend[k], maps[k]):
        t.view = C.pointer(sc)
        t.geometry, t.binning, t.image = s.geom.data_ptr(), s.binning.data_ptr(), s.img.data_ptr()
    blend[k].out_color, blend[k].out_depth, blend[k].out_alpha = s.color.data_ptr(), s.depth.data_ptr(), s.alpha.data_ptr()
    blend[k].binning_capacity = s.capacity
    out = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(3)] + \
          [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(2)]
    planes.append(out)
    maps[k].median_depth, maps[k].depth_m1, maps[k].depth_m2, maps[k].dominant, maps[k].count = (t.data_ptr() for t in out)
CALLS = {"blend_forward": lambda: _lib.check(L.b3gs_blend_forward_batch(NV, blend, stream), "b3gs_blend_forward_batch"),
         "pixel_maps": lambda: _lib.check(L.b3gs_blend_pixel_maps_batch(NV, maps, stream), "b3gs_blend_pixel_maps_batch")}
for f in CALLS.values():     # warm-up
    f()
torch.cuda.synchronize(dev)
entries = int(sum(int(p[4].sum(dtype=torch.int64)) for p in planes))
us = {k: [] for k in CALLS}
for _ in range(BLOCKS):
    for k, f in CALLS.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _r in range(REPS):
            f()
        b.record()
        torch.cuda.synchronize(dev)
        us[k].append(1000.0 * a.elapsed_time(b) / REPS)
med = {k: statistics.median(v) for k, v in us.items()}
print(json.dumps({"tool": "pixelmaps_time", "P": P, "W": W, "H": H, "views": NV, "blocks": BLOCKS, "reps": REPS,
                  "blend_forward_us": round(med["blend_forward"], 1), "pixel_maps_us": round(med["pixel_maps"], 1),
                  "ratio": round(med["pixel_maps"] / med["blend_forward"], 2),
                  "blend_forward_us_min_max": [round(min(us["blend_forward"]), 1), round(max(us["blend_forward"]), 1)],
                  "pixel_maps_us_min_max": [round(min(us["pixel_maps"]), 1), round(max(us["pixel_maps"]), 1)],
                  "blended_entries_per_call": entries}))
