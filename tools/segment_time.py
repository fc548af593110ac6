#!/usr/bin/env python
"""usage (GPU box): python tools/segment_time.py [P W H VIEWS] -- the label votes of b3gs_label_votes_batch for L = 2, 4 and 16
labels against the only way to get the same numbers without it: L calls of b3gs_blend_contribution_batch, one per binary mask
(labels == l); and b3gs_label_render_batch for the same L.  `synth` scene at the headline shape (1M Gaussians, 800x600, 8
views), rendered once by a FusedRasterizer.  Two label planes: "blocks" (32 x 32 pixel squares cycling through the labels: most
quadrants hold one label, as object masks do) and "noise" (a per-pixel draw: every DPP row holds many labels, the worst case).
All calls ALTERNATE in blocks inside one process (they see the same host and device state), each block timed with HIP events
around REPS calls.  The votes of both routes are compared for equality before anything is timed.  Prints one JSON line: medians
in microseconds per call (the L masked contribution calls count as one), and the ratios."""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _lib, synth                   # noqa: E402
from binocular3dgs_amd.fused import FusedRasterizer          # noqa: E402

P, W, H, NV = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (1_000_000, 800, 600, 8)
BLOCKS, REPS = 5, 3
LABELS = (2, 4, 16)
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

lib = _lib.lib()
stream = torch.cuda.current_stream(dev).cuda_stream
scenes = [_lib.B3gsScene() for _ in range(NV)]
for sc in scenes:
    sc.P, sc.W, sc.H, sc.background = P, W, H, bg.data_ptr()


def state(t, k):
    s = fr.slots[k]
    t.view = C.pointer(scenes[k])
    t.geometry, t.binning, t.image = s.geom.data_ptr(), s.binning.data_ptr(), s.img.data_ptr()


yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
gen = torch.Generator(device=dev).manual_seed(0)
keep, CALLS, check = [], {}, []
for L in LABELS:
    for kind in ("blocks", "noise"):
        plane = ((xx // 32 + yy // 32) % L if kind == "blocks" else torch.randint(0, L, (H, W), device=dev, generator=gen)).to(torch.uint8).contiguous()
        masks = [(plane == l).to(torch.uint8).contiguous() for l in range(L)]
        votes = torch.zeros((P, L), dtype=torch.int64, device=dev)
        cols = [torch.zeros(P, dtype=torch.int64, device=dev) for _ in range(L)]
        i32 = [torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(3)]
        lv = (_lib.B3gsLabelVoteView * NV)()
        cvs = [(_lib.B3gsContribView * NV)() for _ in range(L)]
        outs = [_lib.B3gsContribOut(c.data_ptr(), *(t.data_ptr() for t in i32)) for c in cols]
        for k in range(NV):
            state(lv[k], k)
            lv[k].labels = plane.data_ptr()
            for l in range(L):
                state(cvs[l][k], k)
                cvs[l][k].pixel_mask = masks[l].data_ptr()
        keep += [plane, masks, votes, cols, i32, lv, cvs, outs]

        def one_walk(L=L, lv=lv, votes=votes):
            _lib.check(lib.b3gs_label_votes_batch(NV, lv, L, votes.data_ptr(), stream), "b3gs_label_votes_batch")

        def masked_calls(L=L, cvs=cvs, outs=outs):
            for l in range(L):
                _lib.check(lib.b3gs_blend_contribution_batch(NV, cvs[l], C.byref(outs[l]), stream), "b3gs_blend_contribution_batch")
        CALLS[f"votes_L{L}_{kind}"], CALLS[f"contrib_x{L}_{kind}"] = one_walk, masked_calls
        check.append((f"L{L}_{kind}", votes, cols))
    gl = (torch.arange(P, device=dev) % L).to(torch.uint8)
    rv = (_lib.B3gsLabelRenderView * NV)()
    planes = [(torch.empty((H, W), dtype=torch.uint8, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev)) for _ in range(NV)]
    for k in range(NV):
        state(rv[k], k)
        rv[k].label, rv[k].weight = planes[k][0].data_ptr(), planes[k][1].data_ptr()
    keep += [gl, rv, planes]

    def render(L=L, rv=rv, gl=gl):
        _lib.check(lib.b3gs_label_render_batch(NV, rv, L, gl.data_ptr(), stream), "b3gs_label_render_batch")
    CALLS[f"render_L{L}"] = render

for f in CALLS.values():     # warm-up; and the one pass whose results are compared
    f()
torch.cuda.synchronize(dev)
for tag, votes, cols in check:
    assert int(votes.sum()) > 0 and torch.equal(votes, torch.stack(cols, 1)), f"{tag}: the two routes disagree"
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
med = {k: round(statistics.median(v), 1) for k, v in us.items()}
res = {"tool": "segment_time", "P": P, "W": W, "H": H, "views": NV, "blocks": BLOCKS, "reps": REPS, "us": med,
       "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
       "contrib_calls_over_one_walk": {f"L{L}_{kind}": round(med[f"contrib_x{L}_{kind}"] / med[f"votes_L{L}_{kind}"], 2)
                                       for L in LABELS for kind in ("blocks", "noise")}}
print(json.dumps(res))
