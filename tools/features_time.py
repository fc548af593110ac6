#!/usr/bin/env python
"""usage (GPU box): python tools/features_time.py [P W H VIEWS] -- the feature render and the feature lift (csrc/features.hip) for
C = 3, 8, 16 and 64 channels against the only way to get the same maps and sums without them:
  render   ceil(C / 3) forwards per view of the drop-in rasterizer with three channels as colors_precomp (projection, binning,
           sorting and blending every time); the feature render walks the lists of ONE forward, which both routes need, so that
           forward is timed on its own ("forward_batch") and not charged to either
  lift     C calls of b3gs_blend_contribution_batch, one per channel, under a binary pixel mask (what an indicator channel
           costs today; a continuous channel has no route at all)
`synth` scene at the headline shape (1M Gaussians, 800x600, 8 views), rendered once by a FusedRasterizer.  All calls ALTERNATE in
blocks inside one process (they see the same host and device state), each block timed with HIP events around REPS calls.  Before
anything is timed the first three channels of the feature render are compared with the drop-in's planes of view 0 and the lift
of an indicator channel with the masked contribution.  Prints one JSON line: medians in microseconds per call (all views; the
C / 3 forwards and the C contribution calls count as one), and the ratios."""
import ctypes as C
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _lib, synth                   # noqa: E402
from binocular3dgs_amd.fused import FusedRasterizer          # noqa: E402
from binocular3dgs_amd.render import PipelineParams, render  # noqa: E402

P, W, H, NV = (int(x) for x in sys.argv[1:5]) if len(sys.argv) >= 5 else (1_000_000, 800, 600, 8)
BLOCKS, REPS = 5, 2
CHANNELS = (3, 8, 16, 64)
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
pipe = PipelineParams()


def state(t, k):
    s = fr.slots[k]
    t.view = C.pointer(scenes[k])
    t.geometry, t.binning, t.image = s.geom.data_ptr(), s.binning.data_ptr(), s.img.data_ptr()


gen = torch.Generator(device=dev).manual_seed(0)
keep, CALLS, check = [], {}, []
for nch in CHANNELS:
    f = torch.rand((P, nch), device=dev, generator=gen).contiguous()
    planes = [torch.empty((nch, H, W), device=dev) for _ in range(NV)]
    rv = (_lib.B3gsFeatureRenderView * NV)()
    for k in range(NV):
        state(rv[k], k)
        rv[k].out = planes[k].data_ptr()
    triples = [f[:, c:c + 3].contiguous() if c + 3 <= nch else torch.cat([f[:, c:], torch.zeros((P, c + 3 - nch), device=dev)], 1).contiguous()
               for c in range(0, nch, 3)]

    def feature_render(nch=nch, rv=rv, f=f):
        _lib.check(lib.b3gs_feature_render_batch(NV, rv, nch, f.data_ptr(), stream), "b3gs_feature_render_batch")

    def precomp_forwards(triples=triples):
        with torch.no_grad():
            for cam in cams:
                for t in triples:
                    render(cam, model, pipe, bg, override_color=t)
    CALLS[f"feature_render_C{nch}"], CALLS[f"colors_precomp_C{nch}"] = feature_render, precomp_forwards

    # maps: channel c is a binary plane (every pixel of a 32 x 32 block pattern), so that both routes sum the same integers
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    masks = [(((xx // 32 + yy // 32 + c) % 3) == 0).to(torch.uint8).contiguous() for c in range(nch)]
    maps = torch.stack(masks).to(torch.float32).contiguous()
    sums = torch.zeros((P, nch), dtype=torch.int64, device=dev)
    cols = [torch.zeros(P, dtype=torch.int64, device=dev) for _ in range(nch)]
    i32 = [torch.zeros(P, dtype=torch.int32, device=dev) for _ in range(3)]
    lv = (_lib.B3gsFeatureLiftView * NV)()
    cvs = [(_lib.B3gsContribView * NV)() for _ in range(nch)]
    outs = [_lib.B3gsContribOut(c.data_ptr(), *(t.data_ptr() for t in i32)) for c in cols]
    for k in range(NV):
        state(lv[k], k)
        lv[k].maps = maps.data_ptr()
        for c in range(nch):
            state(cvs[c][k], k)
            cvs[c][k].pixel_mask = masks[c].data_ptr()
    scale = (C.c_float * nch)(*([1.0] * nch))
    keep += [f, planes, rv, triples, masks, maps, sums, cols, i32, lv, cvs, outs, scale]

    def feature_lift(nch=nch, lv=lv, sums=sums, scale=scale):
        _lib.check(lib.b3gs_feature_lift_batch(NV, lv, nch, scale, sums.data_ptr(), None, stream), "b3gs_feature_lift_batch")

    def masked_calls(nch=nch, cvs=cvs, outs=outs):
        for c in range(nch):
            _lib.check(lib.b3gs_blend_contribution_batch(NV, cvs[c], C.byref(outs[c]), stream), "b3gs_blend_contribution_batch")
    CALLS[f"feature_lift_C{nch}"], CALLS[f"contrib_x{nch}"] = feature_lift, masked_calls
    check.append((nch, planes, triples, sums, cols))


def forward_batch():
    with torch.no_grad():
        fr.render_batch(views, bg)


CALLS["forward_batch"] = forward_batch
for fn in CALLS.values():     # warm-up; and the one pass whose results are compared
    fn()
torch.cuda.synchronize(dev)
for nch, planes, triples, sums, cols in check:
    assert int(sums.abs().sum()) > 0 and torch.equal(sums, torch.stack(cols, 1)), f"C = {nch}: the two lift routes disagree"
    with torch.no_grad():
        ref = render(cams[0], model, pipe, bg, override_color=triples[0])["render"]
    d = float((ref - planes[0][:3]).abs().max())
    assert float(ref.abs().max()) > 0 and d <= 1e-4, f"C = {nch}: the feature render and the drop-in's colour planes differ by {d}"
us = {k: [] for k in CALLS}
for _ in range(BLOCKS):
    for k, fn in CALLS.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _r in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        us[k].append(1000.0 * a.elapsed_time(b) / REPS)
med = {k: round(statistics.median(v), 1) for k, v in us.items()}
res = {"tool": "features_time", "P": P, "W": W, "H": H, "views": NV, "blocks": BLOCKS, "reps": REPS, "us": med,
       "us_min_max": {k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
       "precomp_forwards_over_feature_render": {f"C{n}": round(med[f"colors_precomp_C{n}"] / med[f"feature_render_C{n}"], 2) for n in CHANNELS},
       "precomp_forwards_over_forward_plus_feature_render": {f"C{n}": round(med[f"colors_precomp_C{n}"] / (med["forward_batch"] + med[f"feature_render_C{n}"]), 2)
                                                             for n in CHANNELS},
       "contrib_calls_over_feature_lift": {f"C{n}": round(med[f"contrib_x{n}"] / med[f"feature_lift_C{n}"], 2) for n in CHANNELS}}
print(json.dumps(res))
