#!/usr/bin/env python
"""usage (GPU box): python tools/frames_time.py [P W H NVIEWS BLOCKS] -- frames/s of a rendered path, three loops compared
INTERLEAVED inside one process (blocks alternate, as tools/eval_time.py does):
  views  evaluate.render_views on the path cameras (the render alone, 8 views per launch)
  path   frames.render_path(out_dir=None): the same renders plus rgb / gray / colour-mapped depth encoded on the device
  ref    the reference-shaped loop (spiral.py:101-131 without the files): one render() per view, then its torch statements
         for the gray depth, a torch.sort percentile, the curve, a LUT gather on the device and the three quantisations
Also times write_png on one frame triple (host zlib work, not part of the ratio).  Default: 1M Gaussians, 120 cameras of
800x600.  Prints the median and best block of each and one JSON line."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import evaluate, frames, synth          # noqa: E402
from binocular3dgs_amd.render import PipelineParams, render   # noqa: E402

P, W, H, NV, BLOCKS = (int(x) for x in sys.argv[1:6]) if len(sys.argv) >= 6 else (1_000_000, 800, 600, 120, 4)
dev = "cuda"

model = synth.synth_model(P, seed=0, device=dev, width=W, height=H)
cams = synth.synth_cameras(W, H, yaws=tuple(-30.0 + 60.0 * k / NV for k in range(NV)), device=dev)
bg = torch.zeros(3, device=dev)
pipe = PipelineParams()
lut = torch.from_numpy(frames.TURBO_U8.astype(np.float64) / 255.0).to(dev)   # any [256,3] table: the gather is what costs


def _q(x):
    return torch.clamp(x * 255 + 0.5, 0, 255).to(torch.uint8)


def ref_loop():
    out = []
    eps = float(np.finfo(np.float32).eps)
    with torch.no_grad():
        for c in cams:
            pkg = render(c, model, pipe, bg)
            rgb, depth, alpha = pkg["render"], pkg["rendered_depth"], pkg["rendered_alpha"]
            d = 1.0 - (depth - depth.min()) / (depth.max() - depth.min())
            v = 1.0 - d * alpha
            s = torch.sort(v.reshape(-1))[0].double()
            n = s.numel()
            q = torch.tensor([0.5, 99.5], dtype=torch.float64, device=dev) * (n / 100)
            j = torch.clamp(q.floor().long() - 1, 0, n - 2)
            b = s[j] + (s[j + 1] - s[j]) * (q - (j + 1))
            lo, hi = -torch.log(b[0] - eps + 1e-6), -torch.log(b[1] + eps + 1e-6)
            cv = -torch.log(v[0] + 1e-6).double()
            x = torch.nan_to_num(torch.clamp((cv - torch.minimum(lo, hi)) / (hi - lo).abs(), 0, 1))
            idx = torch.clamp((x * 256).long(), max=255)
            out.append((_q(rgb), _q(v), _q(lut[idx])))
    return out


def views_loop():
    return evaluate.render_views(model, cams, bg)


def path_loop():
    return frames.render_path(model, cams, bg)


loops = {"views": views_loop, "path": path_loop, "ref": ref_loop}
for fn in loops.values():               # warm-up: kernels loaded, renderers built and sized, allocator warm
    fn()
torch.cuda.synchronize()
times = {k: [] for k in loops}
for blk in range(BLOCKS):
    for name, fn in loops.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times[name].append(NV / (time.perf_counter() - t0))

fr = path_loop()[0]
host = [fr[k].cpu() for k in ("rgb", "depth", "cdepth")]
with tempfile.TemporaryDirectory() as tmp:
    t0 = time.perf_counter()
    for r in range(5):
        for k, h in enumerate(host):
            frames.write_png(os.path.join(tmp, f"{r}_{k}.png"), h)
    png_ms = (time.perf_counter() - t0) / 15 * 1e3

res = {"P": P, "W": W, "H": H, "views": NV, "png_ms_per_image_one_thread": round(png_ms, 2)}
for name, v in times.items():
    res[f"{name}_frames_per_s_median"] = round(statistics.median(v), 1)
    res[f"{name}_frames_per_s_best"] = round(max(v), 1)
    print(f"{name:5s} frames/s  median {statistics.median(v):9.1f}  best {max(v):9.1f}  blocks {[round(x, 1) for x in v]}")
res["path_over_views"] = round(res["path_frames_per_s_median"] / res["views_frames_per_s_median"], 3)
res["path_over_ref"] = round(res["path_frames_per_s_median"] / res["ref_frames_per_s_median"], 2)
print(f"write_png: {png_ms:.2f} ms per 800x600 image on one thread")
print(json.dumps(res))
