#!/usr/bin/env python
"""usage (GPU box): python tools/eval_time.py [P W H NVIEWS BLOCKS] -- views/s of held-out view evaluation, two loops compared
INTERLEAVED inside one process (blocks alternate, as tools/ab_interleaved.py does: both see the same host):
  ref   the reference-shaped loop: render() per view, then torch's psnr (image_utils.py) and ssim (loss_utils.py) of the
        clamped pair, `.item()` per view (train.py:238-252 / metrics.py:96-106 without the PNG files)
  eval  evaluate.evaluate_views(mode="report"): 8 views per forward launch, one metrics launch + one SSIM launch per batch,
        one read-back per batch and one at the end
Default: 1M Gaussians, 8 views of 800x600.  Prints the median and best block of each, and one JSON line."""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import evaluate, loss, synth          # noqa: E402
from binocular3dgs_amd.render import PipelineParams, render  # noqa: E402

P, W, H, NV, BLOCKS = (int(x) for x in sys.argv[1:6]) if len(sys.argv) >= 6 else (1_000_000, 800, 600, 8, 6)
REPS = 5                    # evaluations of all NV views per block
dev = "cuda"

model = synth.synth_model(P, seed=0, device=dev, width=W, height=H)
cams = synth.synth_cameras(W, H, yaws=synth.YAWS_8[:NV] if NV <= 8 else tuple(range(NV)), device=dev)
gen = torch.Generator(device=dev).manual_seed(1)
for c in cams:
    c.original_image = torch.rand(3, H, W, device=dev, generator=gen)
bg = torch.zeros(3, device=dev)
pipe = PipelineParams()


def ref_loop():
    out = []
    with torch.no_grad():
        for c in cams:
            img = torch.clamp(render(c, model, pipe, bg)["render"], 0.0, 1.0)
            gt = torch.clamp(c.original_image, 0.0, 1.0)
            out.append((loss.psnr(img, gt).mean().item(), loss.ssim(img[None], gt[None]).item(),
                        loss.l1_loss(img, gt).item()))
    return out


def eval_loop():
    return evaluate.evaluate_views(model, cams, bg, mode="report")


loops = {"ref": ref_loop, "eval": eval_loop}
for fn in loops.values():              # warm-up: kernels loaded, renderer built and sized, allocator warm
    fn()
    fn()
torch.cuda.synchronize()
a = ref_loop()
b = eval_loop()["per_view"]
dpsnr = max(abs(x[0] - y["PSNR"]) for x, y in zip(a, b))
dssim = max(abs(x[1] - y["SSIM"]) for x, y in zip(a, b))
times = {k: [] for k in loops}
for blk in range(BLOCKS):
    for name, fn in loops.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        times[name].append(REPS * NV / (time.perf_counter() - t0))
res = {"P": P, "W": W, "H": H, "views": NV, "max_dpsnr_db": dpsnr, "max_dssim": dssim}
for name, v in times.items():
    res[f"{name}_views_per_s_median"] = round(statistics.median(v), 1)
    res[f"{name}_views_per_s_best"] = round(max(v), 1)
    print(f"{name:5s} views/s  median {statistics.median(v):9.1f}  best {max(v):9.1f}  blocks {[round(x, 1) for x in v]}")
print(json.dumps(res))
