#!/usr/bin/env python
"""usage (GPU box): python tools/gt_prep_time.py -- ground-truth preparation of 8 views, LLFF-shaped (4032x3024x3 -> 504x378) and
Blender-shaped (800x800x4 -> 400x400), reported separately:
  upload   pinned host memory -> device, asynchronous, events around the 8 copies
  device   b3gs_prepare_gt_batch (events around the call, warm, median of 20): microseconds and GB/s over source bytes read +
           intermediate written and read + output written
  ref      the reference-shaped path on this box: Pillow resize + the torch statements on ONE CPU thread + .cuda().  Without
           Pillow this row is left out (the numpy restatement of the tests is not a fair stand-in).
and the DTU mask at 400x300: the one launch here against the reference's 49-statement loop run on the device.
Prints one JSON line."""
import json
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C                        # noqa: E402
from binocular3dgs_amd import ground_truth as G         # noqa: E402

dev = torch.device("cuda")
rng = np.random.default_rng(0)
out = {}


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
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts)


for name, (Hs, Ws, C), (W, H) in (("llff", (3024, 4032, 3), (504, 378)), ("blender", (800, 800, 4), (400, 400))):
    host = [torch.from_numpy(rng.integers(0, 256, (Hs, Ws, C), dtype=np.uint8)).pin_memory() for _ in range(8)]
    up = events(lambda: [h.to(dev, non_blocking=True) for h in host], n=10, warm=2)
    srcs = [h.to(dev) for h in host]
    tx = [G.device_table(Ws, W, dev)] * 8
    ty = [G.device_table(Hs, H, dev)] * 8
    med, best = events(lambda: _C.prepare_gt(srcs, tx, ty, W, H, True, 0.0))
    co = 3 if C >= 3 else 1
    nbytes = 8 * (Hs * Ws * C + 2 * Hs * W * C + H * W * 4 * (co + (C == 4)))
    row = {"upload_us": up[0], "device_us": med, "device_best_us": best, "device_GBps": nbytes / med / 1e3,
           "source_MB": 8 * Hs * Ws * C / 1e6}
    try:
        from PIL import Image
        torch.set_num_threads(1)
        t0 = time.perf_counter()
        for h in host:
            t = torch.from_numpy(np.array(Image.fromarray(h.numpy()).resize((W, H)))) / 255.0
            t = t.permute(2, 0, 1)
            img = t[:3]
            if C == 4:
                img = img * t[3:4] + (1 - t[3:4])
            img = img.clamp(0.0, 1.0)
            if C == 4:
                img = img * t[3:4]
            img = img.cuda()
        torch.cuda.synchronize()
        row["ref_us"] = (time.perf_counter() - t0) * 1e6
    except ImportError:
        row["ref_us"] = None            # Pillow is not installed here: not measured
    out[name] = row
    print(name, row)

# DTU mask, 400x300: one launch (with the rest of the preparation of an unchanged-size image) against the 49-step loop
src = [torch.from_numpy(rng.integers(0, 60, (300, 400, 3), dtype=np.uint8)).to(dev)]
plain = events(lambda: _C.prepare_gt(src, [None], [None], 400, 300, False, 0.0))[0]
masked = events(lambda: _C.prepare_gt(src, [None], [None], 400, 300, False, G.DTU_THRESHOLD))[0]
gt = _C.prepare_gt(src, [None], [None], 400, 300, False, 0.0)[0][0]


def loop():
    m = gt.max(0, keepdim=True).values < 30 / 255
    c = m.clone()
    for i in range(1, 50):
        m[:, i:] *= c[:, :-i]
    return m.float()


out["dtu_400x300"] = {"with_mask_us": masked, "without_mask_us": plain, "torch_loop_us": events(loop)[0]}
assert torch.equal(loop(), _C.prepare_gt(src, [None], [None], 400, 300, False, G.DTU_THRESHOLD)[0][2])
print(json.dumps(out))
