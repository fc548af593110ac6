#!/usr/bin/env python
"""usage (GPU box): python tools/undistort_time.py -- the undistorter at LLFF's source size, 4032x3024x3, SIMPLE_RADIAL:
  map      b3gs_undistort_map for the pinhole the sizing rule gives (events around the call, warm, median of 20): ms per map
  remap    b3gs_remap_batch for 8 images and for 1 (the same way): ms per image and bytes moved per second, counting the source
           once, the map once per launch and the output and valid plane once (what a perfect cache would move)
  copy     a device copy of the same number of bytes (torch's clone of a uint8 tensor), the rate to hold the remap against,
           beside the streaming rate DESIGN.md records for this part (adam_kernel: 4.9-5.9 TB/s)
Prints one JSON line.  No bar is fixed."""
import json
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import undistort as U            # noqa: E402

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


Ws, Hs, C = 4032, 3024, 3
cam = U.CameraModel("SIMPLE_RADIAL", Ws, Hs, (3300.0, Ws / 2 + 11.0, Hs / 2 - 7.0, -0.08))
pin = U.pinhole_for(cam, device=dev)
W, H = pin[:2]
out = {"source": [Ws, Hs, C], "pinhole": list(pin)}
med, best = events(lambda: U.undistort_map(cam, pin, dev))
out["map_ms"], out["map_best_ms"] = med, best
m = U.undistort_map(cam, pin, dev)
g = torch.Generator(device="cpu").manual_seed(0)
srcs = [torch.randint(0, 256, (Hs, Ws, C), dtype=torch.uint8, generator=g).to(dev) for _ in range(8)]
for n in (8, 1):
    part = srcs[:n]
    med, best = events(lambda: U.remap(part, m))
    nbytes = n * (Hs * Ws * C + H * W * C) + H * W * 8 + H * W
    out[f"remap_{n}"] = {"ms_per_image": med / n, "best_ms_per_image": best / n, "GBps": nbytes / med / 1e6, "bytes": nbytes}
    flat = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)          # a copy reads and writes: half the bytes each way
    cmed, _ = events(lambda: flat.clone())
    out[f"copy_{n}"] = {"ms": cmed, "GBps": nbytes / cmed / 1e6}
    print(f"remap of {n}: {med / n:.3f} ms per image, {nbytes / med / 1e6:.0f} GB/s; a device copy of the same bytes: "
          f"{nbytes / cmed / 1e6:.0f} GB/s; DESIGN.md's streaming kernels: {DESIGN_STREAM_TBPS[0]}-{DESIGN_STREAM_TBPS[1]} TB/s")
_, valid = U.remap(srcs[:1], m)
out["valid_fraction"] = float((valid == 255).float().mean())
print(f"map {W} x {H}: {out['map_ms']:.3f} ms")
print(json.dumps(out))
