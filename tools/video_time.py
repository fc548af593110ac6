#!/usr/bin/env python
"""usage (GPU box): python tools/video_time.py [P NVIEWS BLOCKS] -- seconds per rendered path through frames.render_path, three
ways compared INTERLEAVED inside one process (blocks alternate, medians, as tools/ab_interleaved.py does):
  png    PNG files only (out_dir): raw frames copied to the host, zlib on PNG_THREADS threads
  video  video only (video=..., png=False): baseline JPEG on the device, three Motion-JPEG AVI files
  both   PNG files and the videos
at 800x600 and 504x378.  Also the device time of the JPEG launches of one batch (3 streams of 8 frames, HIP events around
_C.jpeg_encode alone) and the bytes copied to the host per frame.  Default: 1M Gaussians, 180 cameras, 3 blocks.
Prints the times of every block, their medians and one JSON line."""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, frames, synth          # noqa: E402

P, NV, BLOCKS = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (1_000_000, 180, 3)
dev = "cuda"
res = {"P": P, "views": NV, "blocks": BLOCKS}

for W, H in ((800, 600), (504, 378)):
    model = synth.synth_model(P, seed=0, device=dev, width=W, height=H)
    cams = synth.synth_cameras(W, H, yaws=tuple(-30.0 + 60.0 * k / NV for k in range(NV)), device=dev)
    bg = torch.zeros(3, device=dev)
    tmp = tempfile.mkdtemp(prefix="video_time_")

    def run(mode, cams=cams):
        out = os.path.join(tmp, mode)
        shutil.rmtree(out, ignore_errors=True)
        if mode == "png":
            frames.render_path(model, cams, bg, out)
        elif mode == "video":
            frames.render_path(model, cams, bg, video=(out, "t"), png=False)
        else:
            frames.render_path(model, cams, bg, out, video=(out, "t"))

    modes = ("png", "video", "both")
    for m in modes:                       # warm-up: kernels loaded, renderer sized, allocator and the JPEG room warm
        run(m, cams[:16])
    times = {m: [] for m in modes}
    for blk in range(BLOCKS):
        for m in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(m)
            torch.cuda.synchronize()
            times[m].append(time.perf_counter() - t0)
    video_bytes = sum(os.path.getsize(os.path.join(tmp, "video", n)) for n in os.listdir(os.path.join(tmp, "video")))
    png_bytes = sum(os.path.getsize(os.path.join(tmp, "png", n)) for n in os.listdir(os.path.join(tmp, "png")))
    shutil.rmtree(tmp, ignore_errors=True)

    # device time of the JPEG launches of one batch: the three streams of 8 frames
    batch = frames.render_path(model, cams[:8], bg)
    cap = frames._jpeg_capacity.get((H, W, 90), H * W * 3 // 8 + 1024)
    qt = frames._device_qtables(90, dev)
    out = torch.empty(8 * cap, dtype=torch.uint8, device=dev)
    lengths = torch.empty(8, dtype=torch.int64, device=dev)
    ms = []
    for rep in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in ("rgb", "depth", "cdepth"):
            _C.jpeg_encode([f[k] for f in batch], qt, out, cap, lengths)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    tag = f"{W}x{H}"
    for m in modes:
        res[f"{tag}_{m}_s_median"] = round(statistics.median(times[m]), 3)
        print(f"{tag} {m:5s} s/path  median {statistics.median(times[m]):7.3f}  blocks {[round(x, 3) for x in times[m]]}")
    res[f"{tag}_video_over_png"] = round(res[f"{tag}_video_s_median"] / res[f"{tag}_png_s_median"], 3)
    res[f"{tag}_jpeg_device_ms_per_batch"] = round(statistics.median(ms[1:]), 3)
    res[f"{tag}_host_bytes_per_frame_png"] = 3 * H * W
    res[f"{tag}_host_bytes_per_frame_video"] = cap + 8
    res[f"{tag}_video_files_bytes"] = video_bytes
    res[f"{tag}_png_files_bytes"] = png_bytes
    print(f"{tag} JPEG launches of one batch (3 x 8 frames): {res[f'{tag}_jpeg_device_ms_per_batch']} ms on the device; "
          f"host copy per frame {cap + 8} B (video) vs {3 * H * W} B (png)")
print(json.dumps(res))
