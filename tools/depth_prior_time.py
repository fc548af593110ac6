"""Times the depth-prior loss plus its gradient (binocular3dgs_amd/depth_prior.py, two launches per call) against the float32
torch restatement of the definition (tests/depth_prior_ref.py::torch_loss: pad, reshape, per-patch moments, autograd backward)
on the same device: 800x600, patch 64, one view and three views.  The two alternate in blocks in one process, as
tools/ab_interleaved.py does; medians over the blocks, and the launches of one call counted with torch's profiler.

    python tools/depth_prior_time.py [--blocks 9] [--calls 50]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--patch", type=int, default=64)
    args = ap.parse_args(argv)
    import depth_prior_ref as ref
    from binocular3dgs_amd import depth_prior as dp
    dev, W, H, p = "cuda:0", args.width, args.height, args.patch
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(mode="depth", w_global=1.0, w_local=1.0, patch=p, min_valid=16, alpha_min=0.5)
    for nviews in (1, 3):
        views = []
        for _ in range(nviews):
            d = (2 + torch.rand((1, H, W), device=dev, generator=g)).requires_grad_(True)
            views.append(dict(depth=d, alpha=torch.rand((1, H, W), device=dev, generator=g), prior=0.5 * d.detach() + torch.rand((1, H, W), device=dev, generator=g),
                              mask=(torch.rand((1, H, W), device=dev, generator=g) > 0.05).to(torch.uint8), offset_dev=torch.tensor([5, 9], dtype=torch.int32, device=dev)))

        def hip():
            torch.stack(dp.depth_prior_loss_batch(views, **kw)).sum().backward()

        def restated():
            sum(ref.torch_loss(v["depth"], v["alpha"], v["prior"], v["mask"], offset=(5, 9), **kw)[0] for v in views).backward()

        def launches(fn):
            fn()
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            on_device = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
            # (the library's two kernels by name; everything else is autograd's scalar handling around them)
            return sum(e.count for e in on_device), sum(e.count for e in on_device if "depth_prior_sums_kernel" in e.key or "depth_prior_grad_kernel" in e.key)

        times = {"hip": [], "restatement": []}
        for _ in range(args.blocks):
            for name, fn in (("hip", hip), ("restatement", restated)):
                fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.calls * 1e3)
        lh, lr = launches(hip), launches(restated)
        print(f"{nviews} view(s) {W}x{H} patch {p}: hip {statistics.median(times['hip']):.4f} ms ({lh[1]} library launches, {lh[0]} device "
              f"launches with autograd's), restatement {statistics.median(times['restatement']):.4f} ms ({lr[0]} device launches)")


if __name__ == "__main__":
    main()
