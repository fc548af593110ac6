"""Times the normal-prior loss plus its gradients in depth and alpha (binocular3dgs_amd/normal_prior.py, two launches per call)
against a float32 torch restatement of the same loss (the validity rule in torch, then tests/normal_prior_ref.py::torch_loss and
autograd's backward) on the same device: 800x600, one view and three views.  The two alternate in blocks in one process, as
tools/depth_prior_time.py does; medians over the blocks, and the launches of one call counted with torch's profiler.

    python tools/normal_prior_time.py [--blocks 9] [--calls 50]"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

TANFOV, ALPHA_MIN, W_COS, W_L1 = (0.62, 0.47), 0.5, 1.0, 0.5


def valid_set(alpha, mask):
    """interior pixels whose five-point stencil is usable and whose target is unmasked (the c.c > 0 rule never bites on a
    smooth depth; the restatement is allowed to skip it)"""
    u = (alpha[0] >= ALPHA_MIN).float()[None, None]
    five = Fn.conv2d(u, torch.tensor([[0.0, 1, 0], [1, 1, 1], [0, 1, 0]], device=alpha.device)[None, None], padding=1)[0, 0] == 5
    five[0, :] = five[-1, :] = False
    five[:, 0] = five[:, -1] = False
    return five & (mask[0] != 0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    args = ap.parse_args(argv)
    import normal_prior_ref as ref
    from binocular3dgs_amd import normal_prior as npr
    dev, W, H = "cuda:0", args.width, args.height
    g = torch.Generator(device=dev).manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev) / H, torch.arange(W, device=dev) / W, indexing="ij")
    for nviews in (1, 3):
        views = []
        for k in range(nviews):
            a = (0.45 + 0.55 * torch.rand((1, H, W), device=dev, generator=g)).requires_grad_(True)
            z = 2 + 0.5 * xs + 0.3 * ys + 0.2 * torch.sin(5 * xs + k) * torch.cos(4 * ys)
            d = (z[None] * a.detach()).requires_grad_(True)
            t = Fn.normalize(0.3 * torch.randn((3, H, W), device=dev, generator=g) + torch.tensor([0.0, 0.0, -1.0], device=dev)[:, None, None], dim=0)
            views.append(dict(depth=d, alpha=a, target=t, mask=(torch.rand((1, H, W), device=dev, generator=g) > 0.05).to(torch.uint8), cam=TANFOV))

        def hip():
            torch.stack(npr.normal_prior_loss_batch(views, w_cos=W_COS, w_l1=W_L1, alpha_min=ALPHA_MIN)).sum().backward()

        def restated():
            sum(ref.torch_loss(v["depth"], v["alpha"], v["target"], valid_set(v["alpha"].detach(), v["mask"]), *TANFOV, w_cos=W_COS,
                               w_l1=W_L1)[0] for v in views).backward()

        def launches(fn):
            fn()
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            on_device = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
            # (the library's two kernels by name; everything else is autograd's scalar handling around them)
            return sum(e.count for e in on_device), sum(e.count for e in on_device if "normal_prior_forward_kernel" in e.key or "normal_prior_gather_kernel" in e.key)

        hip()
        restated()
        torch.cuda.synchronize()
        one = views[0]
        lh = float(npr.normal_prior_loss(one["depth"], one["alpha"], one["target"], one["mask"], TANFOV, w_cos=W_COS, w_l1=W_L1, alpha_min=ALPHA_MIN, slot=9))
        lr = float(ref.torch_loss(one["depth"], one["alpha"], one["target"], valid_set(one["alpha"].detach(), one["mask"]), *TANFOV, w_cos=W_COS, w_l1=W_L1)[0])
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
        nh, nr = launches(hip), launches(restated)
        print(f"{nviews} view(s) {W}x{H}: hip {statistics.median(times['hip']):.4f} ms ({nh[1]} library launches, {nh[0]} device "
              f"launches with autograd's), restatement {statistics.median(times['restatement']):.4f} ms ({nr[0]} device launches); "
              f"loss of the first view {lh:.6f} / {lr:.6f}")


if __name__ == "__main__":
    main()
