#!/usr/bin/env python
"""usage (GPU box): python tools/pose_time.py -- the camera pose gradient at 1M Gaussians (events around the call, warm, median of 20):
  kernel     b3gs_pose_gradient at sh_degree 3 for 1 view and for 8 views in one launch: ms and bytes per second, counting
             xyz, rotation, features_rest once and their gradients once per view (4 * (3 + 4 + 45) = 208 bytes per Gaussian for
             the parameters, 208 per Gaussian and view for the gradients)
  copy       a device copy of the bytes one view reads (torch's clone), the rate to hold it against
  camera_gradient   one pose.camera_gradient call at 800 x 600 (render, loss, autograd.grad of three tensors, the reduction),
             set against the render + backward of the same call without the reduction
Prints one JSON line.  No bar is fixed."""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, pose, synth                      # noqa: E402
from binocular3dgs_amd.render import PipelineParams, render        # noqa: E402

dev = torch.device("cuda")


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


P, W, H = 1_000_000, 800, 600
model = synth.synth_model(P, seed=0, device=dev, K=16, requires_grad=False)
model.active_sh_degree = 3
xyz, rot, rest = model._xyz.detach(), model._rotation.detach(), model._features_rest.detach().contiguous()
gen = torch.Generator(device=dev).manual_seed(0)
grads = [tuple(torch.randn(t.shape, device=dev, generator=gen) for t in (xyz, rot, rest)) for _ in range(8)]
out = {"P": P}
per_view = 4 * (3 + 4 + 45) * P
for V in (1, 8):
    o = torch.empty((V, 6), dtype=torch.float64, device=dev)
    gs = grads[:V]
    med, best = events(lambda: _C.pose_gradient(3, xyz, rot, rest, [g[0] for g in gs], [g[1] for g in gs], [g[2] for g in gs], None,
                                                [0.0, 0.0, 5.0], o))
    nbytes = per_view * (1 + V)
    out[f"kernel_{V}"] = {"ms": med, "best_ms": best, "bytes": nbytes, "GBps": nbytes / med / 1e6}
    print(f"b3gs_pose_gradient, degree 3, {V} view(s): {med:.3f} ms (best {best:.3f}), {nbytes / med / 1e6:.0f} GB/s")
flat = torch.empty(2 * per_view, dtype=torch.uint8, device=dev)
cmed, _ = events(lambda: flat.clone())
out["copy"] = {"ms": cmed, "GBps": 2 * per_view / cmed / 1e6}
print(f"a device copy of one view's bytes: {cmed:.3f} ms, {2 * per_view / cmed / 1e6:.0f} GB/s read (and as much written)")

cam = synth.synth_cameras(W, H, yaws=(3.0,), device=dev)[0]
bg = torch.zeros(3, device=dev)
gc, gd, ga = synth.synth_pixel_grads(W, H, seed=0, device=dev)
loss_fn = lambda o: (o["render"] * gc).sum() + (o["depth"] * gd).sum() + (o["alpha"] * ga).sum()   # noqa: E731
pipe = PipelineParams()
params = [model._xyz, model._rotation, model._features_rest]


def render_backward():
    for p in params:
        p.requires_grad_(True)
    pkg = render(cam, model, pipe, bg)
    o = dict(pkg, depth=pkg["rendered_depth"], alpha=pkg["rendered_alpha"])
    torch.autograd.grad(loss_fn(o), params)
    for p in params:
        p.requires_grad_(False)


med, best = events(lambda: pose.camera_gradient(model, cam, pipe, bg, loss_fn, pivot=[0.0, 0.0, 5.0]), n=10)
rmed, rbest = events(render_backward, n=10)
out["camera_gradient"] = {"ms": med, "best_ms": best, "render_backward_ms": rmed, "render_backward_best_ms": rbest}
print(f"camera_gradient at {W}x{H}: {med:.3f} ms; the same render + backward without the reduction: {rmed:.3f} ms")
print(json.dumps(out))
