#!/usr/bin/env python
"""usage (GPU box): python tools/poisson_time.py [res=128] [rounds=5] -- the screened Poisson stage (csrc/poisson.hip) on a sphere of
Fibonacci samples whose diameter spans `res` voxels in a grid of (res + 8)^3 nodes: the splat, conjugate-gradient iterations and
the level / support planes, timed with device events in blocks that ALTERNATE inside one process (tools/ab_interleaved.py says why)
with the same iteration written with torch slicing ops on the device (float32 tensors, torch.dot in float32: its sums are not the
stated trees, so it is the yardstick of the time, not a substitute).  One iteration = (solve of 2 n - solve of n iterations) / n with
tol = 0, which removes the right-hand side and the launch of the call.  Prints the median and best block of every setting, the
bytes one iteration must move (stencil: r, p, D in, p, Ap out; update: x, r, p, Ap in, x, r out = 44 bytes per node) divided by its
time, and the end-to-end time (splat + default solve + volume + extraction) beside a TSDF extraction on the same grid."""
import math
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import poisson  # noqa: E402

res = int(sys.argv[1]) if len(sys.argv) > 1 else 128
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
N_IT = 20
pad = 4
voxel = 2.0 / res
dims = (res + 2 * pad,) * 3
origin = (-1.0 - pad * voxel,) * 3
ns = int(4.0 * math.pi * (res / 2.0) ** 2 * 4)                       # about four samples per voxel of surface
k = np.arange(ns) + 0.5
z = 1.0 - 2.0 * k / ns
phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
nrm = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1).astype(np.float32)
pts, nr, w = torch.from_numpy(nrm).to(dev), torch.from_numpy(nrm).to(dev), torch.ones(ns, device=dev)

vol = poisson.PoissonVolume.from_dims(origin, dims, voxel, device=dev)
vol.splat(pts, nr, w)
density, vector = vol.density, vol.vector
n = density.numel()


def torch_apply(p, sd):
    q = torch.nn.functional.pad(p[None, None], (1, 1, 1, 1, 1, 1), mode="replicate")[0, 0]
    s = 6.0 * p - (q[1:-1, 1:-1, :-2] + q[1:-1, 1:-1, 2:] + q[1:-1, :-2, 1:-1] + q[1:-1, 2:, 1:-1] + q[:-2, 1:-1, 1:-1] + q[2:, 1:-1, 1:-1])
    return s + sd * p


def torch_cg(b, sd, iters):
    x, r, p = torch.zeros_like(b), b.clone(), b.clone()
    rr = torch.dot(r.flatten(), r.flatten())
    for _ in range(iters):
        ap = torch_apply(p, sd)
        alpha = rr / torch.dot(p.flatten(), ap.flatten())
        x += alpha * p
        r -= alpha * ap
        rn = torch.dot(r.flatten(), r.flatten())
        p = r + (rn / rr) * p
        rr = rn
    return x


info = vol.solve(poisson.SCREEN, N_IT, 0.0)
b, sd = vol.rhs.clone(), poisson.SCREEN * density
rel = float((torch_cg(b, sd, N_IT) - vol.x).norm() / vol.x.norm())
print(f"{dims[0]}^3 nodes, {ns} samples; {N_IT} iterations against the torch form: relative difference {rel:.2e}")


def end_to_end():
    vol.splat(pts, nr, w)
    vol.solve()
    return vol.extract(0.0)


def tsdf_extract():
    return vol.volume.extract(0.0)


SETTINGS = {
    "splat": lambda: vol.splat(pts, nr, w),
    f"solve {N_IT} iterations": lambda: vol.solve(poisson.SCREEN, N_IT, 0.0),
    f"solve {2 * N_IT} iterations": lambda: vol.solve(poisson.SCREEN, 2 * N_IT, 0.0),
    f"torch {N_IT} iterations": lambda: torch_cg(b, sd, N_IT),
    f"torch {2 * N_IT} iterations": lambda: torch_cg(b, sd, 2 * N_IT),
    "volume (level, support)": lambda: vol.to_tsdf(1),
    "end to end (splat, solve, extract)": end_to_end,
    "extraction alone (as after TSDF fusion)": tsdf_extract,
}
times = {name: [] for name in SETTINGS}
for r in range(rounds + 1):
    for name, call in SETTINGS.items():
        call()                                                        # warm-up of this block
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        e.record()
        torch.cuda.synchronize(dev)
        if r:                                                         # (the first round loads code objects)
            times[name].append(a.elapsed_time(e))
for name, t in times.items():
    print(f"{name:42s} median {statistics.median(t):9.3f} ms   best {min(t):9.3f} ms")


def per_iteration(prefix):
    lo, hi = (statistics.median(times[f"{prefix} {m} iterations"]) for m in (N_IT, 2 * N_IT))
    return (hi - lo) / N_IT


ours, theirs = per_iteration("solve"), per_iteration("torch")
must = 44 * n
done = vol.solve()
print(f"one iteration: {ours:.4f} ms (torch slicing form: {theirs:.4f} ms, {theirs / ours:.1f} x); it must move {must / 1e6:.1f} MB "
      f"-> {must / ours / 1e6:.0f} GB/s")
print(f"default solve: {done['iterations']} iterations, relative residual {done['residual']:.2e}")
