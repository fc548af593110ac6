#!/usr/bin/env python
"""usage (GPU box): python tools/mesh_smooth_time.py [side=1000] [rounds=9] -- the mesh smoothing stage (csrc/meshsmooth.hip) on a
synthetic noisy grid of side x side vertices (1000: 1M vertices, 2M triangles): the adjacency build, one step of the filter and the
vertex normals, timed with device events in blocks that ALTERNATE inside one process (tools/ab_interleaved.py says why) with a torch
formulation of the same step: index_add_ of the neighbours' fp64 positions over the directed edge list, then the same update.  The
torch form uses floating-point atomics, so its sums depend on the schedule: it is the yardstick of the time, not a substitute.
Prints the median and best block of every setting and the bytes per second of the step against the bytes it must move (every
buffer once: both position rows, the offsets, the pinned byte and the neighbour indices) and against the bytes it gathers (one
16-byte row per neighbour, mostly served by the caches).  One step = (smooth of 2 n steps - smooth of n steps) / n, which removes
the pack and unpack passes and the launch of the call."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from binocular3dgs_amd import _C, mesh_tools  # noqa: E402

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
dev = torch.device("cuda:0")
N_STEPS = 10

g = torch.Generator(device="cpu").manual_seed(0)
jj, ii = torch.meshgrid(torch.arange(side), torch.arange(side), indexing="ij")
v = torch.stack([ii.float(), jj.float(), 0.3 * torch.randn(side, side, generator=g)], dim=-1).reshape(-1, 3).to(dev)
q = (jj[:-1, :-1] * side + ii[:-1, :-1]).reshape(-1)
f = torch.stack([torch.stack([q, q + 1, q + side + 1], 1), torch.stack([q, q + side + 1, q + side], 1)], 1).reshape(-1, 3).int().to(dev)
V, F = v.shape[0], f.shape[0]

adj = mesh_tools.adjacency(v, f)
lists = adj.lists()
pairs = int(lists["neighbour_offsets"][-1])
off = lists["neighbour_offsets"].long()
deg = (off[1:] - off[:-1])
dst = torch.repeat_interleave(torch.arange(V, device=dev), deg)
src = lists["neighbour_indices"][:pairs].long()
move = ((deg > 0) & (lists["pinned"] == 0)).unsqueeze(1)
degf = deg.clamp(min=1).double().unsqueeze(1)


def torch_steps(x, n, k=0.5):
    for _ in range(n):
        s = torch.zeros(V, 3, dtype=torch.float64, device=dev).index_add_(0, dst, x[src].double())
        xd = x.double()
        x = torch.where(move, (xd + k * (s / degf - xd)).float(), x)
    return x


SETTINGS = {
    "build": lambda: mesh_tools.adjacency(v, f),
    f"smooth {N_STEPS} steps": lambda: _C.mesh_smooth(v, F, adj.workspace, N_STEPS, 0.5, 0.0, True),
    f"smooth {2 * N_STEPS} steps": lambda: _C.mesh_smooth(v, F, adj.workspace, 2 * N_STEPS, 0.5, 0.0, True),
    "normals": lambda: _C.mesh_vertex_normals(v, f, adj.workspace),
    f"torch index_add_ {N_STEPS} steps": lambda: torch_steps(v, N_STEPS),
    f"torch index_add_ {2 * N_STEPS} steps": lambda: torch_steps(v, 2 * N_STEPS),
}

same = torch.equal(_C.mesh_smooth(v, F, adj.workspace, 1, 0.5, 0.0, True), torch_steps(v, 1))
print(f"{V} vertices, {F} triangles, {pairs} directed pairs; one step equals the torch form bit for bit on this run: {same}")

times = {name: [] for name in SETTINGS}
for r in range(rounds + 1):
    for name, call in SETTINGS.items():
        call()                                                        # warm-up of this block
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(3):
            call()
        b.record()
        torch.cuda.synchronize(dev)
        if r:                                                         # (the first round loads code objects)
            times[name].append(a.elapsed_time(b) / 3.0)
for name, t in times.items():
    print(f"{name:32s} median {statistics.median(t):9.3f} ms   best {min(t):9.3f} ms")


def per_step(prefix):
    lo, hi = (statistics.median(times[f"{prefix} {n} steps"]) for n in (N_STEPS, 2 * N_STEPS))
    return (hi - lo) / N_STEPS


must = V * (16 + 16 + 4 + 1) + pairs * 4
gathered = pairs * 16
ours, theirs = per_step("smooth"), per_step("torch index_add_")
print(f"one step: {ours:.4f} ms (torch index_add_ form: {theirs:.4f} ms)")
print(f"bytes one step must move: {must / 1e6:.1f} MB -> {must / ours / 1e6:.1f} GB/s; with the gathered rows ({gathered / 1e6:.1f} MB): "
      f"{(must + gathered) / ours / 1e6:.1f} GB/s")
