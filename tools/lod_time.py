"""Times lod.coarsen at 1M Gaussians, SH degree 3 (K = 15), at the cells that roughly halve and eighth the count, against a plain
torch implementation of the same moments on the same device: keys and torch.unique, index_add_ sums (float64), torch.linalg.eigh.
The baseline skips what it has no cheap form for (the order of the members, the stable output order, the quaternion); it is a
yardstick for the time, not for the bits.  Prints one JSON line.

python tools/lod_time.py [--P 1000000] [--reps 5]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(P, K, dev, seed=0):
    g = torch.Generator(dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=dev, generator=g)                       # noqa: E731
    n = lambda *s: torch.randn(*s, device=dev, generator=g)                      # noqa: E731
    pos = r(P, 3) * 10.0
    sc = torch.exp(r(P, 3) * (math.log(0.05) - math.log(0.005)) + math.log(0.005))
    return pos, sc, n(P, 4), r(P) * 0.9 + 0.05, n(P, 1, 3), n(P, K, 3) * 0.3


def torch_merge(pos, sc, quat, alpha, dc, rest, cell):
    P = pos.shape[0]
    c = torch.floor((pos - pos.amin(0)) / cell).long()
    key = c[:, 0] | (c[:, 1] << 10) | (c[:, 2] << 20)
    key = torch.where(sc.amax(1) <= cell, key, (1 << 30) + torch.arange(P, device=pos.device))
    _, inv = torch.unique(key, return_inverse=True)
    n = int(inv.max()) + 1
    d = torch.float64
    m = alpha.to(d) * sc.to(d).prod(1)
    M = torch.zeros(n, dtype=d, device=pos.device).index_add_(0, inv, m)
    mu = torch.zeros(n, 3, dtype=d, device=pos.device).index_add_(0, inv, m[:, None] * pos.to(d)) / M[:, None]
    q = quat.to(d) / quat.to(d).norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(P, 3, 3)
    L = R * sc.to(d)[:, None, :]
    dd = pos.to(d) - mu[inv]
    cov = L @ L.transpose(1, 2) + dd[:, :, None] * dd[:, None, :]
    Sig = torch.zeros(n, 3, 3, dtype=d, device=pos.device).index_add_(0, inv, m[:, None, None] * cov) / M[:, None, None]
    lam, V = torch.linalg.eigh(Sig)
    s = lam.clamp_min(1e-20).sqrt()
    al = (M / s.prod(1)).clamp(1 / 255, 0.99)
    f = torch.cat([dc, rest], 1).reshape(P, -1).to(d)
    col = torch.zeros(n, f.shape[1], dtype=d, device=pos.device).index_add_(0, inv, m[:, None] * f) / M[:, None]
    return mu.float(), s.float(), V.float(), al.float(), col.float()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--P", type=int, default=1000000)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args(argv)
    from binocular3dgs_amd import lod
    dev = "cuda"
    acts = make(a.P, 15, dev)
    res = {"P": a.P, "K": 15, "reps": a.reps, "levels": []}
    for ratio in (0.5, 0.125):
        cell = 10.0 / (a.P * ratio) ** (1.0 / 3.0)                              # about ratio * P occupied cells
        rows = lod.merge_activated(*acts, cell)[0].shape[0]
        ours = timed(lambda: lod.merge_activated(*acts, cell), a.reps)
        base = timed(lambda: torch_merge(*acts, cell), a.reps)
        res["levels"].append({"ratio": ratio, "cell": cell, "rows": rows, "hip_ms": round(ours, 3), "torch_ms": round(base, 3),
                              "torch_over_hip": round(base / ours, 2)})
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
