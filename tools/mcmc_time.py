"""python tools/mcmc_time.py [--points 1000000] [--reps 50]

Times, at 1M Gaussians on the device and interleaved in ONE process (A, B, A, B, ..: both sides see the same neighbours):

  noise      mcmc.inject_noise (one launch, 56 B per Gaussian) against the torch expression of the paper's code: a [P,3] normal
             tensor, the [P,3,3] covariance from build_rotation and the scales, a batched product and the sigmoid gate
  relocate   mcmc.relocate at 1 %, 10 % and 50 % dead against a torch implementation: torch.multinomial over the opacities,
             bincount, the correction as tensor expressions with a [51,51] binomial table, index copies of the six tensors and
             of their moments

Device events around every call, a warm-up of each shape, the median and the quartiles of --reps calls.  Prints one JSON line.
The relocation inputs are restored from a saved copy before every call (outside the events).  A measurement path without a
device fails; nothing here falls back.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_rotation(q):
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.empty((q.shape[0], 3, 3), device=q.device)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def torch_noise(model, lr, noise_lr=5e5):
    with torch.no_grad():
        L = build_rotation(model._rotation) * torch.exp(model._scaling).unsqueeze(1)
        cov = L @ L.transpose(1, 2)
        gate = 1.0 / (1.0 + torch.exp(100.0 * (torch.sigmoid(model._opacity) - 0.005)))
        noise = torch.randn_like(model._xyz) * gate * (noise_lr * lr)
        model._xyz.add_(torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1))


def torch_relocate(params, moments, binoms, min_opacity=0.005, n_max=51):
    with torch.no_grad():
        xyz, dc, rest, scaling, rotation, opacity = params
        o = torch.sigmoid(opacity).reshape(-1)
        dead = o <= min_opacity
        idx_dead = dead.nonzero(as_tuple=True)[0]
        if idx_dead.numel() == 0:
            return
        probs = torch.where(dead, torch.zeros_like(o), o)
        src = torch.multinomial(probs, idx_dead.numel(), replacement=True)
        count = torch.bincount(src, minlength=o.shape[0])
        N = (count[src] + 1).clamp(max=n_max)
        os_ = o[src]
        on = 1.0 - torch.pow(1.0 - os_, 1.0 / N.float())
        k = torch.arange(n_max, device=o.device)
        powers = on[:, None] ** (k[None] + 1).float() / torch.sqrt((k + 1).float())[None]           # [n, 51]
        sign = torch.where(k % 2 == 0, 1.0, -1.0)
        rows = (binoms[None] * (powers * sign[None])[:, None, :]).sum(dim=2)                        # [n, 51]: the inner sums
        inner = torch.cumsum(rows, dim=1)
        denom = inner.gather(1, (N - 1)[:, None]).reshape(-1)
        new_s = torch.log(torch.exp(scaling[src]) * (os_ / denom)[:, None])
        on = on.clamp(min_opacity, 1.0 - 2.0 ** -24)
        new_o = torch.log(on / (1.0 - on))[:, None]
        for t in (xyz, dc, rest, rotation):
            t[idx_dead] = t[src]
        opacity[idx_dead], scaling[idx_dead] = new_o, new_s
        opacity[src], scaling[src] = new_o, new_s
        for m in moments:
            m[src] = 0
            m[idx_dead] = 0


def timed(fn, before=None):
    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def quartiles(x):
    q = np.percentile(np.array(x), [25, 50, 75])
    return {"median_ms": round(float(q[1]), 4), "q25_ms": round(float(q[0]), 4), "q75_ms": round(float(q[2]), 4)}


def interleaved(fa, fb, reps, before_a=None, before_b=None, warmup=3):
    for _ in range(warmup):
        timed(fa, before_a), timed(fb, before_b)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(fa, before_a))
        tb.append(timed(fb, before_b))
    return quartiles(ta), quartiles(tb)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/mcmc_time.py measures on the device; none is visible")
    from binocular3dgs_amd import mcmc
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.step import FusedAdam
    P, dev = a.points, "cuda"
    g = torch.Generator().manual_seed(1)

    def model_with(dead_share):
        o = torch.rand(P, 1, generator=g) * 0.9 + 0.05
        o[torch.rand(P, generator=g) < dead_share] = 0.002
        return GaussianModel.from_tensors(torch.randn(P, 3, generator=g), torch.randn(P, 1, 3, generator=g), torch.randn(P, 3, 3, generator=g),
                                          torch.log(torch.rand(P, 3, generator=g) * 0.05 + 0.005), torch.randn(P, 4, generator=g),
                                          torch.log(o / (1 - o)), sh_degree=1, device=dev, requires_grad=False)

    res = {"points": P, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    m = model_with(0.3)
    with torch.no_grad():
        m._opacity.fill_(math.log(0.004 / 0.996))            # the gate open everywhere: both sides do all of their work
    it = [0]

    def hip_noise():
        it[0] += 1
        mcmc.inject_noise(m, 1.6e-4, iteration=it[0], seed=7)

    hn, tn = interleaved(hip_noise, lambda: torch_noise(m, 1.6e-4), a.reps)
    res["noise"] = {"hip": hn, "torch": tn, "hip_GBps": round(56.0 * P / (hn["median_ms"] * 1e-3) / 1e9, 1)}
    binoms = torch.tensor([[math.comb(i, k) if k <= i else 0 for k in range(51)] for i in range(51)], dtype=torch.float32, device=dev)
    res["relocate"] = {}
    for share in (0.01, 0.1, 0.5):
        m = model_with(share)
        opt = FusedAdam(m.parameters(), [1e-3] * 6)
        saved = [p.detach().clone() for p in m.parameters()]
        shaped = []
        off = 0
        for p in m.parameters():
            shaped += [opt.exp_avg[off:off + p.numel()].view_as(p), opt.exp_avg_sq[off:off + p.numel()].view_as(p)]
            off += p.numel()

        def restore():
            with torch.no_grad():
                for p, s in zip(m.parameters(), saved):
                    p.copy_(s)

        hr, tr = interleaved(lambda: mcmc.relocate(m, opt, iteration=5, seed=7), lambda: torch_relocate([p.detach() for p in m.parameters()], shaped, binoms),
                             max(5, a.reps // 5), restore, restore)
        res["relocate"][f"{share:g}"] = {"hip": hr, "torch": tr}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
