#!/usr/bin/env python
"""usage (GPU box): python tools/lpips_time.py [PAIRS W H] -- views per second of lpips.lpips() for 8 pairs at 800x600 with
random_weights(0), INTERLEAVED inside one process (as tools/ab_interleaved.py does: both settings see the same host) with the
same network written with torch.nn.functional.conv2d / max_pool2d on the same device; median and best round per setting, the
largest relative difference of the per-layer terms between the two."""
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from binocular3dgs_amd import lpips as LP            # noqa: E402

n, W, H = (int(x) for x in sys.argv[1:4]) if len(sys.argv) >= 4 else (8, 800, 600)
dev = torch.device("cuda:0")
w = LP.random_weights(0)
gen = torch.Generator(device=dev).manual_seed(0)
x = torch.rand(n, 3, H, W, device=dev, generator=gen)
y = (x + 0.1 * torch.randn(n, 3, H, W, device=dev, generator=gen)).clamp(0, 1)
cw = [t.to(dev) for t in w.conv_w]
cb = [t.to(dev) for t in w.conv_b]
lin = [t.to(dev) for t in w.lin]
shift = torch.tensor(w.shift, device=dev)[None, :, None, None]
scale = torch.tensor(w.scale, device=dev)[None, :, None, None]


def torch_layers(a, b):
    """lpipsPyTorch's statements with torch's own kernels, float32, one pair at a time (as metrics.py calls it)."""
    out = []
    for i in range(a.shape[0]):
        t = (torch.cat([a[i:i + 1], b[i:i + 1]]) - shift) / scale
        terms = []
        for l in range(13):
            if l in (2, 4, 7, 10):
                t = F.max_pool2d(t, 2, 2)
            t = F.relu(F.conv2d(t, cw[l], cb[l], padding=1))
            if l in LP.TAP_AFTER:
                f = t / (torch.sqrt((t ** 2).sum(1, keepdim=True)) + 1e-10)
                d = (f[0] - f[1]) ** 2
                terms.append((d * lin[len(terms)][:, None, None]).sum(0).mean())
        out.append(torch.stack(terms))
    return torch.stack(out)


SETTINGS = {"hip": lambda: LP.lpips_layers(x, y, w), "torch": lambda: torch_layers(x, y)}
with torch.no_grad():
    got = {k: f().double() for k, f in SETTINGS.items()}
    torch.cuda.synchronize(dev)
    rates = {k: [] for k in SETTINGS}
    for _ in range(5):
        for k, f in SETTINGS.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            rates[k].append(n / (time.perf_counter() - t0))
    rel = float(((got["hip"] - got["torch"]).abs() / got["torch"].abs()).max())
    print(f"{n} pairs {W}x{H}: " + " | ".join(f"{k}: median {statistics.median(v):.2f} best {max(v):.2f} views/s" for k, v in rates.items())
          + f" | largest relative difference of the layer terms {rel:.2e}")
