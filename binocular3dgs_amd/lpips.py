"""LPIPS (VGG16, version 0.1) on the device: the third number of the reference's metrics.py:103-117.

    lpips(render, gt, net_type='vgg')      lpipsPyTorch/__init__.py, modules/lpips.py:30-36, modules/networks.py:88-96

The network's arithmetic is csrc/lpips.hip (thirteen 3x3 convolutions on the exact-f32 MFMA, four max-pools, five taps; the
statements are in include/b3gs_raster.h).  The weights are the two files anyone who ran the reference already has -- torchvision's
`vgg16-397923af.pth` and the LPIPS package's `v0.1/vgg.pth` -- given as PATHS: nothing is ever fetched.  Convert them once:

    w = load_weights("vgg16-397923af.pth", "vgg.pth");  save_weights("lpips_vgg.npz", w);  w = load_weights("lpips_vgg.npz")

Images are [n,3,H,W] float32 in [0,1], fed unchanged as the reference does (metrics.py:95-105); normalize=True maps them to
2x - 1 first, the LPIPS package's switch.  There is no CPU path: tests/lpips_ref.py holds the PyTorch statement.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
VGG_LAYERS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # indices of the convolutions in torchvision's vgg16().features
TAP_AFTER = (1, 3, 6, 9, 12)                                     # convolution whose ReLU is tapped: relu1_2 .. relu5_3
TAP_C = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)                                    # networks.py:41-44
SCALE = (.458, .448, .450)
MAX_PAIRS = 8                                                    # B3GS_LPIPS_MAX_PAIRS
MIN_SIDE = 16                                                    # B3GS_LPIPS_MIN_SIDE


class LpipsWeights:
    """13 convolution (weight [Cout,Cin,3,3], bias [Cout]) pairs, 5 `lin` vectors [C_l], shift and scale (3 floats each), float32
    on the CPU.  `.to(device)` repacks the convolutions once for the kernels ([K', Cout], row 9 c + 3 ky + kx) and keeps them."""

    def __init__(self, conv_w: Sequence[torch.Tensor], conv_b: Sequence[torch.Tensor], lin: Sequence[torch.Tensor],
                 shift: Sequence[float] = SHIFT, scale: Sequence[float] = SCALE):
        self.conv_w = [_f32(w) for w in conv_w]
        self.conv_b = [_f32(b) for b in conv_b]
        self.lin = [_f32(v) for v in lin]
        self.shift = tuple(float(np.float32(v)) for v in shift)
        self.scale = tuple(float(np.float32(v)) for v in scale)
        if len(self.conv_w) != 13 or len(self.conv_b) != 13 or len(self.lin) != 5 or len(self.shift) != 3 or len(self.scale) != 3:
            raise ValueError("LpipsWeights: 13 weights, 13 biases, 5 lin vectors, 3 shifts, 3 scales")
        for i in range(13):
            _shape(self.conv_w[i], (CONV_COUT[i], CONV_CIN[i], 3, 3), f"conv {i} weight")
            _shape(self.conv_b[i], (CONV_COUT[i],), f"conv {i} bias")
        for l in range(5):
            _shape(self.lin[l], (TAP_C[l],), f"lin {l}")
        self.device = torch.device("cpu")
        self._packed: Dict[torch.device, "LpipsWeights"] = {}
        self.packed = None              # on a device: (conv_w [K', Cout] x 13, conv_b x 13, lin x 5)

    def to(self, device) -> "LpipsWeights":
        device = torch.device(device)
        if device.type == "cuda" and device.index is None and torch.cuda.is_available():
            device = torch.device("cuda", torch.cuda.current_device())
        if self.packed is not None and device == self.device:
            return self
        hit = self._packed.get(device)
        if hit is None:
            hit = LpipsWeights(self.conv_w, self.conv_b, self.lin, self.shift, self.scale)
            pw = []
            for i, w in enumerate(self.conv_w):
                p = w.reshape(CONV_COUT[i], 9 * CONV_CIN[i]).t().contiguous()
                if i == 0:                     # K = 27: one zero row, the kernels step k in pairs
                    p = torch.cat([p, torch.zeros(1, CONV_COUT[0])])
                pw.append(p.to(device))
            hit.packed = (pw, [b.to(device) for b in self.conv_b], [v.to(device) for v in self.lin])
            hit.device = device
            self._packed[device] = hit
        return hit


def _f32(t) -> torch.Tensor:
    return torch.as_tensor(t).detach().to("cpu", torch.float32).contiguous()


def _shape(t: torch.Tensor, shape, key: str):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{key}: shape {tuple(t.shape)}, expected {tuple(shape)}")


def _take(sd, key: str, shape, path: str) -> torch.Tensor:
    if key not in sd:
        raise ValueError(f"{path}: key {key} is missing")
    t = torch.as_tensor(sd[key])
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{path}: key {key} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def load_weights(vgg_path: str, lin_path: Optional[str] = None) -> LpipsWeights:
    """load_weights(npz) reads what save_weights wrote; load_weights(vgg_path, lin_path) reads torchvision's VGG16 state dict
    (features.<i>.weight / .bias) and the LPIPS package's v0.1 vgg.pth (lin<l>.model.1.weight, [1,C,1,1]).  Files only: a
    missing key or a wrong shape is a ValueError that names the key."""
    if lin_path is None:
        with np.load(vgg_path) as z:
            sd = {k: z[k] for k in z.files}
        cw = [_take(sd, f"conv{i}.weight", (CONV_COUT[i], CONV_CIN[i], 3, 3), vgg_path) for i in range(13)]
        cb = [_take(sd, f"conv{i}.bias", (CONV_COUT[i],), vgg_path) for i in range(13)]
        lin = [_take(sd, f"lin{l}", (TAP_C[l],), vgg_path) for l in range(5)]
        return LpipsWeights(cw, cb, lin, _take(sd, "shift", (3,), vgg_path).tolist(), _take(sd, "scale", (3,), vgg_path).tolist())
    vgg = torch.load(vgg_path, map_location="cpu", weights_only=True)
    lins = torch.load(lin_path, map_location="cpu", weights_only=True)
    cw = [_take(vgg, f"features.{k}.weight", (CONV_COUT[i], CONV_CIN[i], 3, 3), vgg_path) for i, k in enumerate(VGG_LAYERS)]
    cb = [_take(vgg, f"features.{k}.bias", (CONV_COUT[i],), vgg_path) for i, k in enumerate(VGG_LAYERS)]
    lin = [_take(lins, f"lin{l}.model.1.weight", (1, TAP_C[l], 1, 1), lin_path).reshape(TAP_C[l]) for l in range(5)]
    return LpipsWeights(cw, cb, lin)


def save_weights(path: str, weights: LpipsWeights) -> None:
    """One .npz with everything lpips() needs (conv<i>.weight, conv<i>.bias, lin<l>, shift, scale), float32."""
    arrays = {"shift": np.asarray(weights.shift, np.float32), "scale": np.asarray(weights.scale, np.float32)}
    for i in range(13):
        arrays[f"conv{i}.weight"] = weights.conv_w[i].numpy()
        arrays[f"conv{i}.bias"] = weights.conv_b[i].numpy()
    for l in range(5):
        arrays[f"lin{l}"] = weights.lin[l].numpy()
    with open(path, "wb") as fp:
        np.savez(fp, **arrays)


def random_weights(seed: int = 0) -> LpipsWeights:
    """He-scaled normal convolution weights, 0.05 * normal biases, uniform [0,1) lin vectors from a seeded CPU generator: what
    the tests and tools/lpips_time.py run on (activations keep their scale through the thirteen layers)."""
    gen = torch.Generator().manual_seed(int(seed))
    cw, cb = [], []
    for cin, cout in zip(CONV_CIN, CONV_COUT):
        cw.append(torch.randn(cout, cin, 3, 3, generator=gen) * float(np.sqrt(2.0 / (9 * cin))))
        cb.append(0.05 * torch.randn(cout, generator=gen))
    lin = [torch.rand(c, generator=gen) for c in TAP_C]
    return LpipsWeights(cw, cb, lin)


def _stack(x) -> torch.Tensor:
    if isinstance(x, (list, tuple)):
        x = torch.stack(list(x))
    return x[None] if x.dim() == 3 else x


def _chunk(n: int, H: int, W: int, max_workspace_bytes: int) -> int:
    """Pairs per call: at most 8, and at most what `max_workspace_bytes` of workspace holds (never less than 1)."""
    from . import _lib
    L = _lib.lib()
    k = min(n, MAX_PAIRS)
    while k > 1 and L.b3gs_lpips_workspace_bytes(k, H, W) > max_workspace_bytes:
        k -= 1
    return k


def lpips_layers(x, y, weights: LpipsWeights, normalize: bool = False, max_workspace_bytes: int = 1 << 30) -> torch.Tensor:
    """The five per-layer terms of every pair: float64 [n,5] on the device.  x, y: [n,3,H,W] (or [3,H,W], or a list of them).
    Any n: cut into calls of at most 8 pairs and `max_workspace_bytes` of workspace; a pair's bits do not depend on the cut."""
    from . import _C
    x, y = _stack(x), _stack(y)
    w = weights.to(x.device)
    cw, cb, lin = w.packed
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError("lpips: x and y must be [n,3,H,W] of one shape")
    n, _, H, W = x.shape
    if n == 0:
        return torch.empty((0, 5), dtype=torch.float64, device=x.device)
    k = _chunk(n, H, W, int(max_workspace_bytes)) if x.is_cuda and H >= MIN_SIDE and W >= MIN_SIDE else min(n, MAX_PAIRS)
    parts = [_C.lpips_layers(x[i:i + k], y[i:i + k], cw, cb, lin, list(w.shift), list(w.scale), bool(normalize))
             for i in range(0, n, k)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def lpips(x, y, weights: LpipsWeights, normalize: bool = False, max_workspace_bytes: int = 1 << 30) -> torch.Tensor:
    """lpips(x, y, net_type='vgg') of every pair: float64 [n] on the device, the sum of the five layer terms (lpips.py:36)."""
    return lpips_layers(x, y, weights, normalize, max_workspace_bytes).sum(1)


def features(x, weights: LpipsWeights, normalize: bool = False, max_workspace_bytes: int = 1 << 30) -> List[torch.Tensor]:
    """The five tap feature maps relu1_2 .. relu5_3 before normalisation: float32 [n,C_l,H_l,W_l] on the device."""
    from . import _C
    x = _stack(x)
    w = weights.to(x.device)
    cw, cb, _ = w.packed
    if x.dim() != 4:
        raise ValueError("lpips: x must be [n,3,H,W]")
    n, _, H, W = x.shape
    k = _chunk(n, H, W, int(max_workspace_bytes)) if x.is_cuda and n and H >= MIN_SIDE and W >= MIN_SIDE else min(max(n, 1), MAX_PAIRS)
    parts = [_C.lpips_features(x[i:i + k], cw, cb, list(w.shift), list(w.scale), bool(normalize)) for i in range(0, n, k)]
    return [torch.cat([p[l] for p in parts]) if len(parts) > 1 else parts[0][l] for l in range(5)]
