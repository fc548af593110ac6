"""Depth priors in training: the scale- and shift-invariant Pearson depth loss of the sparse-view pipelines (FSGS, SparseGS over
the whole image; DNGaussian, SparseGS over local patches) on the device, and the preparation of the prior planes.

    L = w_global (1 - rho_image) + w_local mean over the counted patches of (1 - rho_patch)

between the rendered depth (or, mode "disparity", 1 / (depth + 1e-5)) and a prior plane that may come from any monocular
network, an RGB-D sensor or MVS.  include/b3gs_raster.h states every rule, csrc/depthprior.hip holds the kernels (two launches
per call for up to 8 views, fp64 in one fixed operation order, no host read, no allocation inside the library, no
floating-point atomic), tests/depth_prior_ref.py restates them in numpy.  The rasterizer's backward already takes
dL/d(rendered_depth): nothing there changes.

    depth_prior_loss / depth_prior_loss_batch   the loss as an autograd Function (capturable in a HIP graph)
    resize_priors / load_priors                 priors of any size -> the training size with a validity plane; a folder of them
    attach_priors                               ... onto the cameras of a scene (Camera.depth_prior / depth_prior_mask)
    align                                       a P + b: the prior in the render's units, from the loss's own sums
    PriorTerm                                   what the trainers share: weights, window, the patch-offset draws
"""
from __future__ import annotations

import os
import random
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MODES = {"depth": 0, "disparity": 1}
PARTS = ("loss", "global", "local", "n_used", "patches", "rho", "a", "b")


def _C():
    from . import _C as mod
    return mod


class _Workspace:
    """Per (device, W, H, patch, slot) persistent buffers, as fused_loss._Workspace: the gradient plane stays alive until
    backward uses it, so every view of a call (and every call of an iteration that names a slot) has its own."""
    _cache = {}

    @classmethod
    def get(cls, dev, W, H, patch, slot):
        key = (dev, W, H, patch, slot)
        if key not in cls._cache:
            n = _C().depth_prior_workspace_bytes(W, H, patch)
            if not n:
                raise ValueError(f"depth_prior_loss: {W}x{H} with patch {patch}: 1 <= W, H, W H <= 2^24, patch 0 or 8 .. 256")
            # (zeroed once: the arrival counter at the head of the workspace resets itself at the end of every call)
            cls._cache[key] = dict(ws=torch.zeros(n, dtype=torch.uint8, device=dev), parts=torch.zeros(8, dtype=torch.float64, device=dev),
                                   g_depth=torch.empty((1, H, W), dtype=torch.float32, device=dev), generation=0)
        return cls._cache[key]


class _DepthPriorLoss(torch.autograd.Function):
    """n views in one call: inputs (depth_0 .. depth_{n-1}) -> (loss_0, parts_0, .., loss_{n-1}, parts_{n-1})."""

    @staticmethod
    def forward(ctx, cfg, *depths):
        views, bufs = [], []
        for k, depth in enumerate(depths):
            alpha, prior, mask, off = cfg["planes"][k]
            if not depth.is_cuda:
                raise _lib.B3gsError("depth_prior_loss needs device tensors (no CPU fallback)")
            H, W = depth.shape[-2:]
            buf = _Workspace.get(depth.device, W, H, cfg["patch"], cfg["slot"] + k)
            bufs.append(buf)
            views.append((depth.detach().contiguous(), alpha.detach().contiguous(), prior.contiguous(), mask.contiguous(), off,
                          buf["g_depth"], buf["parts"], buf["ws"]))
        _C().depth_prior_loss(views, cfg["mode"], cfg["w_global"], cfg["w_local"], cfg["patch"], cfg["min_valid"], cfg["alpha_min"])
        for b in bufs:
            b["generation"] += 1
        # (backward reads the slot's gradient plane by reference: a later forward on the same slot replaces it, which the
        # generation number turns into an error instead of a wrong gradient)
        ctx.bufs, ctx.generations = bufs, [b["generation"] for b in bufs]
        ctx.grads = [b["g_depth"] for b in bufs]
        ctx.shapes = [d.shape for d in depths]
        out = []
        for b in bufs:
            parts = b["parts"].clone()
            out += [parts[0].to(torch.float32), parts]
        ctx.mark_non_differentiable(*out[1::2])
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        out = []
        for k, g in enumerate(ctx.grads):
            go = grads[2 * k]
            if go is not None and ctx.bufs[k]["generation"] != ctx.generations[k]:
                raise _lib.B3gsError("depth_prior_loss: the gradient plane of this slot was replaced by a later call before "
                                     "backward; give calls whose graphs are alive together different `slot`s")
            out.append(None if go is None else (g * go).reshape(ctx.shapes[k]))
        return (None, *out)


def _mask_plane(mask, like):
    if mask is None:
        return torch.ones(like.shape, dtype=torch.uint8, device=like.device)
    return mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)


def depth_prior_loss_batch(views: Sequence[dict], *, mode: str, w_global: float = 1.0, w_local: float = 0.0, patch: int = 0,
                           min_valid: int = 16, alpha_min: float = 0.0, slot: int = 0, return_parts: bool = False):
    """views: dicts with depth, alpha, prior [1,H,W] float32, mask [1,H,W] uint8 (None: all valid) and optionally offset (two
    ints) or offset_dev (int32 [2] on the device: read by the kernels, so a graph replay moves the grid); sizes may differ.
    -> per view the loss (float32 scalar on the device, differentiable in depth), or (loss, parts float64 [8]: PARTS)."""
    if mode not in MODES:
        raise ValueError(f'depth_prior_loss: mode is "depth" or "disparity", not {mode!r}')
    if not 1 <= len(views) <= 8:
        raise ValueError("depth_prior_loss_batch: 1 .. 8 views per call")
    planes = []
    for v in views:
        off = v.get("offset_dev")
        if off is None and v.get("offset") is not None:
            off = torch.tensor([int(v["offset"][0]), int(v["offset"][1])], dtype=torch.int32).to(v["depth"].device)
        planes.append((v["alpha"], v["prior"], _mask_plane(v.get("mask"), v["prior"]), off))
    cfg = dict(planes=planes, mode=MODES[mode], w_global=float(w_global), w_local=float(w_local), patch=int(patch),
               min_valid=int(min_valid), alpha_min=float(alpha_min), slot=int(slot))
    out = _DepthPriorLoss.apply(cfg, *[v["depth"] for v in views])
    return [(out[2 * k], out[2 * k + 1]) if return_parts else out[2 * k] for k in range(len(views))]


def depth_prior_loss(depth, alpha, prior, mask, *, mode: str, w_global: float = 1.0, w_local: float = 0.0, patch: int = 0,
                     min_valid: int = 16, alpha_min: float = 0.0, offset=None, offset_dev=None, slot: int = 0,
                     return_parts: bool = False):
    """One view of depth_prior_loss_batch.  `alpha` and `prior` get no gradient."""
    return depth_prior_loss_batch([dict(depth=depth, alpha=alpha, prior=prior, mask=mask, offset=offset, offset_dev=offset_dev)],
                                  mode=mode, w_global=w_global, w_local=w_local, patch=patch, min_valid=min_valid,
                                  alpha_min=alpha_min, slot=slot, return_parts=return_parts)[0]


def align(prior, parts):
    """a P + b with the least-squares (a, b) of the loss's image sums: the prior in the render's units (mode "disparity":
    in units of 1 / (depth + 1e-5))."""
    return (parts[6] * prior.to(torch.float64) + parts[7]).to(torch.float32)


def resize_priors(priors: Sequence[torch.Tensor], size, masks: Optional[Sequence] = None):
    """priors: float32 [Hsrc, Wsrc] device tensors of any sizes; size = (W, H) -> per prior (P float32 [1,H,W], M uint8
    [1,H,W]): bilinear at pixel centres, a pixel valid iff every tap of non-zero weight is finite, > 0 and unmasked."""
    W, H = int(size[0]), int(size[1])
    masks = [None] * len(priors) if masks is None else list(masks)
    return _C().resize_depth([p for p in priors], masks, W, H)


def _read_prior(directory: str, name: str):
    path = os.path.join(directory, name + ".npy")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"depth prior of view {name!r}: {path} does not exist (float32 / float64 [H,W] .npy)")
    a = np.load(path, allow_pickle=False)
    a = a[..., 0] if a.ndim == 3 and a.shape[-1] == 1 else a[0] if a.ndim == 3 and a.shape[0] == 1 else a
    if a.ndim != 2 or a.dtype not in (np.float32, np.float64):
        raise ValueError(f"{path}: a float32 / float64 [H,W] array is expected, not {a.dtype} {a.shape}")
    mask, mpath = None, os.path.join(directory, name + "_mask.png")
    if os.path.isfile(mpath):
        from .frames import read_png
        m = read_png(mpath)
        m = m if m.ndim == 2 else m[..., 0]
        if m.shape != a.shape:
            raise ValueError(f"{mpath}: {m.shape[1]}x{m.shape[0]}, its prior is {a.shape[1]}x{a.shape[0]}")
        mask = np.ascontiguousarray(m != 0).astype(np.uint8)
    return np.ascontiguousarray(a, dtype=np.float32), mask


def load_priors(directory: str, cameras, size=None, *, device="cuda"):
    """<directory>/<image_name>.npy per camera (float32 / float64 [H,W] of any size; <image_name>_mask.png, 8-bit, optional:
    non-zero = usable) -> per camera (P, M) at `size` = (W, H), default the camera's own.  frames.read_png reads 8-bit files
    only, so 16-bit PNG priors are not matched.  A missing file is a FileNotFoundError that names it."""
    host = [_read_prior(directory, str(c.image_name)) for c in cameras]
    out = []
    for c, (a, m) in zip(cameras, host):
        wh = (int(c.image_width), int(c.image_height)) if size is None else size
        out += resize_priors([torch.from_numpy(a).to(device)], wh, [None if m is None else torch.from_numpy(m).to(device)])
    return out


def attach_priors(directory: str, cameras, *, device="cuda") -> None:
    for c, (p, m) in zip(cameras, load_priors(directory, cameras, device=device)):
        c.depth_prior, c.depth_prior_mask = p, m


def has_prior(cam) -> bool:
    return getattr(cam, "depth_prior", None) is not None


def check_prior_set(cameras) -> bool:
    """True: every camera carries a prior; False: none does; a mixed set is a B3gsError."""
    n = sum(1 for c in cameras if has_prior(c))
    if n not in (0, len(cameras)):
        missing = [str(getattr(c, "image_name", i)) for i, c in enumerate(cameras) if not has_prior(c)]
        raise _lib.B3gsError(f"depth priors: {n} of {len(cameras)} training views carry a prior and {len(missing)} do not "
                             f"({', '.join(missing[:4])}): the graph trainer needs all or none")
    return n > 0


class PriorTerm:
    """The depth-prior term as the trainers share it: the weights, the iteration window and the patch-offset draws, which come
    from a random.Random(seed) of their own -- the view and shift draws of a run do not move when the term is switched on."""

    def __init__(self, *, mode="depth", weight=0.0, local=0.0, patch=0, from_iter=0, until_iter=None, alpha_min=0.0, min_valid=16,
                 seed=0):
        if mode not in MODES:
            raise ValueError(f'depth_prior_mode is "depth" or "disparity", not {mode!r}')
        self.mode, self.weight, self.local, self.patch = mode, float(weight), float(local), int(patch)
        self.from_iter, self.until_iter, self.alpha_min, self.min_valid = int(from_iter), until_iter, float(alpha_min), int(min_valid)
        if self.local != 0.0 and not 8 <= self.patch <= 256:
            raise ValueError("depth_prior_local needs depth_prior_patch in 8 .. 256")
        if self.local == 0.0:
            self.patch = 0
        self.rng = random.Random(seed)
        self._offsets = {}          # device -> (int32 [2] on the device, pinned ring): one buffer for the life of the term

    @property
    def enabled(self) -> bool:
        return self.weight != 0.0 or self.local != 0.0

    def active(self, it: int) -> bool:
        return self.enabled and it >= self.from_iter and (self.until_iter is None or it <= self.until_iter)

    def draw_offset(self):
        return (self.rng.randrange(self.patch), self.rng.randrange(self.patch)) if self.patch else (0, 0)

    def offset_buffer(self, device):
        """The term's int32 [2] on `device`: what the kernels read the patch offsets from (static: a captured graph keeps it)."""
        device = torch.device(device)
        if device not in self._offsets:
            from .camera import _PinnedRing
            self._offsets[device] = (torch.zeros(2, dtype=torch.int32, device=device), _PinnedRing(64, 2))
        return self._offsets[device][0]

    def upload_offset(self, offset, device):
        """offset -> offset_buffer(device): one asynchronous copy from a pinned row, no allocation"""
        buf = self.offset_buffer(device)
        ring = self._offsets[buf.device][1]
        k, row = ring.take()
        words = row.view(torch.int32)
        words[0], words[1] = int(offset[0]), int(offset[1])
        buf.copy_(words, non_blocking=True)
        ring.uploaded(k, buf.device)
        return buf

    def loss(self, cam, pkg, *, offset=None, offset_dev=None, slot=0, prior=None, mask=None):
        """The term of one rendered view (`pkg`: render()'s dict).  prior / mask: static planes in place of the camera's."""
        if offset_dev is None and self.patch:
            offset_dev = self.upload_offset(self.draw_offset() if offset is None else offset, pkg["rendered_depth"].device)
        offset = None
        return depth_prior_loss(pkg["rendered_depth"], pkg["rendered_alpha"], cam.depth_prior if prior is None else prior,
                                cam.depth_prior_mask if mask is None else mask, mode=self.mode, w_global=self.weight,
                                w_local=self.local, patch=self.patch, min_valid=self.min_valid, alpha_min=self.alpha_min,
                                offset=offset, offset_dev=offset_dev, slot=slot)

    def add(self, total, it, cam, pkg):
        """total + the term when this view carries a prior and `it` lies in the window; `total` itself otherwise (no call)."""
        if not has_prior(cam) or not self.active(it):
            return total
        return total + self.loss(cam, pkg)
