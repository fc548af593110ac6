"""Normal priors in training: the normal of the rendered depth map (central differences of the back-projected points, the
depth-to-normal map of DN-Splatter / 2DGS / PGSR) and its loss against a target normal plane on the device,

    L = w_cos mean over the valid pixels of (1 - n.t)  +  w_l1 mean over the valid pixels of |n - t|_1

with gradients in the rendered depth AND the rendered alpha (z = depth / alpha: the render is not normalised), and the
preparation of the target planes.  The target may come from any monocular normal network (Omnidata, DSINE, StableNormal); a
detached features.render_normals plane works as a target too (the loss accepts any unit plane in the camera frame).
include/b3gs_raster.h states every rule, csrc/normalprior.hip holds the kernels (two launches per call for up to 8 views, fp64
in one fixed operation order, no host read, no allocation inside the library, no floating-point atomic),
tests/normal_prior_ref.py restates them in numpy.  The rasterizer's backward already takes dL/d(rendered_depth) and
dL/d(rendered_alpha): nothing there changes.

    depth_normals                                   the forward alone: (normals [3,H,W], valid uint8 [1,H,W])
    normal_prior_loss / normal_prior_loss_batch     the loss as an autograd Function (capturable in a HIP graph)
    resize_normals / load_normal_priors             priors of any size -> the training size, renormalised, with a validity plane
    attach_normal_priors                            ... onto the cameras of a scene (Camera.normal_prior / normal_prior_mask)
    NormalTerm                                      what the trainers share: weights, window, alpha_min

Camera frame: x right, y down, z forward (a surface that faces the camera has n_z < 0).  FRAMES names what a file may hold.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

FRAMES = ("opencv", "opengl", "world")
PARTS = ("loss", "cos", "l1", "n_valid", "mean_dot", "reserved")


def _C():
    from . import _C as mod
    return mod


def tanfov(cam):
    """(tan(FoVx / 2), tan(FoVy / 2)) of a camera, or the pair itself"""
    if isinstance(cam, (tuple, list)):
        return float(cam[0]), float(cam[1])
    return math.tan(float(cam.FoVx) * 0.5), math.tan(float(cam.FoVy) * 0.5)


def _check_alpha_min(alpha_min):
    if not float(alpha_min) > 0.0:
        raise ValueError(f"alpha_min > 0 (z = depth / alpha), not {alpha_min!r}")
    return float(alpha_min)


class _Workspace:
    """Per (device, W, H, slot) persistent buffers, as depth_prior._Workspace: the gradient planes stay alive until backward uses
    them, so every view of a call (and every call of an iteration that names a slot) has its own."""
    _cache = {}

    @classmethod
    def get(cls, dev, W, H, slot):
        key = (dev, W, H, slot)
        if key not in cls._cache:
            n = _C().normal_prior_workspace_bytes(W, H)
            if not n:
                raise ValueError(f"normal_prior_loss: {W}x{H}: 1 <= W, H, W H <= 2^24")
            # (zeroed once: the arrival counter at the head of the workspace resets itself at the end of every call)
            cls._cache[key] = dict(ws=torch.zeros(n, dtype=torch.uint8, device=dev), parts=torch.zeros(6, dtype=torch.float64, device=dev),
                                   g_depth=torch.empty((1, H, W), dtype=torch.float32, device=dev),
                                   g_alpha=torch.empty((1, H, W), dtype=torch.float32, device=dev), generation=0)
        return cls._cache[key]


class _NormalPriorLoss(torch.autograd.Function):
    """n views in one call: inputs (depth_0, alpha_0, .., depth_{n-1}, alpha_{n-1}) -> (loss_0, parts_0, .., loss_{n-1}, parts_{n-1})."""

    @staticmethod
    def forward(ctx, cfg, *planes):
        views, bufs = [], []
        for k in range(len(planes) // 2):
            depth, alpha = planes[2 * k], planes[2 * k + 1]
            target, mask, tfx, tfy, normals, valid = cfg["views"][k]
            if not depth.is_cuda:
                raise _lib.B3gsError("normal_prior_loss needs device tensors (no CPU fallback)")
            H, W = depth.shape[-2:]
            buf = _Workspace.get(depth.device, W, H, cfg["slot"] + k)
            bufs.append(buf)
            views.append((depth.detach().contiguous(), alpha.detach().contiguous(), target.contiguous(),
                          None if mask is None else mask.contiguous(), tfx, tfy, buf["g_depth"], buf["g_alpha"], normals, valid,
                          buf["parts"], buf["ws"]))
        _C().normal_prior_loss(views, cfg["w_cos"], cfg["w_l1"], cfg["alpha_min"])
        for b in bufs:
            b["generation"] += 1
        # (backward reads the slot's gradient planes by reference: a later forward on the same slot replaces them, which the
        # generation number turns into an error instead of a wrong gradient)
        ctx.bufs, ctx.generations = bufs, [b["generation"] for b in bufs]
        ctx.shapes = [p.shape for p in planes]
        out = []
        for b in bufs:
            parts = b["parts"].clone()
            out += [parts[0].to(torch.float32), parts]
        ctx.mark_non_differentiable(*out[1::2])
        return tuple(out)

    @staticmethod
    def backward(ctx, *grads):
        out = []
        for k, b in enumerate(ctx.bufs):
            go = grads[2 * k]
            if go is None:
                out += [None, None]
                continue
            if b["generation"] != ctx.generations[k]:
                raise _lib.B3gsError("normal_prior_loss: the gradient planes of this slot were replaced by a later call before "
                                     "backward; give calls whose graphs are alive together different `slot`s")
            out.append((b["g_depth"] * go).reshape(ctx.shapes[2 * k]) if ctx.needs_input_grad[1 + 2 * k] else None)
            out.append((b["g_alpha"] * go).reshape(ctx.shapes[2 * k + 1]) if ctx.needs_input_grad[2 + 2 * k] else None)
        return (None, *out)


def _mask_plane(mask):
    if mask is None:
        return None
    return mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8)


def normal_prior_loss_batch(views: Sequence[dict], *, w_cos: float = 1.0, w_l1: float = 0.0, alpha_min: float = 0.5, slot: int = 0,
                            return_parts: bool = False, return_normals: bool = False):
    """views: dicts with depth, alpha [1,H,W] float32, target [3,H,W] float32 (unit normals, camera frame), mask [1,H,W] uint8
    (None: all valid) and cam (a Camera, or the pair (tanfovx, tanfovy)); sizes may differ.
    -> per view the loss (float32 scalar on the device, differentiable in depth and alpha), or (loss, parts float64 [6]: PARTS)
    with return_parts, or (loss, parts, normals [3,H,W], valid uint8 [1,H,W]) with return_normals."""
    if not 1 <= len(views) <= 8:
        raise ValueError("normal_prior_loss_batch: 1 .. 8 views per call")
    alpha_min = _check_alpha_min(alpha_min)
    cfg_views, extra = [], []
    for v in views:
        tfx, tfy = tanfov(v["cam"])
        normals = valid = None
        if return_normals:
            H, W = v["depth"].shape[-2:]
            normals = torch.empty((3, H, W), dtype=torch.float32, device=v["depth"].device)
            valid = torch.empty((1, H, W), dtype=torch.uint8, device=v["depth"].device)
        extra.append((normals, valid))
        cfg_views.append((v["target"], _mask_plane(v.get("mask")), tfx, tfy, normals, valid))
    cfg = dict(views=cfg_views, w_cos=float(w_cos), w_l1=float(w_l1), alpha_min=alpha_min, slot=int(slot))
    planes = []
    for v in views:
        planes += [v["depth"], v["alpha"]]
    out = _NormalPriorLoss.apply(cfg, *planes)
    res = []
    for k in range(len(views)):
        if return_normals:
            res.append((out[2 * k], out[2 * k + 1], *extra[k]))
        else:
            res.append((out[2 * k], out[2 * k + 1]) if return_parts else out[2 * k])
    return res


def normal_prior_loss(depth, alpha, target, mask, cam, *, w_cos: float = 1.0, w_l1: float = 0.0, alpha_min: float = 0.5, slot: int = 0,
                      return_parts: bool = False, return_normals: bool = False):
    """One view of normal_prior_loss_batch.  `target` and `mask` get no gradient."""
    return normal_prior_loss_batch([dict(depth=depth, alpha=alpha, target=target, mask=mask, cam=cam)], w_cos=w_cos, w_l1=w_l1,
                                   alpha_min=alpha_min, slot=slot, return_parts=return_parts, return_normals=return_normals)[0]


def depth_normals(depth, alpha, cam, *, alpha_min: float = 0.5, mask=None):
    """The normal of a rendered depth map: depth, alpha [1,H,W] float32 on the device -> (normals float32 [3,H,W] in the camera
    frame, 0 where not valid; valid uint8 [1,H,W]).  Forward only; one launch."""
    alpha_min = _check_alpha_min(alpha_min)
    if not depth.is_cuda:
        raise _lib.B3gsError("depth_normals needs device tensors (no CPU fallback)")
    tfx, tfy = tanfov(cam)
    (n, v), = _C().depth_normals([(depth.detach().contiguous(), alpha.detach().contiguous(), _mask_plane(mask), tfx, tfy)], alpha_min)
    return n, v


def resize_normals(priors: Sequence[torch.Tensor], size, masks: Optional[Sequence] = None):
    """priors: float32 [3, Hsrc, Wsrc] device tensors of any sizes; size = (W, H) -> per prior (n float32 [3,H,W], M uint8
    [1,H,W]): bilinear at pixel centres per component, renormalised; a pixel is valid iff every tap of non-zero weight is finite
    and unmasked and the interpolated vector's squared length is at least 1/4."""
    W, H = int(size[0]), int(size[1])
    masks = [None] * len(priors) if masks is None else list(masks)
    return _C().resize_normals([p for p in priors], masks, W, H)


def to_camera_frame(n: np.ndarray, frame: str, cam=None) -> np.ndarray:
    """n [3,H,W] in `frame` -> the camera frame of the loss (x right, y down, z forward):
    "opencv" as it is; "opengl" (x right, y up, z towards the viewer) negates y and z; "world" rotates by the camera's
    world-to-view rotation (Camera.R is camera-to-world: n_cam = R^T n_world)."""
    if frame not in FRAMES:
        raise ValueError(f"normal_prior_frame is one of {FRAMES}, not {frame!r}")
    if frame == "opencv":
        return n
    if frame == "opengl":
        return n * np.array([1.0, -1.0, -1.0], n.dtype)[:, None, None]
    R = np.asarray(cam.R, np.float64)
    return np.einsum("ji,jhw->ihw", R, n.astype(np.float64)).astype(n.dtype)


def _read_normal_prior(directory: str, name: str):
    """-> (float32 [3,H,W] as stored, uint8 [H,W] mask or None)"""
    npy, png = os.path.join(directory, name + ".npy"), os.path.join(directory, name + ".png")
    if os.path.isfile(npy):
        a = np.load(npy, allow_pickle=False)
        if a.ndim != 3 or a.dtype not in (np.float32, np.float64) or 3 not in (a.shape[0], a.shape[-1]):
            raise ValueError(f"{npy}: a float32 / float64 [H,W,3] or [3,H,W] array is expected, not {a.dtype} {a.shape}")
        a = a.transpose(2, 0, 1) if a.shape[-1] == 3 else a      # ([3,H,3] reads as [H,W,3]: a three-row image is no prior)
        a, path = np.ascontiguousarray(a, dtype=np.float32), npy
    elif os.path.isfile(png):
        from .frames import read_png
        c = read_png(png)
        if c.ndim != 3 or c.shape[-1] < 3:
            raise ValueError(f"{png}: an 8-bit RGB file is expected, not {c.shape}")
        a = np.ascontiguousarray((2.0 * c[..., :3].astype(np.float32) / 255.0 - 1.0).transpose(2, 0, 1), dtype=np.float32)
        path = png
    else:
        raise FileNotFoundError(f"normal prior of view {name!r}: neither {npy} (float32 / float64 [H,W,3] or [3,H,W]) nor {png} "
                                f"(8-bit RGB, n = 2 c / 255 - 1) exists")
    mask, mpath = None, os.path.join(directory, name + "_mask.png")
    if os.path.isfile(mpath):
        from .frames import read_png
        m = read_png(mpath)
        m = m if m.ndim == 2 else m[..., 0]
        if m.shape != a.shape[1:]:
            raise ValueError(f"{mpath}: {m.shape[1]}x{m.shape[0]}, its prior {path} is {a.shape[2]}x{a.shape[1]}")
        mask = np.ascontiguousarray(m != 0).astype(np.uint8)
    return a, mask


def load_normal_priors(directory: str, cameras, size=None, *, frame: str = "opencv", device="cuda"):
    """<directory>/<image_name>.npy per camera (float32 / float64 [H,W,3] or [3,H,W] of any size) or <image_name>.png (8-bit
    RGB, n = 2 c / 255 - 1); <image_name>_mask.png, 8-bit, optional: non-zero = usable.  `frame`: what the files hold (FRAMES);
    converted to the camera frame once, here.  -> per camera (n, M) at `size` = (W, H), default the camera's own.  A missing file
    is a FileNotFoundError that names it."""
    if frame not in FRAMES:
        raise ValueError(f"normal_prior_frame is one of {FRAMES}, not {frame!r}")
    host = [_read_normal_prior(directory, str(c.image_name)) for c in cameras]
    out = []
    for c, (a, m) in zip(cameras, host):
        a = np.ascontiguousarray(to_camera_frame(a, frame, c), dtype=np.float32)
        wh = (int(c.image_width), int(c.image_height)) if size is None else size
        out += resize_normals([torch.from_numpy(a).to(device)], wh, [None if m is None else torch.from_numpy(m).to(device)])
    return out


def attach_normal_priors(directory: str, cameras, *, frame: str = "opencv", device="cuda") -> None:
    for c, (n, m) in zip(cameras, load_normal_priors(directory, cameras, frame=frame, device=device)):
        c.normal_prior, c.normal_prior_mask = n, m


def has_normal_prior(cam) -> bool:
    return getattr(cam, "normal_prior", None) is not None


def check_prior_set(cameras) -> bool:
    """True: every camera carries a normal prior; False: none does; a mixed set is a B3gsError."""
    n = sum(1 for c in cameras if has_normal_prior(c))
    if n not in (0, len(cameras)):
        missing = [str(getattr(c, "image_name", i)) for i, c in enumerate(cameras) if not has_normal_prior(c)]
        raise _lib.B3gsError(f"normal priors: {n} of {len(cameras)} training views carry a prior and {len(missing)} do not "
                             f"({', '.join(missing[:4])}): the graph trainer needs all or none")
    return n > 0


class NormalTerm:
    """The normal-prior term as the trainers share it: the weights, the iteration window and alpha_min (depth_prior.PriorTerm
    without the offset draws: the term draws nothing)."""

    def __init__(self, *, cos=0.0, l1=0.0, from_iter=0, until_iter=None, alpha_min=0.5):
        self.cos, self.l1 = float(cos), float(l1)
        self.from_iter, self.until_iter, self.alpha_min = int(from_iter), until_iter, _check_alpha_min(alpha_min)

    @property
    def enabled(self) -> bool:
        return self.cos != 0.0 or self.l1 != 0.0

    def active(self, it: int) -> bool:
        return self.enabled and it >= self.from_iter and (self.until_iter is None or it <= self.until_iter)

    def loss(self, cam, pkg, *, slot=0, target=None, mask=None):
        """The term of one rendered view (`pkg`: render()'s dict).  target / mask: static planes in place of the camera's."""
        return normal_prior_loss(pkg["rendered_depth"], pkg["rendered_alpha"], cam.normal_prior if target is None else target,
                                 cam.normal_prior_mask if mask is None else mask, cam, w_cos=self.cos, w_l1=self.l1,
                                 alpha_min=self.alpha_min, slot=slot)

    def add(self, total, it, cam, pkg):
        """total + the term when this view carries a prior and `it` lies in the window; `total` itself otherwise (no call)."""
        if not has_normal_prior(cam) or not self.active(it):
            return total
        return total + self.loss(cam, pkg)
