"""Per-image exposure compensation: the learned 3x4 affine colour transform of upstream 3DGS, applied to a render before the
loss so that the model stays in one canonical exposure while every photo of an auto-exposed capture keeps its own brightness
and tint; and its counterpart at evaluation, the closed-form best transform between a held-out render and its photo (the
colour-corrected PSNR of RawNeRF / Zip-NeRF).

    out_c = t_c + a_c0 r + a_c1 g + a_c2 b,   row c of A [3,4] = [a_c0 a_c1 a_c2 t_c],   no clamp,   identity [I | 0]

include/b3gs_raster.h states every rule, csrc/exposure.hip holds the kernels (fp64 in one fixed operation order, one rounding
to float32, no floating-point atomic, no host read, no allocation inside the library), tests/exposure_ref.py restates them in
numpy.  Renders, spirals, meshes and every other tool stay in canonical exposure: nothing but the trainers and `evaluate
--fit_exposure` reads a matrix.

    apply_exposure / apply_exposure_batch   autograd Functions: differentiable in the image and in A (capturable in a HIP graph)
    fit_exposure                            per view the least-squares A between a render and a photo, and a degeneracy flag
    ExposureTerm                            what the trainers share: the table [V,3,4], its row-sparse Adam, the schedule
    write_matrices / read_matrices          exposure.json: {image_name: 3x4}, upstream's layout
"""
from __future__ import annotations

import json
from typing import Optional, Sequence

import torch

from . import _lib

MAX_PLANES = 8


def _C():
    from . import _C as mod
    return mod


def _dev(device) -> torch.device:
    """`device` with its index spelled out ("cuda" and "cuda:0" name one set of buffers)"""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def identity(n=None, device="cpu"):
    eye = torch.eye(3, 4, dtype=torch.float32, device=device)
    return eye if n is None else eye[None].repeat(n, 1, 1).contiguous()


class _Slot:
    """The persistent buffers of one call site: per plane a workspace (zeroed once: the arrival counters at its head reset
    themselves), per matrix of the call a G of 12 doubles followed by their 12 float32 roundings.  `generation` counts the
    forwards: a backward that finds another one than its own would write its G over a later call's."""
    _cache = {}

    def __init__(self):
        self.ws, self.G, self.generation = {}, {}, 0

    @classmethod
    def get(cls, dev, slot):
        if isinstance(slot, _Slot):
            return slot
        key = (_dev(dev), slot)
        if key not in cls._cache:
            cls._cache[key] = _Slot()
        return cls._cache[key]

    def workspace(self, dev, k, W, H):
        key = (_dev(dev), k, W, H)
        if key not in self.ws:
            n = _C().exposure_workspace_bytes(W, H)
            if not n:
                raise ValueError(f"exposure: {W}x{H}: 1 <= W, H, W H <= 2^24")
            self.ws[key] = torch.zeros(n, dtype=torch.uint8, device=dev)
        return self.ws[key]

    def grad(self, dev, group=0):
        key = (_dev(dev), group)
        if key not in self.G:
            self.G[key] = torch.zeros(18, dtype=torch.float64, device=dev)
        return self.G[key]


def _g64(G):
    return G[:12]


def _g32(G):
    return G[12:].view(torch.float32)[:12].view(3, 4)


def _check_image(x, name="image"):
    if not x.is_cuda:
        raise _lib.B3gsError(f"apply_exposure needs device tensors (no CPU fallback): {name} is on {x.device}")
    if x.dim() != 3 or x.shape[0] != 3 or x.dtype != torch.float32:
        raise ValueError(f"apply_exposure: {name} is a float32 [3,H,W] image, not {x.dtype} {tuple(x.shape)}")


class _ExposureApply(torch.autograd.Function):
    """inputs (image_0 .. image_{n-1}, matrix_0 .. matrix_{g-1}) -> the n transformed images; cfg: groups (per plane the index
    of its matrix), rows (per matrix None or the int32 word on the device that names the row of a table), slot."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        n = len(cfg["groups"])
        images = [t.detach().contiguous() for t in tensors[:n]]
        mats = [t.detach().contiguous() for t in tensors[n:]]
        outs = [torch.empty_like(x) for x in images]
        _C().exposure_apply([(x, o, mats[g], cfg["rows"][g]) for x, o, g in zip(images, outs, cfg["groups"])])
        slot = _Slot.get(images[0].device, cfg["slot"])
        slot.generation += 1
        ctx.cfg, ctx.slot, ctx.generation, ctx.images, ctx.mats = cfg, slot, slot.generation, images, mats
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        cfg, slot, images, mats = ctx.cfg, ctx.slot, ctx.images, ctx.mats
        if slot.generation != ctx.generation:
            raise _lib.B3gsError("apply_exposure: the gradient buffers of this slot were taken by a later call before backward; "
                                 "give calls whose graphs are alive together different `slot`s")
        dev = images[0].device
        planes, g_in = [], []
        for k, (x, g) in enumerate(zip(images, cfg["groups"])):
            go = grads[k]
            go = torch.zeros_like(x) if go is None else go.contiguous()
            gi = torch.empty_like(x)
            g_in.append(gi)
            H, W = x.shape[-2:]
            planes.append((x, go, gi, mats[g], cfg["rows"][g], slot.grad(dev, g), slot.workspace(dev, k, W, H)))
        _C().exposure_backward(planes)
        g_mats = []
        for g, A in enumerate(mats):
            if not ctx.needs_input_grad[1 + len(images) + g]:
                g_mats.append(None)
            elif cfg["rows"][g] is None:
                g_mats.append(_g32(slot.grad(dev, g)).clone().view(A.shape))
            else:       # a table that asks for a gradient: its row, placed on the device (the trainers read G instead)
                full = torch.zeros((A.numel() // 12, 12), dtype=torch.float32, device=dev)
                row = cfg["rows"][g].to(torch.int64).clamp(0, full.shape[0] - 1)
                g_mats.append(full.index_copy_(0, row, _g32(slot.grad(dev, g)).reshape(1, 12)).view(A.shape))
        return (None, *[gi if ctx.needs_input_grad[1 + k] else None for k, gi in enumerate(g_in)], *g_mats)


def apply_exposure_batch(images: Sequence[torch.Tensor], matrices: Sequence[torch.Tensor], rows: Optional[Sequence] = None, *, slot=0):
    """images: up to 8 float32 [3,H,W] device tensors of any sizes; matrices: per image a float32 [3,4], or (with rows[k] an
    int32 word on the device) a table [V,3,4] whose row the kernels read on the device.  Images that are given the SAME matrix
    object (and the same row word) share it: backward forms ONE gradient for it, the planes added in fp64 in plane order.
    -> the transformed images.  The gradient of a [3,4] matrix is a float32 [3,4]; `exposure_grad(device, slot, group)`
    holds the 12 doubles behind it (group: the index of the matrix among the distinct ones, in order of first use)."""
    if not 1 <= len(images) <= MAX_PLANES:
        raise ValueError("apply_exposure_batch: 1 .. 8 images per call")
    rows = [None] * len(images) if rows is None else list(rows)
    if len(matrices) != len(images) or len(rows) != len(images):
        raise ValueError("apply_exposure_batch: one matrix (and one row word or None) per image")
    groups, mats, words, seen = [], [], [], {}
    for k, (x, A, r) in enumerate(zip(images, matrices, rows)):
        _check_image(x, f"image {k}")
        if A.dtype != torch.float32 or A.device != x.device or (r is None and tuple(A.shape) != (3, 4)) or \
                (r is not None and (A.dim() != 3 or tuple(A.shape[1:]) != (3, 4))):
            raise ValueError("apply_exposure: A is a float32 [3,4] matrix (or, with a row word, a [V,3,4] table) on the image's device")
        key = (id(A), id(r))
        if key not in seen:
            seen[key] = len(mats)
            mats.append(A)
            words.append(r)
        groups.append(seen[key])
    out = _ExposureApply.apply(dict(groups=groups, rows=words, slot=slot), *images, *mats)
    return list(out)


def apply_exposure(image: torch.Tensor, A: torch.Tensor, *, row=None, slot=0) -> torch.Tensor:
    """One image of apply_exposure_batch."""
    return apply_exposure_batch([image], [A], [row], slot=slot)[0]


def exposure_grad(device, slot=0, group=0) -> torch.Tensor:
    """The 12 doubles G[c][k] the last backward of `slot` left for matrix `group` (a view of the slot's buffer)."""
    return _g64(_Slot.get(device, slot).grad(device, group)).view(3, 4)


_fit_slot = _Slot()


def fit_exposure(renders: Sequence[torch.Tensor], gts: Sequence[torch.Tensor], masks: Optional[Sequence] = None, *,
                 return_sums: bool = False):
    """Per view the A [3,4] that minimises |A (render, 1) - gt|^2 over the pixels whose mask is non-zero (None: all), by the
    4x4 normal equations in fp64, and a flag (int32 [1] on the device): 1 when fewer than 16 pixels were used or the system is
    singular to 2^-40 of its trace -- A is then the identity.  No host read.  -> [(A, flag)] or [(A, flag, sums float64 [23])]."""
    masks = [None] * len(renders) if masks is None else list(masks)
    if len(gts) != len(renders) or len(masks) != len(renders):
        raise ValueError("fit_exposure: one ground truth (and one mask or None) per render")
    out = []
    for k0 in range(0, len(renders), MAX_PLANES):
        planes = []
        for k in range(k0, min(k0 + MAX_PLANES, len(renders))):
            r, g, m = renders[k], gts[k], masks[k]
            _check_image(r, "render")
            _check_image(g, "gt")
            if g.shape != r.shape:
                raise ValueError("fit_exposure: a render and its ground truth have one size")
            dev, (H, W) = r.device, r.shape[-2:]
            if m is not None:
                m = (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).contiguous()
                if m.numel() != H * W:
                    raise ValueError("fit_exposure: a mask is one [H,W] plane of its render's size")
            A = torch.empty((3, 4), dtype=torch.float32, device=dev)
            sums = torch.empty(23, dtype=torch.float64, device=dev)
            flag = torch.empty(1, dtype=torch.int32, device=dev)
            planes.append((r.detach().contiguous(), g.detach().contiguous(), m, A, sums, flag, _fit_slot.workspace(dev, k - k0, W, H)))
            out.append((A, flag, sums) if return_sums else (A, flag))
        _C().exposure_fit(planes)
    return out


# ---- exposure.json: {image_name: 3x4}, upstream's layout ----------------------------------------------------------------------
def write_matrices(path: str, matrices: dict) -> None:
    with open(path, "w") as f:
        json.dump({str(k): [[float(x) for x in row] for row in (v.tolist() if hasattr(v, "tolist") else v)] for k, v in matrices.items()},
                  f, indent=2)


def read_matrices(path: str) -> dict:
    with open(path) as f:
        return {k: torch.tensor(v, dtype=torch.float32).reshape(3, 4) for k, v in json.load(f).items()}


class ExposureTerm:
    """The exposure term as the trainers share it: one 3x4 matrix per training view (identity at the start), Adam moments,
    per-row step counts and running beta products, and the row word and learning rate the kernels read -- all in static
    device memory, so a captured graph keeps them and a replay follows an upload.  Only the row of the view an iteration drew
    moves (csrc/exposure.hip: exposure_adam_kernel); rows of views not drawn do not drift on their momentum, which is a
    deliberate difference from upstream's dense Adam.  The learning rate follows the log-linear schedule of
    xyz_scheduler_args from lr_init to lr_final over `iterations` (upstream's exposure_lr_init / _final)."""

    def __init__(self, names: Sequence, *, device="cuda", lr_init=0.01, lr_final=0.001, iterations=30_000, from_iter=0,
                 betas=(0.9, 0.999), eps=1e-8):
        self.names = [str(n) for n in names]
        if not self.names:
            raise ValueError("ExposureTerm: at least one view")
        if not (lr_init > 0.0 and lr_final > 0.0):
            raise ValueError("exposure_lr_init and exposure_lr_final are > 0")
        self.lr_init, self.lr_final, self.iterations, self.from_iter = float(lr_init), float(lr_final), int(iterations), int(from_iter)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        dev = self.device = _dev(device)
        V = len(self.names)
        self.table = identity(V, dev)
        self.exp_avg = torch.zeros((V, 3, 4), dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros((V, 3, 4), dtype=torch.float32, device=dev)
        self.steps = torch.zeros(V, dtype=torch.int32, device=dev)
        self.prods = torch.ones((V, 2), dtype=torch.float64, device=dev)
        self.block = torch.zeros(2, dtype=torch.float32, device=dev)        # [the row word | the learning rate]
        self.row, self.lr_dev = self.block[:1].view(torch.int32), self.block[1:]
        self._ring = None
        self._view, self._lr = 0, self.lr(0)
        self.slot = _Slot()

    enabled = True

    def active(self, it: int) -> bool:
        return it >= self.from_iter

    def lr(self, it: int) -> float:
        from .loss import expon_lr
        return expon_lr(it, self.lr_init, self.lr_final, max_steps=self.iterations)

    def state(self):
        """the tensors an optimiser step moves (GraphTrainer snapshots them around a capture's warm-up)"""
        return [self.table, self.exp_avg, self.exp_avg_sq, self.steps, self.prods]

    def stage(self, view_index: Optional[int] = None, it: Optional[int] = None) -> None:
        """The row word and / or the learning rate of `it` into device memory: one asynchronous copy from a pinned row."""
        if view_index is not None:
            if not 0 <= int(view_index) < len(self.names):
                raise IndexError(f"ExposureTerm: view {view_index} of {len(self.names)}")
            self._view = int(view_index)
        if it is not None:
            self._lr = self.lr(it)
        if self.device.type != "cuda":
            self.row[0], self.lr_dev[0] = self._view, self._lr
            return
        if self._ring is None:
            from .camera import _PinnedRing
            self._ring = _PinnedRing(64, 2)
        k, host = self._ring.take()
        host.view(torch.int32)[0] = self._view
        host[1] = self._lr
        self.block.copy_(host, non_blocking=True)
        self._ring.uploaded(k, self.device)

    def apply(self, view_index: Optional[int], *images):
        """The images through the row of `view_index` (None: the row staged already), ONE launch and one backward launch for
        all of them; their gradient sums meet in one G in fp64.  -> the transformed images (one image: itself, not a list)."""
        if view_index is not None:
            self.stage(view_index)
        out = apply_exposure_batch(list(images), [self.table] * len(images), [self.row] * len(images), slot=self.slot)
        return out[0] if len(images) == 1 else out

    def grad(self) -> torch.Tensor:
        return _g64(self.slot.grad(self.device, 0))

    def adam(self, skip_if_nonzero=None) -> None:
        """The Adam launch on the staged row with the G of the last backward; nothing but the launch (capturable)."""
        _C().exposure_adam(self.table, self.exp_avg, self.exp_avg_sq, self.steps, self.prods, self.row, self.slot.grad(self.device, 0),
                           self.lr_dev, self.betas[0], self.betas[1], self.eps, skip_if_nonzero)

    def step(self, it: int, skip_if_nonzero=None) -> None:
        """The optimiser step of iteration `it` on the row the last apply() named."""
        self.stage(None, it)
        self.adam(skip_if_nonzero)

    def matrices(self) -> dict:
        """{image_name: 3x4 nested lists} (one host read)"""
        return {n: m for n, m in zip(self.names, self.table.detach().cpu().tolist())}

    def state_dict(self) -> dict:
        return dict(names=list(self.names), table=self.table.detach().cpu().clone(), exp_avg=self.exp_avg.cpu().clone(),
                    exp_avg_sq=self.exp_avg_sq.cpu().clone(), steps=self.steps.cpu().clone(), prods=self.prods.cpu().clone())

    def load_state_dict(self, sd: dict) -> None:
        """By image name: a view the state does not know keeps the identity."""
        at = {n: k for k, n in enumerate(sd["names"])}
        for k, n in enumerate(self.names):
            j = at.get(n)
            if j is None:
                continue
            for mine, key in ((self.table, "table"), (self.exp_avg, "exp_avg"), (self.exp_avg_sq, "exp_avg_sq"), (self.steps, "steps"),
                              (self.prods, "prods")):
                mine[k] = sd[key][j].to(mine.device)
