"""Ground truth of dataset images, prepared on the device from the uint8 source at its own size.

    utils/camera_utils.py:22-45   loadCam: the output size, PILtoTorch, alpha split, white-background composite
    utils/general_utils.py:22-28  PILtoTorch: PIL.Image.resize(size) (BICUBIC, 8 bits per channel), / 255
    scene/cameras.py:40-47        clamp(0, 1), multiply by the alpha mask
    train.py:110-120              the DTU background mask (49 launches per ITERATION there; here once per camera)

The reference resizes every image on one CPU thread before the first iteration (LLFF: 4032x3024 -> 504x378, 36 MB per
image, train and test views).  Here the host only decodes: the uint8 image goes to the device as it is (pinned staging,
asynchronous copy) and b3gs_prepare_gt_batch (csrc/gt_prep.hip) produces `original_image`, `gt_alpha_mask` and `bg_mask` for up
to 8 views per call -- the same bits: the resize is integer arithmetic on coefficient tables this module builds in float64
exactly as Pillow does (resize_table), everything after it is one correctly rounded float32 operation per statement.

What stays on the host: output_size (loadCam's rule) and the tables (a few KB per distinct (in, out), cached).
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_BATCH = 8            # views per b3gs_prepare_gt_batch (B3GS_MAX_GT_VIEWS)
PRECISION_BITS = 22      # fractional bits of a tap (Pillow: 32 - 8 - 2)
DTU_THRESHOLD = 30 / 255
DTU_THRESHOLD_SCAN110 = 15 / 255


def dtu_threshold_for(source_path: str) -> float:
    """train.py:113-116: 30/255, or 15/255 when 'scan110' is in the source path."""
    return DTU_THRESHOLD_SCAN110 if "scan110" in source_path else DTU_THRESHOLD


def scaled_size(orig_w, orig_h, resolution, cap: int) -> Tuple[int, int]:
    """The size rule loadCam and loadRenderCam share (utils/camera_utils.py:22-41, 69-88) at resolution_scale 1.0: they
    differ in the width above which resolution -1 scales down (`cap`: 1600 / 6400)."""
    if resolution in [1, 2, 4, 8]:
        return round(orig_w / (1.0 * resolution)), round(orig_h / (1.0 * resolution))
    if resolution == -1:
        down = orig_w / cap if orig_w > cap else 1
    else:
        down = orig_w / resolution
    scale = float(down) * 1.0
    return int(orig_w / scale), int(orig_h / scale)


def output_size(orig_w: int, orig_h: int, resolution=-1) -> Tuple[int, int]:
    """(width, height) loadCam resizes a orig_w x orig_h image to: resolution 1 / 2 / 4 / 8 divides and rounds, -1 caps the
    width at 1600, anything else is the target width."""
    return scaled_size(orig_w, orig_h, resolution, 1600)


def _cubic(x: np.ndarray) -> np.ndarray:
    """Keys' cubic, a = -0.5 (Pillow's BICUBIC), float64."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


@lru_cache(maxsize=256)
def resize_table(in_size: int, out_size: int) -> np.ndarray:
    """int32 [2 + ksize, out_size] of one axis of PIL.Image.resize (BICUBIC): row 0 the first source index of every output
    index, row 1 its tap count, rows 2.. the taps with 22 fractional bits (0 beyond the count).  Float64 throughout, the
    taps of one output index summed in index order, as Pillow's coefficient pass does."""
    if in_size < 1 or out_size < 1:
        raise ValueError("sizes are at least 1")
    scale = in_size / out_size
    fscale = scale if scale >= 1.0 else 1.0
    support = 2.0 * fscale
    ksize = int(np.ceil(support)) * 2 + 1
    inv = 1.0 / fscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    n = hi - lo
    j = np.arange(ksize, dtype=np.int64)[None, :]
    k = _cubic(((j + lo[:, None]) - center[:, None] + 0.5) * inv)
    k = np.where(j < n[:, None], k, 0.0)
    total = np.cumsum(k, axis=1)[:, -1:]                     # in index order (trailing zeros change nothing)
    k = np.where(total != 0.0, k / np.where(total != 0.0, total, 1.0), k)
    q = np.where(k < 0, np.trunc(-0.5 + k * (1 << PRECISION_BITS)), np.trunc(0.5 + k * (1 << PRECISION_BITS))).astype(np.int64)
    # int32 accumulators on the device: 2^21 + 255 * sum|K| must stay below 2^31
    assert (1 << (PRECISION_BITS - 1)) + 255 * int(np.abs(q).sum(axis=1).max()) < (1 << 31), (in_size, out_size)
    tab = np.empty((2 + ksize, out_size), dtype=np.int32)
    tab[0], tab[1] = lo, n
    tab[2:] = q.T
    tab.setflags(write=False)
    return tab


_device_tables: Dict[tuple, torch.Tensor] = {}


def device_table(in_size: int, out_size: int, device) -> Optional[torch.Tensor]:
    """The table of one axis on the device (None when the size does not change: the pass is skipped)."""
    if in_size == out_size:
        return None
    key = (int(in_size), int(out_size), str(torch.device(device)))
    t = _device_tables.get(key)
    if t is None:
        if len(_device_tables) >= 256:
            _device_tables.clear()
        t = _device_tables[key] = torch.from_numpy(resize_table(int(in_size), int(out_size)).copy()).to(device)
    return t


def _as_source(img) -> torch.Tensor:
    """A contiguous uint8 [Hs, Ws, C] host or device tensor of a numpy array / tensor ([Hs, Ws] counts as one channel)."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError("a source image is uint8 [H, W, C] or [H, W]")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.shape[2] not in (1, 3, 4):
        raise ValueError(f"1, 3 or 4 channels, not {t.shape[2]} (expand gray + alpha to RGBA first)")
    return t.contiguous()


def prepare_ground_truth(sources: Sequence, size: Tuple[int, int], *, white_background: bool = False,
                         dtu_threshold: Optional[float] = None, device="cuda") -> List[tuple]:
    """-> per source (original_image [3,H,W] or [1,H,W], gt_alpha_mask [1,H,W] | None, bg_mask [1,H,W] | None), float32 on
    `device`, for size = (W, H).  sources: uint8 [Hs, Ws, C] images (numpy / CPU tensors are staged in pinned memory and
    uploaded asynchronously; device tensors are taken as they are), C in {1, 3, 4}; their sizes may differ.  `sources` may be
    an iterator: at most 8 decoded images are alive at a time.  gt_alpha_mask comes with 4 channels, bg_mask with a
    `dtu_threshold` (dtu_threshold_for).  `original_image` is final: clamped and multiplied by the alpha mask already
    (camera.Camera(..., prepared=True))."""
    from . import _C
    W, H = int(size[0]), int(size[1])
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("ground truth is prepared on the HIP device: there is no CPU path")
    thr = float(dtu_threshold) if dtu_threshold else 0.0
    out: List[tuple] = []
    batch: List[torch.Tensor] = []

    def flush():
        if not batch:
            return
        tx = [device_table(s.shape[1], W, dev) for s in batch]
        ty = [device_table(s.shape[0], H, dev) for s in batch]
        out.extend(_C.prepare_gt(batch, tx, ty, W, H, bool(white_background), thr))
        batch.clear()               # (the uint8 sources go back to the caching allocator: stream-ordered, safe to reuse)

    for img in sources:
        t = _as_source(img)
        if t.device.type != "cuda":
            t = t.pin_memory().to(dev, non_blocking=True)
        elif t.device != dev:
            t = t.to(dev)
        batch.append(t)
        if len(batch) == MAX_BATCH:
            flush()
    flush()
    return out
