"""Test helper: PIL.Image.resize(size) with its default filter (BICUBIC) on 8-bit images, restated in numpy, and the float
statements that follow it in the reference's loader, on CPU torch tensors.  Independent of binocular3dgs_amd.ground_truth
(scalar Python coefficients here, vectorised ones there): tests compare the two with each other, with Pillow where it is
installed, and with the recorded reference output (tests/golden/scene_prep.npz).  Not part of the package."""
import math

import numpy as np
import torch

BITS = 22


def keys_cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def coefficients(n_in, n_out):
    """-> [(first source index, int64 taps)] per output index"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    inv = 1.0 / fs
    rows = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        k = [keys_cubic((j + lo - center + 0.5) * inv) for j in range(hi - lo)]
        total = 0.0
        for v in k:
            total += v
        if total != 0.0:
            k = [v / total for v in k]
        q = [int(-0.5 + v * (1 << BITS)) if v < 0 else int(0.5 + v * (1 << BITS)) for v in k]
        rows.append((lo, np.array(q, dtype=np.int64)))
    return rows


def table(n_in, n_out):
    """The layout of ground_truth.resize_table: int32 [2 + ksize, n_out]"""
    rows = coefficients(n_in, n_out)
    ksize = int(math.ceil(2.0 * max(n_in / n_out, 1.0))) * 2 + 1
    t = np.zeros((2 + ksize, n_out), dtype=np.int32)
    for i, (lo, q) in enumerate(rows):
        t[0, i], t[1, i] = lo, len(q)
        t[2:2 + len(q), i] = q
    return t


def _pass_axis1(img, n_out):
    """img uint8 [A, n_in, C] -> [A, n_out, C]"""
    A, n_in, C = img.shape
    if n_out == n_in:
        return img
    out = np.empty((A, n_out, C), dtype=np.uint8)
    wide = img.astype(np.int64)
    for i, (lo, q) in enumerate(coefficients(n_in, n_out)):
        acc = (wide[:, lo:lo + len(q), :] * q[None, :, None]).sum(axis=1) + (1 << (BITS - 1))
        out[:, i, :] = np.clip(acc >> BITS, 0, 255)
    return out


def premultiply(rgba):
    a = rgba[..., 3:4].astype(np.int64)
    t = rgba[..., :3].astype(np.int64) * a + 128
    return np.concatenate([((t >> 8) + t) >> 8, a], axis=-1).astype(np.uint8)


def unpremultiply(rgba):
    a = rgba[..., 3:4].astype(np.int64)
    c = rgba[..., :3].astype(np.int64)
    d = np.minimum((255 * c) // np.where(a == 0, 1, a), 255)
    return np.concatenate([np.where((a == 0) | (a == 255), c, d), a], axis=-1).astype(np.uint8)


def resize(img, size):
    """img uint8 [H, W] / [H, W, C], size (w, h) -> the bytes PIL.Image.fromarray(img).resize(size) holds"""
    w, h = size
    flat = img.ndim == 2
    x = img[..., None] if flat else img
    if (x.shape[1], x.shape[0]) != (w, h):
        alpha = x.shape[2] == 4
        if alpha:
            x = premultiply(x)
        x = _pass_axis1(x, w)                                              # horizontal first, stored as uint8
        x = _pass_axis1(x.transpose(1, 0, 2), h).transpose(1, 0, 2)
        if alpha:
            x = unpremultiply(x)
    x = np.ascontiguousarray(x)
    return x[..., 0] if flat else x


def float_statements(resized, white_background=False, dtu_threshold=None):
    """The loader's statements after the resize, on the CPU: -> (original_image, gt_alpha_mask | None, bg_mask | None)"""
    t = torch.from_numpy(np.ascontiguousarray(resized)) / 255.0
    t = t.permute(2, 0, 1) if t.dim() == 3 else t.unsqueeze(-1).permute(2, 0, 1)
    image, mask = t[:3], None
    if t.shape[0] == 4:
        mask = t[3:4]
        if white_background:
            image = image * mask + torch.tensor([1, 1, 1])[:, None, None] * (1 - mask)
    image = image.clamp(0.0, 1.0)
    if mask is not None:
        image = image * mask
    bg = None
    if dtu_threshold:
        dark = image.max(0, keepdim=True).values < dtu_threshold
        bg = dtu_rows(dark).float()
    return image.contiguous(), None if mask is None else mask.contiguous(), bg


def dtu_rows(dark):
    """bool [1, H, W] -> AND over rows max(0, y-49)..y, as a loop over rows"""
    out = torch.empty_like(dark)
    H = dark.shape[1]
    for y in range(H):
        out[:, y] = dark[:, max(0, y - 49):y + 1].all(dim=1)
    return out


def ground_truth(img, size, white_background=False, dtu_threshold=None):
    return float_statements(resize(img, size), white_background, dtu_threshold)
