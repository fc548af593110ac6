"""Yardstick of the depth-derived normals, their loss and the normal-prior resize (csrc/normalprior.hip; the rules are stated in
include/b3gs_raster.h).  numpy float64 in the kernel's own operation and summation order -- every output is meant to be equal bit
for bit -- plus a torch restatement of the DEFINITION (any dtype, differentiable in depth and alpha) that the yardstick's
analytic gradients are checked against and the timing tool runs.

`mutant`: "cross_order" takes cross(tx, ty) in place of cross(ty, tx), "gather_sign" flips the sign of the x + 1 term of the
gather; the tests must catch both."""
from __future__ import annotations

import numpy as np

from depth_prior_ref import fma32, fold, tree256      # the TREE and the FOLD are those of the depth-prior sums

F64, F32 = np.float64, np.float32
PARTS = ("loss", "cos", "l1", "n_valid", "mean_dot", "reserved")


def _cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def rays(W, H, tanfovx, tanfovy):
    rx = ((2.0 * (np.arange(W, dtype=F64) + 0.5)) / F64(W) - 1.0) * F64(tanfovx)
    ry = ((2.0 * (np.arange(H, dtype=F64) + 0.5)) / F64(H) - 1.0) * F64(tanfovy)
    return rx, ry


def _shift(a, dy, dx):
    """out[.., y, x] = a[.., y + dy, x + dx], 0 outside"""
    H, W = a.shape[-2:]
    out = np.zeros_like(a)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def _planes(depth, alpha, exact_inputs):
    if exact_inputs:                     # float64 inputs as they are (the closed-form test: no float32 rounding of the planes)
        d, a = np.asarray(depth, F64), np.asarray(alpha, F64)
    else:
        d, a = np.asarray(depth, F32).astype(F64), np.asarray(alpha, F32).astype(F64)
    H, W = d.shape[-2:]
    return d.reshape(H, W), a.reshape(H, W)


def forward(depth, alpha, mask, tanfovx, tanfovy, alpha_min, *, mutant=None, exact_inputs=False):
    """-> dict(n [3,H,W] float64, valid [H,W] bool, usable [H,W] bool, z, tx, ty, cc, s, rx, ry)"""
    d, a = _planes(depth, alpha, exact_inputs)
    H, W = d.shape
    usable = (a >= F64(alpha_min)) if exact_inputs else (a.astype(F32) >= F32(alpha_min))
    rx, ry = rays(W, H, tanfovx, tanfovy)
    with np.errstate(all="ignore"):
        z = d / a
        p = np.stack([z * rx[None, :], z * ry[:, None], z])
        tx, ty = np.zeros_like(p), np.zeros_like(p)
        if W >= 3:
            tx[:, :, 1:-1] = p[:, :, 2:] - p[:, :, :-2]
        if H >= 3:
            ty[:, 1:-1, :] = p[:, 2:, :] - p[:, :-2, :]
        c = _cross(tx, ty) if mutant == "cross_order" else _cross(ty, tx)
        cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
        interior = np.zeros((H, W), bool)
        interior[1:-1, 1:-1] = True
        u = usable.astype(np.uint8)
        five = usable & (_shift(u, 0, -1) != 0) & (_shift(u, 0, 1) != 0) & (_shift(u, -1, 0) != 0) & (_shift(u, 1, 0) != 0)
        valid = interior & five & (cc > 0.0) & np.isfinite(cc)
        if mask is not None:
            valid &= np.asarray(mask).reshape(H, W) != 0
        s = np.sqrt(np.where(valid, cc, 1.0))
        n = np.where(valid, c / s, 0.0)
    zero = np.zeros_like(tx)
    return dict(n=n, valid=valid, usable=usable, z=z, a=a, tx=np.where(valid, tx, zero), ty=np.where(valid, ty, zero), cc=cc, s=s,
                rx=rx, ry=ry, raw_tx=tx, raw_ty=ty)


def depth_normals(depth, alpha, tanfovx, tanfovy, alpha_min, mask=None):
    """-> (normals float32 [3,H,W], valid uint8 [H,W])"""
    f = forward(depth, alpha, mask, tanfovx, tanfovy, alpha_min)
    return f["n"].astype(F32), f["valid"].astype(np.uint8)


def loss(depth, alpha, target, mask, tanfovx, tanfovy, *, w_cos=1.0, w_l1=0.0, alpha_min=0.5, mutant=None, exact_inputs=False):
    """-> dict(parts [6] float64, block_sums [nb, 3], normals float32 [3,H,W], valid uint8 [H,W], g_depth, g_alpha float32 [H,W];
    with exact_inputs the float64 gradients g_depth64 / g_alpha64 are what a test reads)"""
    f = forward(depth, alpha, mask, tanfovx, tanfovy, alpha_min, mutant=mutant, exact_inputs=exact_inputs)
    n, valid, s, tx, ty = f["n"], f["valid"], f["s"], f["tx"], f["ty"]
    H, W = valid.shape
    npix = H * W
    t = np.asarray(target, F64 if exact_inputs else F32).astype(F64).reshape(3, H, W)
    w_cos, w_l1 = F64(w_cos), F64(w_l1)
    with np.errstate(all="ignore"):
        dot = (n[0] * t[0] + n[1] * t[1]) + n[2] * t[2]
        df = n - t
        q = np.stack([np.ones_like(dot), 1.0 - dot, (np.abs(df[0]) + np.abs(df[1])) + np.abs(df[2])], axis=-1)
        q = np.where(valid[..., None], q, 0.0).reshape(npix, 3)
        nb = -(-npix // 256)
        pad = np.zeros((nb * 256, 3), F64)
        pad[:npix] = q
        block_sums = tree256(pad.reshape(nb, 256, 3))
        S = fold(block_sums)
        N = S[0]
        parts = np.zeros(6, F64)
        inv = F64(0.0)
        if N > 0.0:
            ct, lt = S[1] / N, S[2] / N
            parts[:] = [w_cos * ct + w_l1 * lt, ct, lt, N, 1.0 - ct, 0.0]
            inv = 1.0 / N
        h = w_l1 * np.sign(df) - w_cos * t
        d = (n[0] * h[0] + n[1] * h[1]) + n[2] * h[2]
        e = (h - n * d) / s
        zero = np.zeros_like(e)
        g_ty = np.where(valid, _cross(tx, e), zero)
        g_tx = np.where(valid, _cross(e, ty), zero)
        A, B, C, D = _shift(g_tx, 0, -1), _shift(g_tx, 0, 1), _shift(g_ty, -1, 0), _shift(g_ty, 1, 0)
        gp = ((A + B) + C) - D if mutant == "gather_sign" else ((A - B) + C) - D
        gz = ((gp[0] * f["rx"][None, :] + gp[1] * f["ry"][:, None]) + gp[2]) * inv
        gd = np.where(f["usable"], gz / f["a"], 0.0)
        ga = np.where(f["usable"], (0.0 - gz * f["z"]) / f["a"], 0.0)
    return dict(parts=parts, block_sums=block_sums, normals=n.astype(F32), valid=valid.astype(np.uint8), g_depth=gd.astype(F32),
                g_alpha=ga.astype(F32), g_depth64=gd, g_alpha64=ga, n64=n, forward=f)


def workspace_views(ws64, W, H):
    """-> (block sums [nb, 3], 1 / N, the counter word) out of the workspace of b3gs_normal_prior_loss_batch viewed as float64"""
    nb = -(-(W * H) // 256)
    return ws64[32:32 + 3 * nb].reshape(nb, 3), ws64[8], ws64[:1].view(np.uint64)[0]


# ---- resize ----------------------------------------------------------------------------------------------------------------
def resize(src, W, H, src_mask=None):
    """src [3, Hsrc, Wsrc] -> (n float32 [3, H, W], M uint8 [H, W])"""
    src = np.asarray(src, F32)
    _, Hs, Ws = src.shape
    good_src = np.isfinite(src).all(axis=0)
    if src_mask is not None:
        good_src &= np.asarray(src_mask) != 0
    xs, ys = np.meshgrid(np.arange(W, dtype=F32), np.arange(H, dtype=F32))
    sx = fma32(xs + F32(0.5), F32(Ws) / F32(W), F32(-0.5))
    sy = fma32(ys + F32(0.5), F32(Hs) / F32(H), F32(-0.5))
    bx, by = np.floor(sx), np.floor(sy)
    fx, fy = sx - bx, sy - by
    xa, xb = np.clip(bx.astype(np.int64), 0, Ws - 1), np.clip(bx.astype(np.int64) + 1, 0, Ws - 1)
    ya, yb = np.clip(by.astype(np.int64), 0, Hs - 1), np.clip(by.astype(np.int64) + 1, 0, Hs - 1)
    gx, gy = F32(1.0) - fx, F32(1.0) - fy
    w = [gx * gy, fx * gy, gx * fy, fx * fy]
    at = [(ya, xa), (ya, xb), (yb, xa), (yb, xb)]
    ok = np.ones((H, W), bool)
    for wk, (yy, xx) in zip(w, at):
        ok &= (wk == 0) | good_src[yy, xx]
    val = []
    for c in range(3):
        p = [np.where((wk != 0) & good_src[yy, xx], src[c][yy, xx], F32(0.0)).astype(F32) for wk, (yy, xx) in zip(w, at)]
        val.append(fma32(w[3], p[3], fma32(w[2], p[2], fma32(w[1], p[1], w[0] * p[0]))).astype(F64))
    l = (val[0] * val[0] + val[1] * val[1]) + val[2] * val[2]
    ok &= l >= 0.25
    with np.errstate(all="ignore"):
        s = np.sqrt(l)
        out = np.stack([np.where(ok, v / s, 0.0) for v in val]).astype(F32)
    return out, ok.astype(np.uint8)


# ---- the definition, in torch (any dtype; autograd gives the gradients) -----------------------------------------------------
def torch_loss(depth, alpha, target, valid, tanfovx, tanfovy, *, w_cos=1.0, w_l1=0.0):
    """depth, alpha [1,H,W], target [3,H,W] of one dtype, valid [H,W] bool (the yardstick's valid set, or any set of interior
    pixels) -> (L, mean n.t).  Written from the definition: a pixel grid, torch.linalg.cross, a masked mean."""
    import torch
    H, W = depth.shape[-2:]
    dt, dev = depth.dtype, depth.device
    gx = (2 * (torch.arange(W, dtype=dt, device=dev) + 0.5) / W - 1) * tanfovx
    gy = (2 * (torch.arange(H, dtype=dt, device=dev) + 0.5) / H - 1) * tanfovy
    one = torch.ones((), dtype=dt, device=dev)
    z = depth[0] / torch.where(alpha[0] > 0, alpha[0], one)
    pts = torch.stack([z * gx[None, :], z * gy[:, None], z], dim=-1)                       # [H, W, 3]
    du = pts[1:-1, 2:] - pts[1:-1, :-2]
    dv = pts[2:, 1:-1] - pts[:-2, 1:-1]
    sel = valid[1:-1, 1:-1]
    c = torch.linalg.cross(dv, du, dim=-1)[sel]
    n = c / c.norm(dim=-1, keepdim=True)
    t = target.permute(1, 2, 0)[1:-1, 1:-1][sel]
    count = sel.sum().clamp(min=1).to(dt)              # (no host read)
    dots = (n * t).sum(-1)
    total = w_cos * (1 - dots).sum() / count + w_l1 * (n - t).abs().sum() / count
    return total, dots.sum() / count


# ---- the inputs the CPU and the device tests share --------------------------------------------------------------------------
# name -> (W, H): one interior pixel; none; block seams, 16-wide tile seams and holes at the border; 305 blocks
CASES = {"3x3": (3, 3), "2x5": (2, 5), "37x29": (37, 29), "300x260": (300, 260)}
ALPHA_MIN, TANFOV = 0.5, (0.62, 0.47)


def make_case(W, H, seed=0):
    """-> depth, alpha float32 [1,H,W], target float32 [3,H,W], mask uint8 [1,H,W]: a smooth surface seen through alpha in
    [0.6, 1] (the render is depth = z alpha), alpha holes (single pixels, a block on the border, two blocks that touch), masked
    target pixels, targets that are the true normals perturbed and renormalised."""
    rng = np.random.default_rng(seed + 17 * W + H)
    ys, xs = np.mgrid[0:H, 0:W].astype(F64)
    u, v = xs / max(W - 1, 1), ys / max(H - 1, 1)
    z = 2.0 + 0.5 * u + 0.3 * v + 0.2 * np.sin(5.0 * u) * np.cos(4.0 * v)
    alpha = (0.6 + 0.4 * rng.random((H, W))).astype(F32)
    mask = np.ones((H, W), np.uint8)
    if W * H > 9:
        alpha[rng.random((H, W)) < 0.01] = 0.25
        mask[rng.random((H, W)) < 0.03] = 0
    if W >= 30 and H >= 20:
        alpha[0:3, 5:8] = 0.25                     # touches the top border
        alpha[H // 2:H // 2 + 2, W - 2:W] = 0.0    # touches the right border: z = depth / 0
        alpha[10:12, 14:17] = 0.25                 # two blocks that touch each other, across the x = 16 seam
        alpha[12:14, 16:19] = 0.25
    depth = (z * alpha.astype(F64)).astype(F32)
    true = forward(depth, alpha, None, *TANFOV, ALPHA_MIN)["n"]
    t = np.where(true.any(axis=0), true, np.array([0.0, 0.0, -1.0])[:, None, None]) + 0.2 * rng.standard_normal((3, H, W))
    t = (t / np.sqrt((t * t).sum(axis=0))).astype(F32)
    return depth[None], alpha[None], t, mask[None]


def conditions(W, H, case):
    """-> (N, interior pixels, number of pixels with 0 < c.c < 1e-6 |tx|^2 |ty|^2 among the five-usable interior ones)"""
    depth, alpha, target, mask = case
    f = forward(depth, alpha, mask, *TANFOV, ALPHA_MIN)
    tx, ty = f["raw_tx"], f["raw_ty"]
    with np.errstate(all="ignore"):
        bound = 1e-6 * (tx * tx).sum(axis=0) * (ty * ty).sum(axis=0)
        thin = f["valid"] & (f["cc"] > 0) & (f["cc"] < bound)
    return int(f["valid"].sum()), max(W - 2, 0) * max(H - 2, 0), int(thin.sum())
