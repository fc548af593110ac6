"""Yardstick of the depth-prior loss and the prior resize (csrc/depthprior.hip; the rules are stated in include/b3gs_raster.h).
numpy float64 in the kernel's own summation order -- every output is meant to be equal bit for bit -- plus a torch restatement
of the DEFINITION (any dtype, differentiable) that the yardstick's gradient is checked against and the timing tool runs.

`mutant`: "origin" moves the patch grid's origin by one pixel, "drop_rho" drops the rho (x - mx) / cxx term of the gradient;
the tests must catch both."""
from __future__ import annotations

import numpy as np

F64, F32 = np.float64, np.float32
LANES = np.arange(64)


def _butterfly(v, axis):
    """xor butterfly 32, 16, .., 1 over an axis of 64: every lane ends with the same sum"""
    for d in (32, 16, 8, 4, 2, 1):
        v = v + np.take(v, LANES ^ d, axis=axis)
    return v


def tree256(v):
    """v [.., 256, k] -> [.., k]: butterfly per group of 64, then (g0 + g1) + (g2 + g3)"""
    v = v.reshape(v.shape[:-2] + (4, 64, v.shape[-1]))
    g = _butterfly(v, -2)[..., 0, :]
    return (g[..., 0, :] + g[..., 1, :]) + (g[..., 2, :] + g[..., 3, :])


def fold(parts):
    """parts [n, k] -> [k]: lane l adds rows l, l + 64, .. in order to +0, then the butterfly"""
    n, k = parts.shape
    rows = -(-max(n, 1) // 64)
    pad = np.zeros((rows * 64, k), F64)
    pad[:n] = parts
    acc = np.zeros((64, k), F64)
    for r in pad.reshape(rows, 64, k):
        acc = acc + r
    return _butterfly(acc, 0)[0]


def pixel_terms(depth, alpha, prior, mask, mode, alpha_min):
    """-> used [n] bool, x, y, t' [n] float64 (zero where not used)"""
    d = np.asarray(depth, F32).reshape(-1).astype(F64)
    used = (np.asarray(mask).reshape(-1) != 0) & (np.asarray(alpha, F32).reshape(-1) >= F32(alpha_min))
    with np.errstate(all="ignore"):
        if mode == "disparity":
            x = 1.0 / (d + 1e-5)
            t = 0.0 - x * x
        else:
            x, t = d, np.ones_like(d)
    y = np.asarray(prior, F32).reshape(-1).astype(F64)
    z = np.zeros_like(d)
    return used, np.where(used, x, z), np.where(used, y, z), np.where(used, t, z)


def derive(s, min_valid):
    """the six sums of a set -> dict(flag, mx, my, cxx, den, rho, term, cxy, cyy); a skipped set: all zero"""
    out = dict(flag=0.0, mx=0.0, my=0.0, cxx=0.0, den=0.0, rho=0.0, term=0.0, cxy=0.0, cyy=0.0)
    n = s[0]
    if not n >= float(min_valid):
        return out
    with np.errstate(all="ignore"):
        cxx = s[3] - (s[1] * s[1]) / n
        cyy = s[4] - (s[2] * s[2]) / n
        cxy = s[5] - (s[1] * s[2]) / n
        if not cxx > 0.0 or not cyy > 0.0:
            return out
        den = np.sqrt(cxx * cyy)
        rho = cxy / den
    out.update(flag=1.0, mx=s[1] / n, my=s[2] / n, cxx=cxx, den=den, rho=rho, term=1.0 - rho, cxy=cxy, cyy=cyy)
    return out


def _gradient(row, x, y, t, mutant):
    with np.errstate(all="ignore"):
        u = (y - row["my"]) / row["den"]
        w = (row["rho"] * (x - row["mx"])) / row["cxx"]
        if mutant == "drop_rho":
            w = np.zeros_like(w)
        return (0.0 - (u - w)) * t


def loss(depth, alpha, prior, mask, *, mode="depth", w_global=1.0, w_local=0.0, patch=0, min_valid=16, alpha_min=0.0,
         offset=(0, 0), mutant=None):
    """-> dict(parts [8] float64, grad [H, W] float32, image_sums [6], patch_sums [npatch, 6], patch_flags [npatch])"""
    depth = np.asarray(depth, F32)
    H, W = depth.shape[-2:]
    npix = H * W
    used, x, y, t = pixel_terms(depth, alpha, prior, mask, mode, alpha_min)
    q = np.stack([used.astype(F64), x, y, x * x, y * y, x * y], axis=1)
    nbg = -(-npix // 256)
    pad = np.zeros((nbg * 256, 6), F64)
    pad[:npix] = q
    image_sums = fold(tree256(pad.reshape(nbg, 256, 6)))
    head = derive(image_sums, min_valid)

    p = int(patch)
    w_local = float(w_local) if p else 0.0
    gx = (W + p - 1) // p + 1 if p else 0
    gy = (H + p - 1) // p + 1 if p else 0
    ox = min(max(int(offset[0]), 0), p - 1) if p else 0
    oy = min(max(int(offset[1]), 0), p - 1) if p else 0
    shift = 1 if mutant == "origin" else 0
    rows, psums = [], np.zeros((gx * gy, 6), F64)
    k = np.arange(p * p)
    steps = -(-(p * p) // 256) if p else 0
    for pid in range(gx * gy):
        px = (pid % gx) * p - ox + shift + k % p
        py = (pid // gx) * p - oy + shift + k // p
        inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        qk = np.zeros((steps * 256, 6), F64)
        qk[:p * p][inside] = q[py[inside] * W + px[inside]]
        v = np.zeros((256, 6), F64)
        for r in qk.reshape(steps, 256, 6):
            v = v + r
        psums[pid] = tree256(v)
        rows.append(derive(psums[pid], min_valid))
    flags = np.array([r["flag"] for r in rows], F64)
    if rows:
        tsum, count = fold(np.stack([np.array([r["term"] for r in rows], F64), flags], axis=1))
    else:
        tsum, count = 0.0, 0.0
    mean = tsum / count if count > 0.0 else 0.0
    a = off = 0.0
    if head["flag"]:
        a = head["cxy"] / head["cyy"]
        off = head["mx"] - a * head["my"]
    parts = np.array([w_global * head["term"] + w_local * mean, head["term"], mean, image_sums[0], count, head["rho"], a, off], F64)

    gg = _gradient(head, x, y, t, mutant) if head["flag"] else np.zeros(npix, F64)
    gp = np.zeros(npix, F64)
    if p and count > 0.0:
        ix, iy = np.arange(npix) % W, np.arange(npix) // W
        pid = ((iy + oy - shift) // p) * gx + (ix + ox - shift) // p
        for r_id in np.unique(pid[used]):
            if rows[r_id]["flag"]:
                sel = used & (pid == r_id)
                gp[sel] = _gradient(rows[r_id], x[sel], y[sel], t[sel], mutant)
    lg = w_global * gg
    lp = (w_local * gp) / count if count > 0.0 else np.zeros(npix, F64)
    grad = np.where(used, lg + lp, 0.0).astype(F32).reshape(H, W)
    return dict(parts=parts, grad=grad, image_sums=image_sums, patch_sums=psums, patch_flags=flags, grid=(gx, gy))


# ---- the workspace of b3gs_depth_prior_loss_batch as float64 words (csrc/depthprior.hip: HEAD, ROW) -------------------------
def workspace_views(ws64, W, H, patch):
    """-> image sums [6], patch sums [npatch, 6], patch flags [npatch] out of the workspace viewed as float64"""
    nbg = -(-(W * H) // 256)
    start = 32 + (6 * nbg + 31) // 32 * 32
    npatch = ((W + patch - 1) // patch + 1) * ((H + patch - 1) // patch + 1) if patch else 0
    rows = ws64[start:start + 16 * npatch].reshape(npatch, 16)
    return ws64[8:14], rows[:, :6], rows[:, 6]


# ---- resize ----------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """float32 fma(a, b, c) with ONE rounding: the product is exact in float64, the sum's error comes from TwoSum, and a
    float64 result that sits exactly between two float32 values is moved off the tie towards the exact value"""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b
    r = p + c
    bb = r - p
    err = (p - (r - bb)) + (c - bb)
    r32 = r.astype(F32)
    back = r32.astype(F64)
    other = np.nextafter(r32, np.where(r > back, np.inf, -np.inf).astype(F32)).astype(F64)
    tie = (r != back) & (r == (back + other) / 2.0) & (err != 0.0)
    r = np.where(tie, np.nextafter(r, np.where(err > 0.0, np.inf, -np.inf)), r)
    return r.astype(F32)


def resize(src, W, H, src_mask=None):
    """src [Hsrc, Wsrc] -> (P float32 [H, W], M uint8 [H, W])"""
    src = np.asarray(src, F32)
    Hs, Ws = src.shape
    with np.errstate(all="ignore"):
        valid = np.isfinite(src) & (src > 0)
    if src_mask is not None:
        valid &= np.asarray(src_mask) != 0
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
    p = []
    for wk, (yy, xx) in zip(w, at):
        live = wk != 0
        good = valid[yy, xx]
        ok &= ~live | good
        p.append(np.where(live & good, src[yy, xx], F32(0.0)).astype(F32))
    val = fma32(w[3], p[3], fma32(w[2], p[2], fma32(w[1], p[1], w[0] * p[0])))
    return np.where(ok, val, F32(0.0)).astype(F32), ok.astype(np.uint8)


# ---- the definition, in torch (any dtype; autograd gives the gradient) -----------------------------------------------------
def torch_loss(depth, alpha, prior, mask, *, mode="depth", w_global=1.0, w_local=0.0, patch=0, min_valid=16, alpha_min=0.0,
               offset=(0, 0)):
    """depth, alpha, prior [1,H,W] of one dtype, mask [1,H,W] -> (L, rho_image): pad, reshape, per-patch moments (no unfold)"""
    import torch
    import torch.nn.functional as Fn
    D = depth[0]
    used = (mask[0] != 0) & (alpha[0] >= alpha_min)
    zero = torch.zeros((), dtype=D.dtype, device=D.device)
    x = torch.where(used, D if mode == "depth" else 1.0 / (torch.where(used, D, zero + 1.0) + 1e-5), zero)
    y = torch.where(used, prior[0], zero)
    u = used.to(D.dtype)

    def terms(planes, dims):
        n, sx, sy, sxx, syy, sxy = (v.sum(dims) for v in planes)
        ns = n.clamp(min=1.0)
        cxx, cyy, cxy = sxx - sx * sx / ns, syy - sy * sy / ns, sxy - sx * sy / ns
        ok = (n >= min_valid) & (cxx > 0) & (cyy > 0)
        rho = cxy / torch.sqrt(torch.where(ok, cxx * cyy, zero + 1.0))
        return torch.where(ok, 1.0 - rho, zero), ok, rho

    planes = [u, x, y, x * x, y * y, x * y]
    tg, okg, rho = terms(planes, (0, 1))
    total = w_global * tg
    if patch and w_local != 0.0:
        H, W = D.shape
        ox, oy = offset
        gx, gy = -(-(W + ox) // patch), -(-(H + oy) // patch)
        tiles = [Fn.pad(v, (ox, gx * patch - W - ox, oy, gy * patch - H - oy)).reshape(gy, patch, gx, patch) for v in planes]
        tp, okp, _ = terms(tiles, (1, 3))
        total = total + w_local * (tp.sum() / okp.sum().clamp(min=1).to(D.dtype))
    return total, torch.where(okg, rho, zero)


# ---- the inputs the CPU and the device tests share --------------------------------------------------------------------------
# (W, H, patch, offset): partial border patches on all four sides; a last patch row of ONE pixel row; a wide, flat image
CASES = {"70x37_o0_0": (70, 37, 16, (0, 0)), "70x37_o15_15": (70, 37, 16, (15, 15)), "70x37_o5_9": (70, 37, 16, (5, 9)),
         "40x33_last_row_1px": (40, 33, 16, (0, 0)), "300x7_p8": (300, 7, 8, (3, 5))}
MIN_VALID, ALPHA_MIN = 12, 0.5


def patch_ids(W, H, p, offset):
    gx = (W + p - 1) // p + 1
    ys, xs = np.mgrid[0:H, 0:W]
    return ((ys + offset[1]) // p) * gx + (xs + offset[0]) // p


def make_case(W, H, p, offset, seed=0):
    """-> depth, alpha, prior float32 [1,H,W], mask uint8 [1,H,W], and the three patches (by index) that were prepared: the
    largest patch has a constant prior, the next one alpha below ALPHA_MIN, the third no valid pixel."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(F64)
    depth = (2.0 + 0.03 * xs + 0.05 * ys + 0.3 * np.sin(0.4 * xs) * np.cos(0.3 * ys) + 0.05 * rng.standard_normal((H, W))).astype(F32)
    prior = (0.5 * depth + 1.0 + 0.1 * rng.standard_normal((H, W))).astype(F32)
    alpha = (0.6 + 0.4 * rng.random((H, W))).astype(F32)
    mask = (rng.random((H, W)) >= 0.02).astype(np.uint8)
    pid = patch_ids(W, H, p, offset)
    ids, counts = np.unique(pid, return_counts=True)
    a, b, c = ids[np.argsort(-counts, kind="stable")[:3]]
    prior[pid == a] = 2.0
    alpha[pid == b] = 0.25
    mask[pid == c] = 0
    return depth[None], alpha[None], prior[None], mask[None], (int(a), int(b), int(c))
