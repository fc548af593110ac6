"""Yardstick of the exposure kernels (csrc/exposure.hip; the rules are stated in include/b3gs_raster.h): numpy float64 in the
kernels' own operation orders -- the block tree, the fold, the Cholesky order, the running beta products -- so that every output
is meant to be equal bit for bit.

`mutant` of backward(): "transposed" applies A transposed in g_in, "no_bias" leaves the bias column out of G; the GPU parity
tests must tell both from the kernel."""
from __future__ import annotations

import numpy as np

F64, F32 = np.float64, np.float32
LANES = np.arange(64)
IDENTITY = np.eye(3, 4, dtype=F32)


def _butterfly(v, axis):
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


def plane_sum(q):
    """q [npix, k] per-pixel quantities -> [k]: one partial per 256-pixel block (tree), the partials folded in block order"""
    npix, k = q.shape
    nb = -(-npix // 256)
    pad = np.zeros((nb * 256, k), F64)
    pad[:npix] = q
    return fold(tree256(pad.reshape(nb, 256, k)))


def _planes(image):
    x = np.asarray(image, F32)
    return x.reshape(3, -1).astype(F64), x.shape


def apply(image, A):
    """-> float32 [3, H, W]: ((t + a0 r) + a1 g) + a2 b in float64, rounded once"""
    x, shape = _planes(image)
    a = np.asarray(A, F32).reshape(3, 4).astype(F64)
    out = [((a[c, 3] + a[c, 0] * x[0]) + a[c, 1] * x[1]) + a[c, 2] * x[2] for c in range(3)]
    return np.stack(out).astype(F32).reshape(shape)


def backward(images, g_outs, A, mutant=None):
    """The planes that share the matrix A -> (g_in per plane float32 [3, H, W], G float64 [3, 4]): the planes' folds added in
    plane order to +0."""
    a = np.asarray(A, F32).reshape(3, 4).astype(F64)
    if mutant == "transposed":
        a = np.concatenate([a[:, :3].T, a[:, 3:]], axis=1)
    total = np.zeros(12, F64)
    g_ins = []
    for image, g_out in zip(images, g_outs):
        x, shape = _planes(image)
        g, _ = _planes(g_out)
        g_ins.append(np.stack([(a[0, k] * g[0] + a[1, k] * g[1]) + a[2, k] * g[2] for k in range(3)]).astype(F32).reshape(shape))
        q = np.zeros((x.shape[1], 12), F64)
        for c in range(3):
            for k in range(3):
                q[:, 4 * c + k] = g[c] * x[k]
            if mutant != "no_bias":
                q[:, 4 * c + 3] = g[c]
        total = total + plane_sum(q)
    return g_ins, total.reshape(3, 4)


AT = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))        # S[i][j] among the 10 unique entries


def fit_sums(render, gt, mask=None):
    """-> float64 [23]: n, the 10 unique entries of S (rr rg rb r gg gb g bb b n), the 12 of B[c][i]"""
    x, _ = _planes(render)
    y, _ = _planes(gt)
    npix = x.shape[1]
    used = np.ones(npix, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)
    x4 = np.concatenate([x, np.ones((1, npix), F64)])
    q = np.zeros((npix, 22), F64)
    at = 0
    for i in range(4):
        for j in range(i, 4):
            q[:, at] = x4[i] * x4[j]
            at += 1
    for c in range(3):
        for i in range(4):
            q[:, 10 + 4 * c + i] = x4[i] * y[c]
    q[~used] = 0.0
    f = plane_sum(q)
    return np.concatenate([f[9:10], f])


def solve(sums, rounded=True):
    """sums [23] -> (A float32 [3, 4], flag): the Cholesky order of the header; degenerate -> (identity, 1).
    rounded=False: the float64 solution before its one rounding."""
    f = np.asarray(sums, F64)[1:]
    n = f[9]
    if not n >= 16.0:
        return IDENTITY.copy(), 1
    trace = ((f[0] + f[4]) + f[7]) + f[9]
    thr = trace * F64(2.0 ** -40)
    L = np.zeros((4, 4), F64)
    with np.errstate(all="ignore"):
        for j in range(4):
            d = f[AT[j][j]]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            if not d > thr:
                return IDENTITY.copy(), 1
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 4):
                s = f[AT[i][j]]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        A = np.zeros((3, 4), F64)
        for c in range(3):
            y = np.zeros(4, F64)
            a = np.zeros(4, F64)
            for i in range(4):
                s = f[10 + 4 * c + i]
                for k in range(i):
                    s = s - L[i, k] * y[k]
                y[i] = s / L[i, i]
            for i in (3, 2, 1, 0):
                s = y[i]
                for k in range(i + 1, 4):
                    s = s - L[k, i] * a[k]
                a[i] = s / L[i, i]
            A[c] = a
    return (A.astype(F32) if rounded else A), 0


def fit(render, gt, mask=None):
    """-> (A float32 [3, 4], flag, sums float64 [23])"""
    sums = fit_sums(render, gt, mask)
    A, flag = solve(sums)
    return A, flag, sums


def matrix_of_sums(sums):
    """S [4, 4] and B [4, 3] of a sums vector (for lstsq comparisons)"""
    f = np.asarray(sums, F64)[1:]
    S = np.array([[f[AT[i][j]] for j in range(4)] for i in range(4)])
    return S, f[10:].reshape(3, 4).T


def adam(state, row, grad, lr, beta1=0.9, beta2=0.999, eps=1e-8, skip=0):
    """state: dict(table, exp_avg, exp_avg_sq float32 [V, 3, 4], steps int32 [V], prods float64 [V, 2]) -> the new state (a
    copy); only `row` moves; skip != 0 or a row outside the table: nothing does."""
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    V = s["steps"].shape[0]
    if skip or not 0 <= row < V:
        return s
    b1, b2 = F64(beta1), F64(beta2)
    p1, p2 = s["prods"][row, 0] * b1, s["prods"][row, 1] * b2
    s["prods"][row] = (p1, p2)
    s["steps"][row] += 1
    g = np.asarray(grad, F64).reshape(3, 4)
    lr = F64(F32(lr))
    m = b1 * s["exp_avg"][row].astype(F64) + (1.0 - b1) * g
    v = b2 * s["exp_avg_sq"][row].astype(F64) + ((1.0 - b2) * g) * g
    mhat = m / (1.0 - p1)
    den = np.sqrt(v) / np.sqrt(1.0 - p2) + F64(eps)
    s["exp_avg"][row] = m.astype(F32)
    s["exp_avg_sq"][row] = v.astype(F32)
    s["table"][row] = (s["table"][row].astype(F64) - (lr * mhat) / den).astype(F32)
    return s


def new_state(V):
    return dict(table=np.repeat(IDENTITY[None], V, 0).copy(), exp_avg=np.zeros((V, 3, 4), F32), exp_avg_sq=np.zeros((V, 3, 4), F32),
                steps=np.zeros(V, np.int32), prods=np.ones((V, 2), F64))
