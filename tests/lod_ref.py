"""The yardstick of binocular3dgs_amd/csrc/lod.hip: merging Gaussians into moment-matched levels of detail, restated from
include/b3gs_raster.h statement by statement.

Float32 statements are numpy float32 operations (one rounding each).  The fp64 statements of a merged Gaussian are written
on Python floats, which ARE IEEE binary64 (the same + - * / and math.sqrt, each correctly rounded, as numpy.float64; merely
quicker one scalar at a time), and on numpy float64 arrays for the colour channels; the kernel is compiled with
-ffp-contract=off, so a product and the sum that takes it are two roundings there as here.  Every output is rounded once to
float32.  The GPU test compares all of them bit for bit.

mutant: None, "no_ddT" (the covariance without the d d^T term) or "reverse" (members summed in reverse order): what the
parity checks must catch (tests/test_lod_ref_cpu.py).
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32
MAX_CELLS = 1024
NO_KEY = 0xFFFFFFFF
SWEEPS = 4          # B3GS_MERGE_JACOBI_SWEEPS of include/b3gs_raster.h
ALPHA_LO = 1.0 / 255.0
ALPHA_HI = 0.99


def _rot(A, V, p, q, r):
    """one Jacobi rotation in the plane (p, q) of the symmetric A (lists of lists, both triangles kept) and of V's columns"""
    apq = A[p][q]
    if apq == 0.0:
        return
    diff = A[q][q] - A[p][p]
    den = 2.0 * apq
    theta = diff / den
    th2 = theta * theta
    rt = math.sqrt(th2 + 1.0)
    sg = 1.0 if theta >= 0.0 else -1.0
    t = sg / (abs(theta) + rt)
    t2 = t * t
    c = 1.0 / math.sqrt(t2 + 1.0)
    s = t * c
    tau = t * apq
    A[p][p] = A[p][p] - tau
    A[q][q] = A[q][q] + tau
    A[p][q] = A[q][p] = 0.0
    arp, arq = A[r][p], A[r][q]
    rp = c * arp - s * arq
    rq = s * arp + c * arq
    A[r][p] = A[p][r] = rp
    A[r][q] = A[q][r] = rq
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = c * vkp - s * vkq
        V[k][q] = s * vkp + c * vkq


def _swap(lam, V, x, y):
    lam[x], lam[y] = lam[y], lam[x]
    for k in range(3):
        V[k][x], V[k][y] = V[k][y], V[k][x]


def jacobi(a00, a01, a02, a11, a12, a22, sweeps=SWEEPS):
    """-> (lam [3] descending, V 3x3 with the eigenvectors in its columns, det V = +1)"""
    A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(sweeps):
        _rot(A, V, 0, 1, 2)
        _rot(A, V, 0, 2, 1)
        _rot(A, V, 1, 2, 0)
    lam = [A[0][0], A[1][1], A[2][2]]
    if lam[1] > lam[0]:
        _swap(lam, V, 0, 1)
    if lam[2] > lam[1]:
        _swap(lam, V, 1, 2)
        if lam[1] > lam[0]:
            _swap(lam, V, 0, 1)
    det = ((V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]))
           + V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]))
    if det < 0.0:
        for k in range(3):
            V[k][2] = -V[k][2]
    return lam, V


def rotation_of(qw, qx, qy, qz):
    """the rotation matrix of a quaternion of any non-zero norm, normalised in fp64"""
    qn = math.sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz)
    qw, qx, qy, qz = qw / qn, qx / qn, qy / qn, qz / qn
    return [[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
            [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
            [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]]


def quaternion_of(V):
    """Shepperd's branches, one fixed rule; normalised, w >= 0"""
    tr = (V[0][0] + V[1][1]) + V[2][2]
    if tr > 0.0:
        s = math.sqrt(tr + 1.0) * 2.0
        q = [0.25 * s, (V[2][1] - V[1][2]) / s, (V[0][2] - V[2][0]) / s, (V[1][0] - V[0][1]) / s]
    elif V[0][0] > V[1][1] and V[0][0] > V[2][2]:
        s = math.sqrt(((1.0 + V[0][0]) - V[1][1]) - V[2][2]) * 2.0
        q = [(V[2][1] - V[1][2]) / s, 0.25 * s, (V[0][1] + V[1][0]) / s, (V[0][2] + V[2][0]) / s]
    elif V[1][1] > V[2][2]:
        s = math.sqrt(((1.0 + V[1][1]) - V[0][0]) - V[2][2]) * 2.0
        q = [(V[0][2] - V[2][0]) / s, (V[0][1] + V[1][0]) / s, 0.25 * s, (V[1][2] + V[2][1]) / s]
    else:
        s = math.sqrt(((1.0 + V[2][2]) - V[0][0]) - V[1][1]) * 2.0
        q = [(V[1][0] - V[0][1]) / s, (V[0][2] + V[2][0]) / s, (V[1][2] + V[2][1]) / s, 0.25 * s]
    qn = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    q = [x / qn for x in q]
    if q[0] < 0.0:
        q = [-x for x in q]
    return q


def moments(idx, pos, scale, quat, alpha, weights=None, mutant=None):
    """The fp64 moments of one cluster (idx: its members in order) -> dict of Python floats / lists, before any rounding:
    M, sum_a, m (per member), mu, Sigma (six entries 00 01 02 11 12 22), smin."""
    if mutant == "reverse":
        idx = list(idx)[::-1]
    a_i, sum_a, sum_m = [], 0.0, 0.0
    smin = F(np.finfo(F).max)
    for i in idx:
        s0, s1, s2 = (float(x) for x in scale[i])
        smin = min(smin, scale[i].min())
        v = (s0 * s1) * s2
        ai = float(alpha[i]) * v
        a_i.append(ai)
        sum_a = sum_a + ai
        if weights is not None:
            sum_m = sum_m + float(weights[i]) * ai
    weighted = weights is not None and sum_m != 0.0
    M = sum_m if weighted else sum_a
    m = [float(weights[i]) * ai if weighted else ai for i, ai in zip(idx, a_i)]
    S = [0.0, 0.0, 0.0]
    for i, mi in zip(idx, m):
        for k in range(3):
            S[k] = S[k] + mi * float(pos[i][k])
    mu = [S[0] / M, S[1] / M, S[2] / M]
    C = [0.0] * 6
    for i, mi in zip(idx, m):
        R = rotation_of(*(float(x) for x in quat[i]))
        var = [float(scale[i][k]) * float(scale[i][k]) for k in range(3)]
        d = [float(pos[i][k]) - mu[k] for k in range(3)]
        e = 0
        for x in range(3):
            for y in range(x, 3):
                cov = ((R[x][0] * var[0]) * R[y][0] + (R[x][1] * var[1]) * R[y][1]) + (R[x][2] * var[2]) * R[y][2]
                C[e] = C[e] + mi * (cov if mutant == "no_ddT" else cov + d[x] * d[y])
                e += 1
    return {"M": M, "sum_a": sum_a, "m": m, "mu": mu, "Sigma": [c / M for c in C], "smin": float(smin), "idx": list(idx)}


def merged(mo):
    """the moments of one cluster -> fp64 (mu [3], scales [3], quaternion [4], alpha, volume), before the rounding"""
    lam, V = jacobi(*mo["Sigma"])
    fl = mo["smin"] * mo["smin"]
    sc = [math.sqrt(fl if l < fl else l) for l in lam]
    q = quaternion_of(V)
    vol = (sc[0] * sc[1]) * sc[2]
    al = mo["sum_a"] / vol
    al = ALPHA_LO if al < ALPHA_LO else (ALPHA_HI if al > ALPHA_HI else al)
    return mo["mu"], sc, q, al, vol


def colours(mo, dc, rest):
    """every channel: sum m_i f_i / M, members in order -> (dc [3], rest [3 K]) float64 arrays"""
    acc_d = np.zeros(3, np.float64)
    acc_r = np.zeros(rest.shape[1], np.float64)
    for i, mi in zip(mo["idx"], mo["m"]):
        acc_d = acc_d + np.float64(mi) * dc[i].astype(np.float64)
        acc_r = acc_r + np.float64(mi) * rest[i].astype(np.float64)
    return acc_d / np.float64(mo["M"]), acc_r / np.float64(mo["M"])


def cell_keys(pos, scale, cell):
    """-> (key uint32 [P]: 30 bits z-major, NO_KEY for a Gaussian that is not mergeable; rows beyond the 1024 cells of an axis)"""
    P = pos.shape[0]
    cell = F(cell)
    if P == 0:
        return np.zeros(0, np.uint32), 0
    with np.errstate(all="ignore"):
        o = np.fmin.reduce(pos, axis=0).astype(F)
        c = np.floor(((pos - o).astype(F) / cell).astype(F))
        ok = (c >= 0) & (c < MAX_CELLS)
        over = ~ok.all(axis=1)
        ci = np.where(ok, c, 0).astype(np.uint32)
        key = ci[:, 0] | (ci[:, 1] << np.uint32(10)) | (ci[:, 2] << np.uint32(20))
        key = np.where(over, np.uint32(0), key)
        big = np.maximum(np.maximum(scale[:, 0], scale[:, 1]), scale[:, 2])
        key = np.where(big <= cell, key, np.uint32(NO_KEY)).astype(np.uint32)
    return key, int(over.sum())


def merge(pos, scale, quat, alpha, dc, rest, cell, weights=None, mutant=None):
    """The whole rule on numpy arrays (float32 [P,3], [P,3], [P,4], [P], [P,3], [P,3K]; weights float64 [P] or None) -> dict:
    positions, scales, quaternions, opacities, features_dc, features_rest (float32), cluster_of, members (int32), totals
    {clusters, pass, merged, nonfinite, over}.  With a non-zero error count only the totals are returned."""
    P = pos.shape[0]
    rest = rest.reshape(P, int(np.prod(rest.shape[1:])))
    dc = dc.reshape(P, 3)
    fin = (np.isfinite(pos).all(1) & np.isfinite(scale).all(1) & np.isfinite(quat).all(1) & np.isfinite(alpha) & np.isfinite(dc).all(1)
           & np.isfinite(rest).all(1))
    if weights is not None:
        fin &= np.isfinite(weights)
    key, over = cell_keys(pos, scale, cell)
    order = np.argsort(key, kind="stable")
    sk = key[order]
    head = np.ones(P, bool)
    head[1:] = (sk[1:] != sk[:-1]) | (sk[1:] == NO_KEY)
    row_of_sorted = np.cumsum(head) - 1
    rows = int(head.sum())
    starts = np.append(np.flatnonzero(head), P)
    members = np.diff(starts).astype(np.int32)
    cluster_of = np.empty(P, np.int32)
    cluster_of[order] = row_of_sorted.astype(np.int32)
    npass = int((key == NO_KEY).sum())
    totals = {"clusters": rows - npass, "pass": npass, "merged": int(members[members >= 2].sum()), "nonfinite": int((~fin).sum()),
              "over": over}
    if totals["nonfinite"] or totals["over"]:
        return {"totals": totals}
    out = {"positions": np.empty((rows, 3), F), "scales": np.empty((rows, 3), F), "quaternions": np.empty((rows, 4), F),
           "opacities": np.empty(rows, F), "features_dc": np.empty((rows, 3), F), "features_rest": np.empty((rows, rest.shape[1]), F),
           "cluster_of": cluster_of, "members": members, "totals": totals}
    for r in range(rows):
        idx = order[starts[r]:starts[r + 1]]
        if len(idx) == 1:
            i = idx[0]
            for name, src in (("positions", pos), ("scales", scale), ("quaternions", quat), ("opacities", alpha), ("features_dc", dc),
                              ("features_rest", rest)):
                out[name][r] = src[i]
            continue
        mo = moments(idx, pos, scale, quat, alpha, weights, mutant)
        mu, sc, q, al, _ = merged(mo)
        cd, cr = colours(mo, dc, rest)
        out["positions"][r] = np.array(mu, np.float64).astype(F)
        out["scales"][r] = np.array(sc, np.float64).astype(F)
        out["quaternions"][r] = np.array(q, np.float64).astype(F)
        out["opacities"][r] = F(np.float64(al))
        out["features_dc"][r] = cd.astype(F)
        out["features_rest"][r] = cr.astype(F)
    return out


# ---- test data shared by the CPU mutants and the GPU parity test -----------------------------------------------------------------
def random_gaussians(P, K, seed, extent=4.0, scale=(0.01, 0.2)):
    """activated float32 inputs: positions in [0, extent)^3, log-uniform scales, unnormalised quaternions of either sign of w"""
    g = np.random.default_rng(seed)
    pos = (g.random((P, 3)) * extent).astype(F)
    sc = np.exp(g.uniform(math.log(scale[0]), math.log(scale[1]), (P, 3))).astype(F)
    quat = (g.normal(size=(P, 4)) * g.uniform(0.5, 2.0, (P, 1))).astype(F)
    alpha = g.uniform(0.02, 0.98, P).astype(F)
    dc = g.normal(size=(P, 3)).astype(F)
    rest = (g.normal(size=(P, 3 * K)) * 0.3).astype(F)
    return pos, sc, quat, alpha, dc, rest


OUTPUTS = ("positions", "scales", "quaternions", "opacities", "features_dc", "features_rest", "cluster_of", "members")


def same_bits(a: dict, b: dict) -> bool:
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in OUTPUTS)


def _with(arrs, **kw):
    names = ("pos", "scale", "quat", "alpha", "dc", "rest")
    d = dict(zip(names, (a.copy() for a in arrs)))
    d.update(kw)
    return tuple(d[n] for n in names)


SIZES = (0, 1, 63, 64, 65, 257, 2000)
DEGREES = (0, 1, 2, 3)


def cases():
    """name -> (the six input arrays, cell, weights or None): the CPU data of tests/test_gpu_lod.py"""
    out = {}
    for P in SIZES:                                        # every size at every SH degree: a few members per cluster
        for deg in DEGREES:
            K = (deg + 1) ** 2 - 1
            out[f"P{P}_deg{deg}"] = (random_gaussians(P, K, seed=100 * deg + P % 97), 0.75 if P < 2000 else 0.5, None)
    g = np.random.default_rng(7)
    # a cell so fine that every cluster is one Gaussian (scales below it: all of them mergeable)
    out["singletons"] = (random_gaussians(2000, 3, seed=1, scale=(1e-4, 1e-3)), 4.0 / 1000.0, None)
    # one cell holds all 2000: the long member loop, 32 chunks of the colour kernel
    out["one_cell"] = (random_gaussians(2000, 15, seed=2), 8.0, None)
    out["one_cell_weighted"] = (random_gaussians(2000, 3, seed=3), 8.0, g.uniform(0.0, 5.0, 2000))
    # 4500 Gaussians in 5 x 5 x 5 cells of about 36: clusters straddle the 256-thread workgroups of every kernel, the 32-row
    # blocks and 64-member chunks of the colour kernel and the 4096-key tile of the sort
    out["straddle"] = (random_gaussians(4500, 3, seed=4, scale=(0.01, 0.1)), 0.8, g.uniform(0.0, 2.0, 4500))
    # pass-throughs: every fifth Gaussian has a scale above the cell, one has its largest scale exactly equal to it (mergeable)
    a = random_gaussians(257, 8, seed=5, scale=(0.01, 0.2))
    sc = a[1].copy()
    sc[::5, 1] = F(0.9)
    sc[3] = (F(0.1), F(0.75), F(0.2))
    sc[4] = np.nextafter(F(0.75), F(1)), F(0.1), F(0.1)
    out["pass_through"] = (_with(a, scale=sc), 0.75, None)
    # weights: a cluster whose weights are all 0 (w = 1 there), clusters with one zero-weight member
    a = random_gaussians(257, 3, seed=6)
    w = g.uniform(0.1, 3.0, 257)
    key, _ = cell_keys(a[0], a[1], 1.0)
    big = np.bincount(key[key != NO_KEY] & 0xFFFF).argmax()          # (keys of 4 x 4 x 4 cells fit 30 bits; the low ones do)
    w[(key & 0xFFFF) == big] = 0.0
    w[::7] = 0.0
    out["weights_zero"] = (a, 1.0, w)
    # degenerate clusters, all in one cell
    a = random_gaussians(64, 3, seed=8)
    out["coincident"] = (_with(a, pos=np.tile(a[0][:1], (64, 1))), 8.0, None)
    pos = np.zeros((65, 3), F)
    pos[:, 0] = np.linspace(0.0, 3.0, 65, dtype=F)
    flat = np.tile(np.array([[0.05, 1e-6, 0.02]], F), (65, 1))
    quat = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], F), (65, 1))
    a = random_gaussians(65, 3, seed=9)
    out["collinear_flat"] = (_with(a, pos=pos, scale=flat, quat=quat), 8.0, None)
    a = random_gaussians(63, 8, seed=10)
    out["identical"] = (tuple(np.tile(x[:1], (63,) + (1,) * (x.ndim - 1)) for x in _with(a, alpha=np.full(63, 0.6, F))), 8.0, None)
    # Equal masses and colour values +B, small ones, -B: the big terms cancel and what is left of the small ones depends on the
    # order of the additions at a level float32 still shows (elsewhere fp64 order effects, 1e-16, vanish in the rounding)
    a = random_gaussians(8, 3, seed=13)
    dc, rest = a[4].copy(), a[5].copy()
    dc[:, 0] = [2.0 ** 36, 0.3, 0.7, 1.1, -2.0 ** 36, 0.2, 0.9, 0.4]
    rest[:, 4] = [0.3, 2.0 ** 33, 0.7, 1.1, 0.2, 0.9, -2.0 ** 33, 0.4]
    out["cancelling_colours"] = (_with(a, scale=np.tile(a[1][:1], (8, 1)), alpha=np.full(8, 0.5, F), dc=dc, rest=rest), 8.0, None)
    return out
