"""The numpy float64 statement of csrc/pose.hip (include/b3gs_raster.h states the arithmetic): the per-row terms in the header's
operation order, the chunking rule, the workgroup tree and the one-wave fold.  The device equals pose_sums bit for bit
(tests/test_gpu_pose.py); tests/test_pose_cpu.py holds it against autograd of oracle/dense_torch.py through the camera.

Inputs are taken as float64 values as they come (float32 arrays widen exactly; the CPU identity test passes float64 gradients).

Mutants and ablation switches (as in edit_ref.py): mut="no_sh" drops the SH term, mut="quat_right" uses q (x) e_k in place of
e_k (x) q; mut="no_quat" drops the quaternion term, mut="mean_only" keeps the cross product alone.
"""
import numpy as np

TPB = 256
MAX_NB = 1024
R3, R6, R6H, R10H = 1.7320508075688772, 2.4494897427831779, 1.2247448713915890, 1.5811388300841898
# the header's statements "s, a, j, m" per band: (axis, a, j, m) in order
STATEMENTS = {
    1: ((0, 1.0, 0, 1), (1, 1.0, 1, 2), (2, 1.0, 0, 2)),
    2: ((0, 1.0, 0, 3), (0, R3, 1, 2), (0, 1.0, 1, 4), (1, -1.0, 0, 1), (1, R3, 2, 3), (1, 1.0, 3, 4), (2, 2.0, 0, 4), (2, 1.0, 1, 3)),
    3: ((0, R6H, 0, 5), (0, R10H, 1, 4), (0, R6H, 1, 6), (0, R6, 2, 3), (0, R10H, 2, 5), (1, -R6H, 0, 1), (1, -R10H, 1, 2),
        (1, R6, 3, 4), (1, R10H, 4, 5), (1, R6H, 5, 6), (2, 3.0, 0, 6), (2, 2.0, 1, 5), (2, 1.0, 2, 4)),
}
FIRST = {1: 0, 2: 3, 3: 8}          # the first features_rest row of a band


def generators():
    """(G1 [3,3,3], G2 [3,5,5], G3 [3,7,7]) from the statements: G[k][j][m] = a, G[k][m][j] = -a"""
    out = []
    for band in (1, 2, 3):
        n = 2 * band + 1
        G = np.zeros((3, n, n))
        for k, a, j, m in STATEMENTS[band]:
            G[k, j, m], G[k, m, j] = a, -a
        out.append(G)
    return tuple(out)


def nblocks(P):
    return min(max((P + 4 * TPB - 1) // (4 * TPB), 1), MAX_NB)


def row_parts(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree, mut=None):
    """-> (cross [P,3], h [P,3] (before the 1/2), s [P,3]) float64 in the header's operation order"""
    f64 = lambda a, cols: np.asarray(a, np.float64).reshape(-1, *cols)  # noqa: E731
    mu, q, g, gq = f64(xyz, (3,)), f64(rotation, (4,)), f64(gx, (3,)), f64(gr, (4,))
    c = np.asarray(pivot, np.float64).reshape(3)
    P = mu.shape[0]
    with np.errstate(all="ignore"):
        dx, dy, dz = mu[:, 0] - c[0], mu[:, 1] - c[1], mu[:, 2] - c[2]
        cross = np.stack([dy * g[:, 2] - dz * g[:, 1], dz * g[:, 0] - dx * g[:, 2], dx * g[:, 1] - dy * g[:, 0]], 1)
        qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        gw, gqx, gqy, gqz = gq[:, 0], gq[:, 1], gq[:, 2], gq[:, 3]
        if mut == "quat_right":          # <g_q, q (x) e_k>: the last two products change sign
            h = np.stack([((gqx * qw - gw * qx) - gqz * qy) + gqy * qz, ((gqy * qw - gw * qy) - gqx * qz) + gqz * qx,
                          ((gqz * qw - gw * qz) - gqy * qx) + gqx * qy], 1)
        else:
            h = np.stack([((gqx * qw - gw * qx) + gqz * qy) - gqy * qz, ((gqy * qw - gw * qy) + gqx * qz) - gqz * qx,
                          ((gqz * qw - gw * qz) + gqy * qx) - gqx * qy], 1)
        s = [np.zeros(P), np.zeros(P), np.zeros(P)]
        if sh_degree > 0:
            K = (sh_degree + 1) ** 2 - 1
            fr, gfr = f64(rest, (K, 3)), f64(gf, (K, 3))
            for band in range(1, sh_degree + 1):
                o = FIRST[band]
                for ch in range(3):
                    for k, a, j, m in STATEMENTS[band]:
                        s[k] = s[k] + a * (gfr[:, o + j, ch] * fr[:, o + m, ch] - gfr[:, o + m, ch] * fr[:, o + j, ch])
    return cross, h, np.stack(s, 1)


def row_terms(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree, mut=None):
    """[P,6]: (cross_k + 0.5 h_k) + s_k, g_mu_k"""
    cross, h, s = row_parts(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree, mut)
    with np.errstate(all="ignore"):
        if mut == "mean_only":
            tau = cross
        elif mut == "no_quat":
            tau = cross + s
        elif mut == "no_sh":
            tau = cross + 0.5 * h
        else:
            tau = (cross + 0.5 * h) + s
    return np.concatenate([tau, np.asarray(gx, np.float64).reshape(-1, 3)], 1)


def _butterfly(v):
    """xor butterfly 32, 16, .., 1 over the last axis (64 lanes): every lane ends with the same sum"""
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ d]
    return v[..., 0]


def fold(terms, skip=None):
    """[P,6] per-row terms -> the six sums in the kernel's order: thread t of workgroup g adds the rows 256 g + t, + 256 nb, ..
    in order from +0; the workgroup's butterfly, (wave 0 + wave 1) + (wave 2 + wave 3); one wave folds the partials b = lane,
    lane + 64, .. and its butterfly.  P = 0: zeros."""
    P = terms.shape[0]
    if P == 0:
        return np.zeros(6)
    with np.errstate(all="ignore"):
        if skip is not None:
            terms = np.where(np.asarray(skip).reshape(-1, 1) != 0, 0.0, terms)
        nb = nblocks(P)
        per = nb * TPB
        J = (P + per - 1) // per
        terms = np.concatenate([terms, np.zeros((J * per - P, 6))]).reshape(J, nb, TPB, 6)
        t = np.zeros((nb, TPB, 6))
        for j in range(J):
            t = t + terms[j]
        wv = _butterfly(np.moveaxis(t.reshape(nb, 4, 64, 6), 2, 3))          # [nb, 4, 6]
        part = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])                 # [nb, 6]
        lanes = np.zeros((64, 6))
        for b0 in range(0, nb, 64):
            seg = part[b0:b0 + 64]
            lanes[:len(seg)] = lanes[:len(seg)] + seg
        return _butterfly(lanes.T)


def pose_sums(xyz, rotation, rest, grads, skips, pivot, sh_degree, mut=None):
    """float64 [V,6] = {tau_x, tau_y, tau_z, f_x, f_y, f_z} of the SCENE twist per view; grads: [(gx, gr, gf)], skips: None or
    per view None / [P]"""
    out = []
    for v, (gx, gr, gf) in enumerate(grads):
        terms = row_terms(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree, mut)
        out.append(fold(terms, None if skips is None else skips[v]))
    return np.stack(out)


def abs_scale(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree, skip=None):
    """float64 [6]: the sums of the ABSOLUTE per-Gaussian parts, sum_i |cross_k| + |h_k / 2| + |s_k| and sum_i |g_mu_k| -- the
    size of what the six numbers are summed from, free of cancellation"""
    cross, h, s = row_parts(xyz, rotation, rest, gx, gr, gf, pivot, sh_degree)
    a = np.concatenate([np.abs(cross) + 0.5 * np.abs(h) + np.abs(s), np.abs(np.asarray(gx, np.float64).reshape(-1, 3))], 1)
    if skip is not None:
        a = np.where(np.asarray(skip).reshape(-1, 1) != 0, 0.0, a)
    return a.sum(0)
