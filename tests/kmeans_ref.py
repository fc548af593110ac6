"""numpy float64 yardstick of csrc/kmeans.hip (not a test module): the scores of every (row, code) with the rounding bound of
the float32 chain the kernel runs, the update and the distortion in the kernel's documented summation order, and the seeded
cases the CPU and the GPU tests share.

The kernel's score of (n, k) is the float32 chain a_0 = -h_k, a_{d+1} = fmaf(x_nd, c_kd, a_d) with h_k = float32(|c_k|^2 / 2).
Against the exact s_nk = x_n . c_k - |c_k|^2 / 2 a chain of D fused multiply-adds started from a rounded h_k is off by at most

    e_nk = gamma (h_k + sum_d |x_nd| |c_kd|) + u h_k,    gamma = (D + 1) u / (1 - (D + 1) u),  u = 2^-24

(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: the bound of a length D + 1 inner product; u h_k is the
rounding of h_k itself).  It is derived, not measured.  A row is DECIDED when its best fp64 score beats every other code by more
than the two bounds together: then every correct implementation returns that code.
"""
import numpy as np

U = 2.0 ** -24
CHUNK = 256        # members of an update chunk
TPB = 256          # threads of a distortion workgroup
DBLOCKS = 256      # most distortion partials
ROW_TILE = 512     # data rows of an assignment workgroup
CODE_TILE = 128    # codes staged per step (the MFMA tile is 32)


def half_norms(c):
    """float32 of |c_k|^2 / 2, the sum in fp64 with d ascending."""
    c64 = np.asarray(c, np.float32).astype(np.float64)
    s = np.zeros(c64.shape[0])
    for d in range(c64.shape[1]):
        s = s + c64[:, d] * c64[:, d]
    return (0.5 * s).astype(np.float32)


def scores(x, c):
    """fp64 [N,K]: x_n . c_k - |c_k|^2 / 2."""
    x64, c64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    return x64 @ c64.T - 0.5 * (c64 * c64).sum(1)[None, :]


def bounds(x, c):
    """fp64 [N,K]: e_nk of the module docstring."""
    x64, c64 = np.abs(np.asarray(x, np.float32).astype(np.float64)), np.abs(np.asarray(c, np.float32).astype(np.float64))
    D = x64.shape[1]
    gamma = (D + 1) * U / (1.0 - (D + 1) * U)
    h = 0.5 * (c64 * c64).sum(1)
    return gamma * (h[None, :] + x64 @ c64.T) + U * h[None, :]


def assign(x, c):
    """-> (best [N] int64: the smallest k of the largest fp64 score, decided [N] bool, S, E)."""
    S, E = scores(x, c), bounds(x, c)
    best = np.argmax(S, axis=1)
    rows = np.arange(S.shape[0])
    gap = S[rows, best][:, None] - S
    need = E[rows, best][:, None] + E
    need[rows, best] = -1.0
    return best, np.all(gap > need, axis=1), S, E


def admissible(codes, best, S, E):
    """bool [N]: codes[n] scores within the two bounds of the best."""
    rows = np.arange(S.shape[0])
    codes = np.asarray(codes, np.int64)
    return S[rows, best] - S[rows, codes] <= E[rows, best] + E[rows, codes]


def step_bound(x, c, w=None):
    """sum_n w_n 2 max_k e_nk: how far a Lloyd step's distortion may rise because assignments are decided in float32."""
    e = 2.0 * bounds(x, c).max(axis=1)
    return float(e.sum() if w is None else (np.asarray(w, np.float32).astype(np.float64) * e).sum())


def update(x, w, codes, c):
    """The kernel's update: members of a code in row order, chunks of CHUNK members summed from 0 in member order, chunk sums
    added from 0 in chunk order; c_k = float32(S / W); no member or W == 0 keeps the centroid."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    N, D = x64.shape
    w64 = np.ones(N) if w is None else np.asarray(w, np.float32).astype(np.float64)
    codes = np.asarray(codes, np.int64)
    terms = np.concatenate([x64 * w64[:, None], w64[:, None]], axis=1)      # every product is exact
    out = np.array(c, np.float32, copy=True)
    order = np.argsort(codes, kind="stable")
    starts = np.searchsorted(codes[order], np.arange(out.shape[0] + 1))
    for k in range(out.shape[0]):
        m = order[starts[k]:starts[k + 1]]
        if m.size == 0:
            continue
        tot = np.zeros(D + 1)
        for j in range(0, m.size, CHUNK):
            s = np.zeros(D + 1)
            for row in m[j:j + CHUNK]:
                s = s + terms[row]
            tot = tot + s
        if tot[D] != 0.0:
            out[k] = (tot[:D] / tot[D]).astype(np.float32)
    return out


def _butterfly(v):
    """xor butterfly 32, 16, .., 1 over the last axis (64 lanes): every lane ends with the same sum."""
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ d]
    return v[..., 0]


def distortion(x, w, c, codes):
    """sum_n w_n |x_n - c_code(n)|^2 in the kernel's order (csrc/kmeans.hip, DISTORTION)."""
    x64, c64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    N, D = x64.shape
    df = x64 - c64[np.asarray(codes, np.int64)]
    a = np.zeros(N)
    for d in range(D):
        a = a + df[:, d] * df[:, d]
    v = a if w is None else np.asarray(w, np.float32).astype(np.float64) * a
    nb = min((N + TPB - 1) // TPB, DBLOCKS)
    per = nb * TPB
    J = (N + per - 1) // per
    v = np.concatenate([v, np.zeros(J * per - N)]).reshape(J, nb, TPB)
    t = np.zeros((nb, TPB))
    for j in range(J):
        t = t + v[j]
    wv = _butterfly(t.reshape(nb, 4, 64))
    part = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])
    lanes = np.zeros(64)
    for b0 in range(0, nb, 64):
        seg = part[b0:b0 + 64]
        lanes[:seg.size] = lanes[:seg.size] + seg
    return float(_butterfly(lanes))


# ---- the seeded cases the CPU test (undecided share) and the GPU test (the device) share ------------------------------------
FLOAT_CASES = [(3001, 33, 7, 101), (2999, 257, 7, 102), (3000, 33, 12, 103), (3001, 257, 12, 104), (2999, 33, 48, 105),
               (3000, 257, 48, 106)]      # (N, K, D, seed)


def float_case(N, K, D, seed):
    """x ~ N(0, 1) [N,D] float32 and a codebook of K of its rows moved by N(0, 0.1)."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, D)).astype(np.float32)
    c = (x[g.choice(N, K, replace=False)] + 0.1 * g.standard_normal((K, D))).astype(np.float32)
    return x, c


def integer_case(N, K, D, seed, duplicates=False):
    """Integers in [-8, 8]: every float32 chain is exact.  duplicates: the upper half of the codebook repeats the lower half."""
    g = np.random.default_rng(seed)
    x = g.integers(-8, 9, (N, D)).astype(np.float32)
    c = g.integers(-8, 9, (K, D)).astype(np.float32)
    if duplicates and K > 1:
        c[K // 2:K // 2 * 2] = c[:K // 2]
    return x, c
