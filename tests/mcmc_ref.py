"""The yardstick of binocular3dgs_amd/mcmc.py (csrc/mcmc.hip): every rule of include/b3gs_raster.h's MCMC section restated with
numpy and the standard library -- Philox4x32-10 from its definition, the integer weights and their scans in Python integers,
sampling by mulhi and searchsorted, the correction in float64 in the kernel's operation order, the noise in float64.

Two MUTANTS that the tests must reject (relocate_ref(mutant=...)):
  "ge"      sampling takes the first row with W >= t instead of W > t: it lands on zero-weight (dead) rows
  "count"   N = count instead of count + 1
"""
import math
from itertools import accumulate

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
N_MAX = 51


def philox4x32(counter, key, rounds=10):
    """One block: counter (4 words), key (2 words) -> 4 words.  Python integers."""
    c = [int(x) & MASK for x in counter]
    k = [int(x) & MASK for x in key]
    for r in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def philox_blocks(index, offset, stream_id, seed):
    """Vectorised over `index` (array of block indices): -> uint64 [n, 4] holding 32-bit words."""
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    c0 = np.asarray(index, dtype=np.uint64) & m
    c1 = np.full_like(c0, int(offset) & MASK)
    c2 = np.full_like(c0, int(stream_id) & MASK)
    c3 = np.zeros_like(c0)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for r in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=1)


def random_u32(n, seed, stream_id, offset):
    """element e = word e % 4 of the block with index e / 4"""
    b = philox_blocks(np.arange((n + 3) // 4), offset, stream_id, seed)
    return b.reshape(-1)[:n].astype(np.uint32)


def random_normal64(n, seed, stream_id, offset):
    """float64, NOT rounded: element e from block e / 4, pair (w0, w1) for e % 4 < 2 else (w2, w3); even e: cos, odd e: sin"""
    b = philox_blocks(np.arange((n + 3) // 4), offset, stream_id, seed).astype(np.float64)
    pairs = b.reshape(-1, 2)
    u1, u2 = (pairs[:, 0] + 0.5) * 2.0 ** -32, (pairs[:, 1] + 0.5) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.stack([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)], axis=1)
    return out.reshape(-1)[:n]


def draws64(n, seed, offset):
    """the 64-bit draws of dead ranks 0 .. n-1 (stream_id 1): w0 | w1 << 32, Python integers"""
    b = philox_blocks(np.arange(n), offset, 1, seed)
    return [int(w0) | (int(w1) << 32) for w0, w1 in zip(b[:, 0], b[:, 1])]


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-np.asarray(raw, dtype=np.float32).astype(np.float64)))


def classify(opacity_raw, P_old, min_opacity):
    """-> dead bool [P], q Python integers [P]"""
    o = sigmoid64(np.asarray(opacity_raw).reshape(-1))
    dead = (o <= float(np.float32(min_opacity))) | (np.arange(o.shape[0]) >= P_old)
    q = [0 if d else int(x * 16777216.0) for d, x in zip(dead, o)]
    return dead, q


def scans(dead, q):
    """-> rank (the dead rows in front), W (inclusive sums), total; Python integers"""
    d = [int(x) for x in dead]
    incl = list(accumulate(d))
    rank = [a - b for a, b in zip(incl, d)]
    W = list(accumulate(q))
    return rank, W, (W[-1] if W else 0)


def sample(dead, rank, W, total, draws, mutant=None):
    """-> src int64 [P] (-1: not relocated), count int64 [P]"""
    P = len(W)
    src = np.full(P, -1, dtype=np.int64)
    count = np.zeros(P, dtype=np.int64)
    if total == 0:
        return src, count
    Wa = np.array(W, dtype=np.uint64)
    for i in range(P):
        if not dead[i]:
            continue
        t = (int(draws[rank[i]]) * total) >> 64
        s = int(np.searchsorted(Wa, np.uint64(t), side="left" if mutant == "ge" else "right"))
        src[i] = s
        count[s] += 1
    return src, count


def binomial(n, k):
    return float(math.comb(n, k))


def corrected(o, N, scale_raw, min_opacity):
    """float64 in the kernel's order -> (raw opacity, raw scales [3]) as float64, NOT rounded; also (o', denom)"""
    o = float(o)
    on = 1.0 - math.pow(1.0 - o, 1.0 / float(N))
    denom = 0.0
    for a in range(1, N + 1):
        p = on
        for k in range(a):
            term = (binomial(a - 1, k) * p) / math.sqrt(float(k + 1))
            denom = denom - term if k & 1 else denom + term
            p = p * on
    lo, hi = float(np.float32(min_opacity)), 1.0 - 2.0 ** -24
    oc = min(max(on, lo), hi)
    raw_o = math.log(oc / (1.0 - oc))
    raw_s = [math.log((math.exp(float(np.float32(s))) * o) / denom) for s in scale_raw]
    return raw_o, raw_s, on, denom


def relocate_ref(params, P_old=None, min_opacity=0.005, n_max=N_MAX, seed=0, offset=0, draws=None, moments=None, mutant=None):
    """params: six float32 arrays in model order (xyz, features_dc, features_rest, scaling, rotation, opacity).
    -> dict(src, count, rank, wsum, total, dead, params (new float32 arrays; opacity / scaling ALSO as float64 in params64),
    written bool [P], moments)"""
    xyz, dc, rest, scaling, rotation, opacity = [np.array(p, dtype=np.float32, copy=True) for p in params]
    P = xyz.shape[0]
    P_old = P if P_old is None else P_old
    dead, q = classify(opacity, P_old, min_opacity)
    rank, W, total = scans(dead, q)
    n_dead = int(np.sum(dead))
    if draws is None:
        draws = draws64(n_dead, seed, offset)
    src, count = sample(dead, rank, W, total, draws, mutant)
    o64 = sigmoid64(opacity.reshape(-1))
    new_o, new_s = opacity.reshape(-1).astype(np.float64), scaling.reshape(P, 3).astype(np.float64)
    out_o, out_s = new_o.copy(), new_s.copy()
    written = np.zeros(P, dtype=bool)
    fresh = {}
    for i in range(P):
        if dead[i] or count[i] <= 0:
            continue
        N = int(count[i]) if mutant == "count" else int(count[i]) + 1
        N = max(1, min(N, n_max))
        ro, rs, _, _ = corrected(o64[i], N, scaling.reshape(P, 3)[i], min_opacity)
        fresh[i] = (ro, rs)
        out_o[i], out_s[i] = ro, rs
        written[i] = True
    flat = [xyz.reshape(P, -1), dc.reshape(P, -1), rest.reshape(P, -1), None, rotation.reshape(P, -1), None]
    for i in range(P):
        s = int(src[i])
        if s < 0 or s not in fresh:
            continue                                    # (the "ge" mutant lands on dead rows: no corrected values there)
        for t in (0, 1, 2, 4):
            flat[t][i] = flat[t][s]
        out_o[i], out_s[i] = fresh[s]
        written[i] = True
    res = dict(src=src, count=count, rank=np.array(rank, dtype=np.int64), wsum=np.array(W, dtype=np.uint64), total=total, dead=dead,
               written=written, opacity64=out_o, scaling64=out_s,
               params=[xyz, dc, rest, out_s.astype(np.float32).reshape(scaling.shape), rotation, out_o.astype(np.float32).reshape(opacity.shape)])
    if moments is not None:
        res["moments"] = [np.where(written.reshape((P,) + (1,) * (m.ndim - 1)), 0.0, m).astype(np.float32) for m in moments]
    return res


def rotation_matrix64(q):
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)
    return R


def noise_ref(scaling, rotation, opacity, normals, noise_lr, lr_xyz):
    """float64: -> (the step Sigma n g noise_lr lr [P,3], g [P], max s [P])"""
    s = np.exp(np.asarray(scaling, dtype=np.float64))
    R = rotation_matrix64(rotation)
    n = np.asarray(normals, dtype=np.float64)
    t = np.einsum("pjk,pj->pk", R, n) * s * s
    d = np.einsum("pjk,pk->pj", R, t)
    o = 1.0 / (1.0 + np.exp(-np.asarray(opacity, dtype=np.float64).reshape(-1)))
    with np.errstate(over="ignore"):
        g = 1.0 / (1.0 + np.exp(100.0 * (o - 0.005)))
    return d * g[:, None] * (float(noise_lr) * float(lr_xyz)), g, s.max(axis=1)


def ulp32(x):
    """the spacing of float32 at |x| (float64 array)"""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


# ---- the shared cases of tests/test_mcmc_cpu.py and tests/test_gpu_mcmc.py ------------------------------------------------------
def make_rows(P, dead, seed=0, K=9):
    """Six float32 arrays in model order; `dead` bool [P].  Alive opacities in [0.02, 0.99], dead ones in [0.0005, 0.004]: none
    near the threshold 0.005.  features_rest is nonzero everywhere, so a row copy that misses a column shows."""
    rng = np.random.default_rng(seed)
    dead = np.asarray(dead, dtype=bool)
    o = np.where(dead, rng.uniform(0.0005, 0.004, P), rng.uniform(0.02, 0.99, P))
    rest = rng.uniform(0.1, 1.0, (P, K // 3, 3)) * rng.choice([-1.0, 1.0], (P, K // 3, 3))
    f = np.float32
    return [rng.normal(0, 1, (P, 3)).astype(f), rng.normal(0, 1, (P, 1, 3)).astype(f), rest.astype(f),
            np.log(rng.uniform(0.01, 0.1, (P, 3))).astype(f), rng.normal(0, 1, (P, 4)).astype(f), np.log(o / (1 - o)).reshape(P, 1).astype(f)]


def random_dead(P, share, seed):
    return np.random.default_rng(1000 + seed).random(P) < share


def pattern_dead(P=300):
    d = np.zeros(P, dtype=bool)
    d[0:10], d[100:150], d[P - 10:P] = True, True, True
    return d


U64_MAX = (1 << 64) - 1


def relocation_cases(sizes=(1, 63, 64, 65, 1023, 1024, 1025, 2049, 70000)):
    """-> list of (name, dead bool [P], draws or None).  draws: Python integers by dead rank."""
    cases = [(f"P{P}", random_dead(P, 0.1 if P > 1 else 0.0, P), None) for P in sizes]
    cases.append(("no_dead", np.zeros(500, dtype=bool), None))
    cases.append(("all_dead", np.ones(130, dtype=bool), None))
    one = np.ones(201, dtype=bool)
    one[77] = False
    cases.append(("one_alive_200_dead", one, None))
    cases.append(("runs", pattern_dead(), None))
    n = int(pattern_dead().sum())
    cases.append(("runs_draw_ends", pattern_dead(), [0 if j % 2 == 0 else U64_MAX for j in range(n)]))
    return cases
