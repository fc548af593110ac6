"""The yardstick of the plane-sweep matcher (csrc/sweep.hip): a plain numpy restatement of the
algorithm, statement by statement, in ONE arithmetic type T -- float64 (the yardstick) or float32 (the same operations in the
same order; no fused multiply-add anywhere: numpy has none).  Both read the same float32 homographies, so their difference is
the rounding of the arithmetic alone; the maker stores its largest value over all valid scores as `err32`.

Also here: the synthetic scene of golden G16 (tests/golden/sweep.npz) -- pinhole cameras on a short baseline looking at a
slanted textured plane with a nearer plane in front of part of it -- whose images, correspondences and depths are analytic.

    gray(img)                       integer luma (77 R + 150 G + 29 B + 128) >> 8
    node_axes(W, H, stride)         x = 3 + i stride <= W - 4, y = 3 + j stride <= H - 4; node n = j * nx + i
    plan(K, w2c_a, w2c_b, ...)      float64 -> float32: D homographies, the map of the consistency check, 1/far, the step
    score_volume(...)               [D, N] ZNCC and validity
    select(...)                     best / uniqueness / parabola per node
    consistency(...)                the left/right check of one direction
    match_pair(...)                 both directions of a view pair
"""
from typing import NamedTuple

import numpy as np

R = 3
TAPS = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]          # row-major: the order of every sum
NONE = -1.0
NEAR_TIE = 1e-4                                                                    # scores closer than this may order differently in float32
EDGE_TIE = 1e-4                                                                    # pixels: a tap this close to the frame's edge may fall on either side


class Params(NamedTuple):
    stride: int = 2
    hypotheses: int = 128
    min_score: float = 0.8
    margin: float = 0.05
    min_var: float = 4.0
    cyc_steps: float = 1.5


def gray(img: np.ndarray) -> np.ndarray:
    c = img.astype(np.int32)
    return ((77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8).astype(np.uint8)


def node_axes(W: int, H: int, stride: int):
    return np.arange(R, W - R, stride), np.arange(R, H - R, stride)


class Plan(NamedTuple):
    homographies: np.ndarray       # float32 [D,3,3]  a -> b, plane k of a
    proj: np.ndarray               # float32 [12]     K R K^-1 (9, row-major) and K t (3)
    inv_far: np.float32
    step: np.float32


def plan(K, w2c_a, w2c_b, near: float, far: float, D: int) -> Plan:
    K = np.asarray(K, np.float64)
    rel = np.asarray(w2c_b, np.float64) @ np.linalg.inv(np.asarray(w2c_a, np.float64))
    Rm, t = rel[:3, :3], rel[:3, 3]
    Kinv = np.linalg.inv(K)
    inv_far, step = 1.0 / far, (1.0 / near - 1.0 / far) / (D - 1)
    n = np.array([0.0, 0.0, 1.0])
    hs = np.stack([K @ (Rm + np.outer(t, n) * (inv_far + step * k)) @ Kinv for k in range(D)])
    proj = np.concatenate([(K @ Rm @ Kinv).ravel(), K @ t])
    return Plan(hs.astype(np.float32), proj.astype(np.float32), np.float32(inv_far), np.float32(step))


class Volume(NamedTuple):
    scores: np.ndarray             # [D,N] T
    valid: np.ndarray              # [D,N] bool
    va: np.ndarray                 # [N] T: sum of squares of the node's own centred patch
    edge: np.ndarray               # [D,N] float64: smallest distance of any tap to a validity boundary (pixels / w units)


def score_volume(gray_a, gray_b, homographies, stride: int, T) -> Volume:
    H, W = gray_a.shape
    xs, ys = node_axes(W, H, stride)
    X, Y = np.meshgrid(xs, ys)
    X, Y = X.ravel(), Y.ravel()
    N = len(X)
    ga, gb = gray_a.astype(T), gray_b.astype(T).ravel()
    px, py = X.astype(T), Y.astype(T)
    n49, one = T(len(TAPS)), T(1)
    a = [ga[Y + dy, X + dx] for dy, dx in TAPS]
    sa = np.zeros(N, T)
    for v in a:
        sa = sa + v
    ma = sa / n49
    da = [v - ma for v in a]
    va = np.zeros(N, T)
    for v in da:
        va = va + v * v
    D = len(homographies)
    scores, valid, edge = np.zeros((D, N), T), np.zeros((D, N), bool), np.full((D, N), np.inf)
    wm, hm = T(W - 1), T(H - 1)
    for k in range(D):
        h = homographies[k].astype(T).ravel()
        ok = np.ones(N, bool)
        sb, sbb, cov = np.zeros(N, T), np.zeros(N, T), np.zeros(N, T)
        for i, (dy, dx) in enumerate(TAPS):
            x, y = px + T(dx), py + T(dy)
            hx = (h[0] * x + h[1] * y) + h[2]
            hy = (h[3] * x + h[4] * y) + h[5]
            hw = (h[6] * x + h[7] * y) + h[8]
            front = hw > 0
            r = one / np.where(front, hw, one)
            u, v = hx * r, hy * r
            good = front & (u >= 0) & (u <= wm) & (v >= 0) & (v <= hm)
            with np.errstate(invalid="ignore"):
                dist = np.minimum.reduce([np.abs(u), np.abs(wm - u), np.abs(v), np.abs(hm - v)]).astype(np.float64)
            edge[k] = np.minimum(edge[k], np.where(front, dist, np.inf))
            edge[k] = np.minimum(edge[k], np.abs(hw).astype(np.float64) * 1e2)     # |w| < 1e-6 is as fragile as 1e-4 px
            ok &= good
            u, v = np.where(good, u, T(0)), np.where(good, v, T(0))
            x0, y0 = np.minimum(np.floor(u), T(W - 2)), np.minimum(np.floor(v), T(H - 2))
            fx, fy = u - x0, v - y0
            at = y0.astype(np.int64) * W + x0.astype(np.int64)
            top = gb[at] * (one - fx) + gb[at + 1] * fx
            bot = gb[at + W] * (one - fx) + gb[at + W + 1] * fx
            b = (top * (one - fy) + bot * fy) - ma
            sb = sb + b
            sbb = sbb + b * b
            cov = cov + da[i] * b
        vb = sbb - (sb * sb) / n49
        den = va * vb
        pos = den > T(1e-6)
        scores[k] = np.where(pos, cov / np.sqrt(np.where(pos, den, one)), T(0))
        valid[k] = ok
    return Volume(scores, valid, va, edge)


class Selection(NamedTuple):
    has: np.ndarray                # [N] bool
    k: np.ndarray                  # [N] int: best hypothesis (meaningful where any hypothesis is valid)
    best: np.ndarray               # [N] T
    second: np.ndarray             # [N] T: best valid score outside k +- 1 (-inf: none)
    lcr: np.ndarray                # [3,N] T: scores at k - 1, k, k + 1 (nan where not available)
    refined: np.ndarray            # [N] bool
    invd: np.ndarray               # [N] T, NONE where not has
    fragile: np.ndarray            # [N] bool: a decision of this node lies within NEAR_TIE / EDGE_TIE of its threshold


def select(vol: Volume, p: Params, inv_far, step, T) -> Selection:
    D, N = vol.scores.shape
    idx = np.arange(N)
    s = np.where(vol.valid, vol.scores, T(-np.inf))
    k = np.argmax(s, axis=0)
    best = s[k, idx]
    textured = vol.va / T(len(TAPS)) >= T(p.min_var)
    anyv = vol.valid.any(axis=0)
    outside = vol.valid & (np.abs(np.arange(D)[:, None] - k[None, :]) > 1)
    second = np.where(outside, vol.scores, T(-np.inf)).max(axis=0)
    unique = ~(second > best - T(p.margin))
    has = textured & anyv & (best >= T(p.min_score)) & unique
    kl, kr = np.clip(k - 1, 0, D - 1), np.clip(k + 1, 0, D - 1)
    can = (k > 0) & (k < D - 1) & vol.valid[kl, idx] & vol.valid[kr, idx]
    l, c, r = vol.scores[kl, idx], vol.scores[k, idx], vol.scores[kr, idx]
    denom = (l - T(2) * c) + r
    refined = can & (denom < 0)
    off = np.where(refined, (T(0.5) * (l - r)) / np.where(refined, denom, T(1)), T(0))
    invd = T(inv_far) + T(step) * (k.astype(T) + off)
    # near-ties: any decision that float32 rounding may take the other way
    srt = np.sort(s, axis=0)
    with np.errstate(invalid="ignore"):
        top_two = (srt[-1] - srt[-2] < NEAR_TIE) if D > 1 else np.zeros(N, bool)
        fragile = (top_two | (np.abs(best - p.min_score) < NEAR_TIE) | (np.abs(second - (best - p.margin)) < NEAR_TIE)
                   | (np.abs(vol.va / len(TAPS) - p.min_var) < 1e-3) | (vol.edge < EDGE_TIE).any(axis=0))
        fragile |= refined & (np.abs(denom) < 4 * NEAR_TIE)                        # a vertex that rounding can move by a step
        fragile |= can & ~refined & (np.abs(denom) < NEAR_TIE)
    nan = T(np.nan)
    return Selection(has, k, best, second, np.stack([np.where(can, l, nan), c, np.where(can, r, nan)]), refined,
                     np.where(has, invd, T(NONE)), fragile)


class Direction(NamedTuple):
    keep: np.ndarray               # [N] bool
    q: np.ndarray                  # [N,2] T: the node's correspondence in the other view (nan where the node has no value)
    partner: np.ndarray            # [N] int: nearest node of the other view, -1 when outside its node grid
    fragile: np.ndarray            # [N] bool


def consistency(sel_a: Selection, sel_b: Selection, proj, W: int, H: int, p: Params, step, T) -> Direction:
    xs, ys = node_axes(W, H, p.stride)
    nx, ny = len(xs), len(ys)
    X, Y = np.meshgrid(xs, ys)
    x, y = X.ravel().astype(T), Y.ravel().astype(T)
    m = np.asarray(proj).astype(T)
    invd = np.where(sel_a.has, sel_a.invd, T(1))
    hx = ((m[0] * x + m[1] * y) + m[2]) + m[9] * invd
    hy = ((m[3] * x + m[4] * y) + m[5]) + m[10] * invd
    hw = ((m[6] * x + m[7] * y) + m[8]) + m[11] * invd
    front = hw > 0
    r = T(1) / np.where(front, hw, T(1))
    qx, qy, inb = hx * r, hy * r, invd * r
    fi, fj = (qx - T(R)) / T(p.stride), (qy - T(R)) / T(p.stride)
    i, j = np.rint(fi), np.rint(fj)
    inside = front & (i >= 0) & (i <= nx - 1) & (j >= 0) & (j <= ny - 1)
    nb = np.where(inside, j * nx + i, 0).astype(np.int64)
    tol = T(p.cyc_steps) * T(step)
    diff = np.abs(sel_b.invd[nb] - inb)
    keep = sel_a.has & inside & sel_b.has[nb] & (diff <= tol)
    half = lambda f: np.abs(np.abs(f - np.floor(f)) - 0.5) < EDGE_TIE  # noqa: E731
    fragile = sel_a.fragile | (sel_a.has & (half(fi) | half(fj) | (inside & sel_b.fragile[nb])
                                            | (inside & sel_b.has[nb] & (np.abs(diff - tol) < 1e-3 * tol))))
    q = np.stack([np.where(sel_a.has, qx, T(np.nan)), np.where(sel_a.has, qy, T(np.nan))], axis=1)
    return Direction(keep, q, np.where(inside & sel_a.has, nb, -1), fragile)


class PairResult(NamedTuple):
    sel: tuple                     # (Selection of a, Selection of b)
    dirs: tuple                    # (Direction a -> b, Direction b -> a)
    vols: tuple


def match_pair(img_a, img_b, K, w2c_a, w2c_b, near: float, far: float, p: Params, T=np.float64) -> PairResult:
    ga, gb = gray(np.asarray(img_a)), gray(np.asarray(img_b))
    H, W = ga.shape
    pab, pba = plan(K, w2c_a, w2c_b, near, far, p.hypotheses), plan(K, w2c_b, w2c_a, near, far, p.hypotheses)
    va, vb = score_volume(ga, gb, pab.homographies, p.stride, T), score_volume(gb, ga, pba.homographies, p.stride, T)
    sa, sb = select(va, p, pab.inv_far, pab.step, T), select(vb, p, pba.inv_far, pba.step, T)
    dab = consistency(sa, sb, pab.proj, W, H, p, pab.step, T)
    dba = consistency(sb, sa, pba.proj, W, H, p, pba.step, T)
    return PairResult((sa, sb), (dab, dba), (va, vb))


def keypoints(W: int, H: int, stride: int, d: Direction):
    """-> (kp_source [n,2], kp_target [n,2]) float32 of the kept nodes, in node order"""
    xs, ys = node_axes(W, H, stride)
    X, Y = np.meshgrid(xs, ys)
    src = np.stack([X.ravel(), Y.ravel()], axis=1).astype(np.float32)
    return src[d.keep], d.q[d.keep].astype(np.float32)


# ---- the synthetic scene ---------------------------------------------------------------------------------------------------
class Scene(NamedTuple):
    W: int
    H: int
    K: np.ndarray                  # [3,3] float64
    c2ws: np.ndarray               # [V,4,4] float64
    back: np.ndarray               # plane n . X = d as (nx, ny, nz, d): the slanted background
    front: np.ndarray              # the nearer plane ...
    front_box: tuple               # ... which exists for x0 <= X <= x1, y0 <= Y <= y1 (world)
    stripe_box: tuple              # world x / y range of the periodic stripes on the background
    stripe_period: float
    waves: np.ndarray              # [n,3,4]: per sinusoid and channel (kx, ky, phase, amplitude)
    near: float
    far: float


def _rot(yaw: float, pitch: float) -> np.ndarray:
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])


def make_scene(W: int = 96, H: int = 72, seed: int = 7, baseline: float = 0.6, n_views: int = 3, toe_in: bool = False) -> Scene:
    """toe_in: every camera looks at the middle of the background (a long baseline keeps its overlap)"""
    rng = np.random.default_rng(seed)
    f = 100.0 * W / 96.0
    K = np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1.0]])
    spots = [(-0.5, 0.0), (0.5, 0.0), (0.0, 0.85), (0.0, -0.7)]                    # a triangle (and a spare): three baselines of one length
    c2ws = []
    for v in range(n_views):
        m = np.eye(4)
        m[:3, :3] = _rot(0.012 * (v - 1), 0.008 * (1 - v))
        m[:3, 3] = [spots[v][0] * baseline, spots[v][1] * baseline, 0.02 * v]
        if toe_in:
            fwd = np.array([0.0, 0.0, 4.0]) - m[:3, 3]
            fwd /= np.linalg.norm(fwd)
            right = np.cross([0.0, 1.0, 0.0], fwd)
            right /= np.linalg.norm(right)
            m[:3, :3] = np.stack([right, np.cross(fwd, right), fwd], axis=1) @ m[:3, :3]
        c2ws.append(m)
    waves = []
    for period in (0.16, 0.23, 0.31, 0.45, 0.7, 1.1):                              # world units: 4 .. 28 pixels at depth 4
        ang = rng.uniform(0, np.pi)
        kx, ky = 2 * np.pi / period * np.cos(ang), 2 * np.pi / period * np.sin(ang)
        waves.append([[kx, ky, rng.uniform(0, 2 * np.pi), rng.uniform(14, 24)] for _ in range(3)])
    return Scene(W, H, K, np.stack(c2ws), np.array([-0.06, -0.03, 1.0, 4.0]), np.array([0.04, 0.0, 1.0, 2.6]),
                 (-2.0, -0.35, -0.45, 0.45), (-0.1, 1.5, -0.95, 0.95), 0.32, np.array(waves), 1.6, 6.5)


def _texture(sc: Scene, X: np.ndarray, on_front: np.ndarray) -> np.ndarray:
    x, y = X[..., 0], X[..., 1]
    x, y = np.where(on_front, 1.54 * x + 10.0, x), np.where(on_front, 1.54 * y, y)  # another part of the texture, the same periods in pixels
    out = np.full(X.shape[:-1] + (3,), 128.0)
    for wv in sc.waves:
        for ch in range(3):
            kx, ky, ph, amp = wv[ch]
            out[..., ch] += amp * np.sin(kx * x + ky * y + ph)
    sx0, sx1, sy0, sy1 = sc.stripe_box
    stripes = ~on_front & (X[..., 0] >= sx0) & (X[..., 0] <= sx1) & (X[..., 1] >= sy0) & (X[..., 1] <= sy1)
    s = 128.0 + 90.0 * np.sin(2 * np.pi / sc.stripe_period * X[..., 0])
    return np.where(stripes[..., None], s[..., None], out)


def cast(sc: Scene, view: int, u: np.ndarray, v: np.ndarray):
    """the surface seen at pixel (u, v) of a view -> (world point [...,3], depth z, on_front, striped)"""
    c2w = sc.c2ws[view]
    d_cam = np.stack([(u - sc.K[0, 2]) / sc.K[0, 0], (v - sc.K[1, 2]) / sc.K[1, 1], np.ones_like(u, dtype=np.float64)], axis=-1)
    d = d_cam @ c2w[:3, :3].T
    o = c2w[:3, 3]
    hit = {}
    for name, pl in (("back", sc.back), ("front", sc.front)):
        s = (pl[3] - pl[:3] @ o) / (d @ pl[:3])
        hit[name] = (s, o + s[..., None] * d)
    x0, x1, y0, y1 = sc.front_box
    sf, Xf = hit["front"]
    on_front = (sf > 0) & (Xf[..., 0] >= x0) & (Xf[..., 0] <= x1) & (Xf[..., 1] >= y0) & (Xf[..., 1] <= y1)
    z = np.where(on_front, sf, hit["back"][0])                                    # d_cam has z = 1: the ray parameter IS the depth
    X = np.where(on_front[..., None], Xf, hit["back"][1])
    sx0, sx1, sy0, sy1 = sc.stripe_box
    striped = ~on_front & (X[..., 0] >= sx0) & (X[..., 0] <= sx1) & (X[..., 1] >= sy0) & (X[..., 1] <= sy1)
    return X, z, on_front, striped


def render(sc: Scene, view: int) -> np.ndarray:
    v, u = np.meshgrid(np.arange(sc.H, dtype=np.float64), np.arange(sc.W, dtype=np.float64), indexing="ij")
    X, _, on_front, _ = cast(sc, view, u, v)
    return np.clip(np.round(_texture(sc, X, on_front)), 0, 255).astype(np.uint8)


def w2c(sc: Scene, view: int) -> np.ndarray:
    return np.linalg.inv(sc.c2ws[view])


STRIPE_MARGIN_Y = 0.6


class Truth(NamedTuple):
    q: np.ndarray                  # [N,2] the true correspondence of every node of a in b
    z: np.ndarray                  # [N] the node's true depth in a
    eligible: np.ndarray           # [N] textured surface, seen by b as well, the 7x7 patch inside b's frame
    striped: np.ndarray            # [N] the whole 7x7 patch lies in the striped region, more than a period from its left and right
                                   #     ends and STRIPE_MARGIN_Y from its top and bottom: the next stripe along ANY epipolar line of
                                   #     the rig is inside the region as well


def truth(sc: Scene, a: int, b: int, stride: int) -> Truth:
    xs, ys = node_axes(sc.W, sc.H, stride)
    Xg, Yg = np.meshgrid(xs.astype(np.float64), ys.astype(np.float64))
    u, v = Xg.ravel(), Yg.ravel()
    X, z, _, _ = cast(sc, a, u, v)
    m = w2c(sc, b)
    Xb = X @ m[:3, :3].T + m[:3, 3]
    q = np.stack([sc.K[0, 0] * Xb[:, 0] / Xb[:, 2] + sc.K[0, 2], sc.K[1, 1] * Xb[:, 1] / Xb[:, 2] + sc.K[1, 2]], axis=1)
    _, zb, _, _ = cast(sc, b, q[:, 0], q[:, 1])
    seen = np.abs(zb - Xb[:, 2]) < 1e-6
    inside = (q[:, 0] >= R + 1) & (q[:, 0] <= sc.W - 2 - R) & (q[:, 1] >= R + 1) & (q[:, 1] <= sc.H - 2 - R)
    all_striped, any_striped = np.ones(len(u), bool), np.zeros(len(u), bool)
    for dy, dx in TAPS:
        Xt, _, _, st = cast(sc, a, u + dx, v + dy)
        all_striped &= st & (Xt[:, 0] >= sc.stripe_box[0] + 1.25 * sc.stripe_period) & (Xt[:, 0] <= sc.stripe_box[1] - 1.25 * sc.stripe_period)
        all_striped &= (Xt[:, 1] >= sc.stripe_box[2] + STRIPE_MARGIN_Y) & (Xt[:, 1] <= sc.stripe_box[3] - STRIPE_MARGIN_Y)
        any_striped |= st
    return Truth(q, z, seen & inside & ~any_striped, all_striped)
