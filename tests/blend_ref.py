"""The per-tile alpha blend restated in numpy -- TEST INFRASTRUCTURE, the reference of tests/test_gpu_blend_edges.py.

The sequential algorithm of oracle/tile_ref.c on 2D records and tile lists, nothing culled: per pixel, in list order,
skip when power > 0, alpha = min(0.99, opacity exp(power)), skip when alpha < 1/255, stop WITHOUT blending when
T (1 - alpha) < 1e-4.  Vectorised over the 256 pixels of a tile, looped over the list.

  records  [P, >= 10]  x, y, conic xx, xy, yy, opacity, r, g, b, depth  (the first ten floats of the device's 64-byte record;
                       columns 10, 11, where present, are its bounding-box half-extents)
  lists    one index array per tile: segment 1 followed by segment 2 (tile_lists)

dtype=float64 is the reference.  dtype=float32 rounds once per operation in the kernels' operation order (the exponent as
blend_power() forms it, the reverse step and the Bw recurrence as bwd_eval() does; a fused multiply-add is one rounding of
the exact product-sum): the noise yardstick the GPU bounds are derived from.
"""
import numpy as np

TILE = 16
ALPHA_MAX, ALPHA_MIN_DEN, T_EPS = 0.99, 255.0, 1e-4
SEAMS = (63, 64, 127, 128, 255, 256)       # list positions next to a 64-entry mask word / a staged-chunk boundary
# scratch-row columns: conic xx, xy, yy, depth | mean2D x, y | colour r, g, b | opacity
COLS = ("conic_xx", "conic_xy", "conic_yy", "depth", "mean_x", "mean_y", "col_r", "col_g", "col_b", "opacity")


def tile_lists(point_list, ranges, point_list2=None, ranges2=None):
    """-> (lists, len1): per tile the Gaussian indices of segment 1 + segment 2, and the length of segment 1.  Empty
    ranges may be stored as (0xFFFFFFFF, 0)."""
    pl = np.asarray(point_list).astype(np.int64)
    pl2 = pl if point_list2 is None else np.asarray(point_list2).astype(np.int64)
    r1 = np.asarray(ranges).astype(np.int64) & 0xFFFFFFFF
    r2 = None if ranges2 is None else np.asarray(ranges2).astype(np.int64) & 0xFFFFFFFF
    lists, len1 = [], []
    for t in range(len(r1)):
        a, b = (int(r1[t, 0]), int(r1[t, 1])) if r1[t, 1] > r1[t, 0] else (0, 0)
        seg = pl[a:b]
        if r2 is not None and r2[t, 1] > r2[t, 0]:
            seg = np.concatenate([seg, pl2[int(r2[t, 0]):int(r2[t, 1])]])
        lists.append(seg)
        len1.append(b - a)
    return lists, np.asarray(len1, dtype=np.int64)


def _fma(a, b, c, dtype):
    if dtype == np.float64:
        return a * b + c
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _tile_pixels(t, gx, W, H):
    tx, ty = t % gx, t // gx
    k = np.arange(TILE * TILE)
    px, py = tx * TILE + k % TILE, ty * TILE + k // TILE
    quad = (k % TILE >= 8).astype(np.int64) + 2 * (k // TILE >= 8).astype(np.int64)
    return px, py, (px < W) & (py < H), quad


def _eval(r, fpx, fpy, dtype):
    """One record against the tile's pixels: dx, dy, power, G, opacity * G, alpha, footprint-live."""
    f = dtype
    dx, dy = r[0] - fpx, r[1] - fpy
    q = _fma(r[4] * dy, dy, (r[2] * dx) * dx, f)
    power = _fma(-r[3] * dx, dy, f(-0.5) * q, f)
    G = np.exp(power)
    a_raw = r[5] * G
    alpha = np.minimum(f(ALPHA_MAX), a_raw)
    live = ~(power > 0) & ~(alpha < f(1.0) / f(ALPHA_MIN_DEN))
    return dx, dy, power, G, a_raw, alpha, live


class State:
    """What forward() found.  Images [.., H, W]; per tile t: ids[t] (the list), alive[t] / blended[t] [L, 256] (footprint
    reaches the pixel / blended into it), clamp[t] [L, 256] (opacity exp(power) >= 0.99 where blended)."""


def forward(records, lists, W, H, bg, dtype=np.float64):
    f = np.dtype(dtype).type
    R = np.asarray(records)[:, :10].astype(f)
    bgv = np.asarray(bg).astype(f)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    st = State()
    st.records, st.lists, st.W, st.H, st.bg, st.dtype, st.grid = np.asarray(records), lists, W, H, bgv, f, (gx, gy)
    st.color, st.depth, st.alpha = np.zeros((3, H, W), f), np.zeros((H, W), f), np.zeros((H, W), f)
    st.final_T, st.n_contrib = np.ones((H, W), f), np.zeros((H, W), np.int64)
    st.sat_pos = np.full((H, W), -1, np.int64)          # list position of the entry that saturated the pixel
    st.margin = np.full((H, W), np.inf)
    st.work = np.zeros(gx * gy, np.int64)
    st.ids, st.alive, st.blended, st.clamp = [], [], [], []
    for t in range(gx * gy):
        ids = np.asarray(lists[t], np.int64)
        L = len(ids)
        px, py, inside, _q = _tile_pixels(t, gx, W, H)
        fpx, fpy = px.astype(f), py.astype(f)
        T, active = np.ones(256, f), inside.copy()
        C, Dp, Ac = np.zeros((3, 256), f), np.zeros(256, f), np.zeros(256, f)
        last, sat, margin = np.zeros(256, np.int64), np.full(256, -1, np.int64), np.full(256, np.inf)
        alive, blended, clamp = np.zeros((L, 256), bool), np.zeros((L, 256), bool), np.zeros((L, 256), bool)
        for k in range(L):
            r = R[ids[k]]
            _dx, _dy, power, _G, a_raw, alpha, fp = _eval(r, fpx, fpy, f)
            alive[k] = fp & inside
            if not active.any():
                continue
            live = fp & active
            test_T = T * (f(1.0) - np.where(live, alpha, f(0.0)))
            stop = live & (test_T < f(T_EPS))
            blend = live & ~stop
            if f is np.float64:
                m = np.abs(a_raw * ALPHA_MIN_DEN - 1.0)
                m = np.where(live, np.minimum(m, np.abs(test_T / T_EPS - 1.0)), m)
                margin = np.where(active, np.minimum(margin, m), margin)
            w = np.where(blend, alpha * T, f(0.0))
            for ch in range(3):
                C[ch] = _fma(r[6 + ch], w, C[ch], f)
            Dp = _fma(r[9], w, Dp, f)
            Ac = Ac + w
            T = np.where(blend, test_T, T)
            last = np.where(blend, k + 1, last)
            sat = np.where(stop, k, sat)
            blended[k] = blend
            clamp[k] = blend & (a_raw >= f(ALPHA_MAX))
            active = active & ~stop
        yy, xx = py[inside], px[inside]
        for ch in range(3):
            st.color[ch, yy, xx] = _fma(T, bgv[ch], C[ch], f)[inside]
        st.depth[yy, xx], st.alpha[yy, xx] = Dp[inside], Ac[inside]
        st.final_T[yy, xx], st.n_contrib[yy, xx] = T[inside], last[inside]
        st.sat_pos[yy, xx], st.margin[yy, xx] = sat[inside], margin[inside]
        st.work[t] = int(last.max())
        st.ids.append(ids); st.alive.append(alive); st.blended.append(blended); st.clamp.append(clamp)
    return st


def backward(st, gc, gd=None, ga=None):
    """Per-Gaussian sums of the blend backward for pixel gradients gc [3, H, W], gd, ga [H, W] (None = zeros): float64
    [P, 10] in the scratch row's column order and units (mean2D columns scaled by 0.5 W, 0.5 H; background term included).
    Walks every pixel's list backwards from its n_contrib, in st.dtype."""
    f = st.dtype
    W, H, (gx, gy) = st.W, st.H, st.grid
    R = np.asarray(st.records)[:, :10].astype(f)
    P = R.shape[0]
    gc = np.asarray(gc).reshape(3, H, W).astype(f)
    gd = np.zeros((H, W), f) if gd is None else np.asarray(gd).reshape(H, W).astype(f)
    ga = np.zeros((H, W), f) if ga is None else np.asarray(ga).reshape(H, W).astype(f)
    rows = np.zeros((P, 10), f)
    half_w, half_h = f(0.5) * f(W), f(0.5) * f(H)
    for t in range(gx * gy):
        ids, blended = st.ids[t], st.blended[t]
        if len(ids) == 0 or not blended.any():
            continue
        px, py, inside, quad = _tile_pixels(t, gx, W, H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        z = lambda a: np.where(inside, a[cy, cx], f(0.0)).astype(f)  # noqa: E731
        dCr, dCg, dCb, dD, dA = z(gc[0]), z(gc[1]), z(gc[2]), z(gd), z(ga)
        T_final = z(st.final_T)
        bg_dot = (st.bg[0] * dCr + st.bg[1] * dCg) + st.bg[2] * dCb
        fpx, fpy = px.astype(f), py.astype(f)
        T, Bw = T_final.copy(), np.zeros(256, f)
        deepest = int(np.nonzero(blended.any(1))[0].max())
        for k in range(deepest, -1, -1):
            live = blended[k]
            if not live.any():
                continue
            r = R[ids[k]]
            dx, dy, _p, G, _a, alpha, _fp = _eval(r, fpx, fpy, f)
            G, alpha = np.where(live, G, f(0.0)), np.where(live, alpha, f(0.0))
            inv = f(1.0) / (f(1.0) - alpha)
            T = T * inv
            wgt = alpha * T
            cw = r[6] * dCr
            cw = _fma(r[7], dCg, cw, f)
            cw = _fma(r[8], dCb, cw, f)
            cw = _fma(r[9], dD, cw, f)
            cw = cw + dA
            diff = cw - Bw
            Bw = _fma(alpha, diff, Bw, f)
            dL_da = _fma(-T_final * inv, bg_dot, diff * T, f)
            s = G * (r[5] * dL_da)
            u, v, nw = r[2] * dx, r[4] * dy, -r[3] * dx
            sh = f(-0.5) * s
            shx = sh * dx
            p = np.stack([shx * dx, shx * dy, (sh * dy) * dy, wgt * dD,
                          (s * half_w) * -_fma(r[3], dy, u, f), (s * half_h) * (nw - v),
                          wgt * dCr, wgt * dCg, wgt * dCb, G * dL_da])
            if f is np.float64:
                rows[ids[k]] += p.sum(1)
            else:   # one sum per quadrant, then one add per (quadrant, Gaussian), as the kernels' atomics
                for q in range(4):
                    if live[quad == q].any():
                        rows[ids[k]] = rows[ids[k]] + p[:, quad == q].sum(1, dtype=np.float32)
    return rows.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# strata, all from a float64 State
# ---------------------------------------------------------------------------------------------------------------------
def extents(records):
    """Bounding-box half-extents of the alpha >= 1/255 footprint: columns 10, 11 of a device record, else restated from
    conic and opacity (sqrt(2 ln(255 opacity) cov) 1.001 + 0.05; no footprint below opacity 0.0039)."""
    r = np.asarray(records, np.float64)
    if r.shape[1] >= 12:
        return r[:, 10], r[:, 11]
    with np.errstate(all="ignore"):          # (rows of Gaussians outside every list hold nothing)
        det = r[:, 2] * r[:, 4] - r[:, 3] ** 2
        a, c = r[:, 4] / det, r[:, 2] / det
        tau2 = 2.0 * np.log(np.maximum(255.0 * r[:, 5], 1.0))
        ok = r[:, 5] >= 0.0039
        return (np.where(ok, np.sqrt(tau2 * a) * 1.001 + 0.05, -1e30), np.where(ok, np.sqrt(tau2 * c) * 1.001 + 0.05, -1e30))


def pairs(st, fragile_margin):
    """One row per (tile, list position, quadrant): dict of flat arrays
       gid, tile, pos, quad | n_alive (footprint-live pixels inside the image), n_blend (pixels it was blended into),
       n_solid (of those, the non-fragile ones) | reach (bounding box reaches the quadrant) | walked (pos below the
       quadrant's deepest n_contrib: the backward evaluates it unless culled) | near (some pixel of the quadrant has this
       Gaussian's opacity exp(power) within fragile_margin of 1/255) | finish (the position after which no pixel of the
       quadrant is active; list length if some pixel never saturates)."""
    W, H, (gx, gy) = st.W, st.H, st.grid
    R = np.asarray(st.records, np.float64)
    ex, ey = extents(st.records)
    out = {k: [] for k in ("gid", "tile", "pos", "quad", "n_alive", "n_blend", "n_solid", "reach", "walked", "near", "finish")}
    for t in range(gx * gy):
        ids = st.ids[t]
        L = len(ids)
        if L == 0:
            continue
        px, py, inside, quad = _tile_pixels(t, gx, W, H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        solid = inside & (st.margin[cy, cx] >= fragile_margin)
        last = np.where(inside, st.n_contrib[cy, cx], 0)
        sat = np.where(inside, st.sat_pos[cy, cx], -1)
        tx, ty = (t % gx) * TILE, (t // gx) * TILE
        fpx, fpy = px.astype(np.float64), py.astype(np.float64)
        r = R[ids]
        dx, dy = r[:, 0:1] - fpx, r[:, 1:2] - fpy
        a_raw = r[:, 5:6] * np.exp(-0.5 * (r[:, 2:3] * dx * dx + r[:, 4:5] * dy * dy) - r[:, 3:4] * dx * dy)
        nearpix = (np.abs(a_raw * ALPHA_MIN_DEN - 1.0) < fragile_margin) & inside
        for q in range(4):
            m = quad == q
            qin = inside & m
            x0, y0 = tx + 8 * (q & 1), ty + 8 * (q >> 1)
            reach = ((r[:, 0] - ex[ids] <= x0 + 7) & (r[:, 0] + ex[ids] >= x0) &
                     (r[:, 1] - ey[ids] <= y0 + 7) & (r[:, 1] + ey[ids] >= y0))
            if not qin.any():
                finish = 0
            elif (sat[qin] < 0).any():
                finish = L
            else:
                finish = int(sat[qin].max())
            out["gid"].append(ids); out["tile"].append(np.full(L, t)); out["pos"].append(np.arange(L))
            out["quad"].append(np.full(L, q)); out["n_alive"].append(st.alive[t][:, m].sum(1))
            out["n_blend"].append(st.blended[t][:, m].sum(1))
            out["n_solid"].append((st.blended[t][:, m] & solid[m]).sum(1))
            out["reach"].append(reach); out["walked"].append(np.arange(L) < int(last[m].max()))
            out["near"].append(nearpix[:, m].any(1)); out["finish"].append(np.full(L, finish))
    return {k: (np.concatenate(v) if v else np.zeros(0, np.int64)) for k, v in out.items()}


def strata(st, fragile_margin):
    """-> (masks, lost, pr).  masks: per-Gaussian boolean [P] for every stratum; lost: the same members that fragility
    takes out of the comparison (every pixel that made them a member is fragile, or -- cullable -- the Gaussian is within
    the margin of being live there); pr = pairs().

      cullable     a (tile, quadrant) the bounding box reaches and the backward walks, with 0 live pixels
      corner       1-3 pixels blended in a quadrant
      seam         sits at list position 63, 64, 127, 128, 255 or 256 and is blended into at least one pixel
      sat_at_seam  blended into a pixel whose saturating entry or last contributor is at one of those positions
      late         evaluated by a quadrant 1-3 candidates after its last pixel finished (candidates: footprint-live entries)
      clamped      opacity exp(power) >= 0.99 at a pixel it is blended into
      faint        opacity < 2/255, blended somewhere"""
    P = np.asarray(st.records).shape[0]
    W, H, (gx, gy) = st.W, st.H, st.grid
    pr = pairs(st, fragile_margin)
    seam_pos = np.isin(pr["pos"], SEAMS)
    sel = dict(cullable=pr["reach"] & pr["walked"] & (pr["n_alive"] == 0),
               corner=(pr["n_blend"] >= 1) & (pr["n_blend"] <= 3),
               seam=seam_pos & (pr["n_blend"] >= 1))
    gone = dict(cullable=pr["near"], corner=pr["n_solid"] == 0, seam=pr["n_solid"] == 0)
    # late: per quadrant, the first three footprint-live entries behind its finish position
    cand = pr["n_alive"] > 0
    behind = cand & (pr["pos"] > pr["finish"])
    late = np.zeros(len(cand), bool)
    key = (pr["tile"] * 4 + pr["quad"])
    for kq in np.unique(key[behind]):
        idx = np.nonzero(behind & (key == kq))[0]
        late[idx[np.argsort(pr["pos"][idx])][:3]] = True
    sel["late"], gone["late"] = late, np.zeros(len(cand), bool)
    masks, lost = {}, {}
    for k in sel:
        masks[k] = np.zeros(P, bool); masks[k][pr["gid"][sel[k]]] = True
        keep = np.zeros(P, bool); keep[pr["gid"][sel[k] & ~gone[k]]] = True
        lost[k] = masks[k] & ~keep
    # per pixel: sat_at_seam; per (entry, pixel): clamped
    for k in ("sat_at_seam", "clamped", "faint"):
        masks[k], lost[k] = np.zeros(P, bool), np.zeros(P, bool)
    keep_sat, keep_cl, keep_faint = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool)
    sat_pix = np.isin(st.sat_pos, SEAMS) | np.isin(st.n_contrib - 1, SEAMS)
    st.sat_at_seam = sat_pix
    op = np.asarray(st.records, np.float64)[:, 5]
    for t in range(gx * gy):
        ids = st.ids[t]
        if len(ids) == 0:
            continue
        px, py, inside, _q = _tile_pixels(t, gx, W, H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        solid = inside & (st.margin[cy, cx] >= fragile_margin)
        sp = inside & sat_pix[cy, cx]
        b = st.blended[t]
        masks["sat_at_seam"][ids[(b & sp).any(1)]] = True
        keep_sat[ids[(b & sp & solid).any(1)]] = True
        masks["clamped"][ids[st.clamp[t].any(1)]] = True
        keep_cl[ids[(st.clamp[t] & solid).any(1)]] = True
        f_ = op[ids] < 2.0 / 255.0
        masks["faint"][ids[f_ & b.any(1)]] = True
        keep_faint[ids[f_ & (b & solid).any(1)]] = True
    lost["sat_at_seam"], lost["clamped"] = masks["sat_at_seam"] & ~keep_sat, masks["clamped"] & ~keep_cl
    lost["faint"] = masks["faint"] & ~keep_faint
    return masks, lost, pr


def touched_rows(st, fragile_margin):
    """[P] bool: blended into at least one non-fragile pixel (every other Gaussian's row must be exactly zero when the
    pixel gradients are zeroed at the fragile pixels)."""
    P = np.asarray(st.records).shape[0]
    W, H, (gx, gy) = st.W, st.H, st.grid
    out = np.zeros(P, bool)
    for t in range(gx * gy):
        if len(st.ids[t]) == 0:
            continue
        px, py, inside, _q = _tile_pixels(t, gx, W, H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        solid = inside & (st.margin[cy, cx] >= fragile_margin)
        out[st.ids[t][(st.blended[t] & solid).any(1)]] = True
    return out


def tile_solid(st, fragile_margin):
    """[tiles] bool: every pixel of the tile is non-fragile."""
    W, H, (gx, gy) = st.W, st.H, st.grid
    out = np.zeros(gx * gy, bool)
    for t in range(gx * gy):
        px, py, inside, _q = _tile_pixels(t, gx, W, H)
        out[t] = bool((st.margin[py[inside], px[inside]] >= fragile_margin).all())
    return out
