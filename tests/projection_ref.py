"""float64 numpy reference of the forward projection (csrc/preprocess.hip, preprocess_fwd_kernel), written from the
formulas of the published algorithm and of DESIGN.md -- independently of oracle/tile_ref.c and of the kernel; the SH basis
and the 3D covariance come from oracle/dense_torch.py.

project(...) -> dict of per-Gaussian arrays: what the kernel stores (pixel position, conic, radius, colour, clamp bits,
footprint half-extents, reference and tight rect) and, for every integer or boolean DECISION, a margin and a rounding scale:
  margin  the distance of the float64 quantity from the threshold at which the decision flips, in the units of the comparison
  scale   the size of the terms the quantity is summed from, so that eps32 * scale is one float32 rounding of it (0 where the
          float32 evaluation is exact: the decision is then never fragile)
A decision is FRAGILE when margin < FRAGILE_ULPS * EPS32 * scale.

Inputs are the float32 values the kernel receives (activated parameters, camera matrices, tan(fov/2), the scale modifier),
taken to float64 exactly; every operation behind that is float64.  KNOBS are the constants a mutation test changes on a COPY of
this module (tests/test_projection_ref_cpu.py)."""
import numpy as np
import torch

TILE = 16
EPS32 = float(np.finfo(np.float32).eps)           # 2^-23
NEAR = float(np.float32(0.2))
OP_GATE = float(np.float32(0.0039))
ALPHA_MIN = 1.0 / 255.0
# A decision within this many float32 roundings (EPS32 * scale) of its threshold may be taken either way by a float32
# implementation.  Measured by tests/test_projection_ref_cpu.py over every scene, camera, size and SH configuration of
# helpers.PROJ_*: oracle/tile_ref.c (float32) decides NONE of its ~330 000 integer and boolean decisions against this reference,
# so the multiple comes from how far its stored quantities really move, in the same `scale` units: the largest
# |float32 - float64| / (EPS32 * scale) is 0.84 (view depth; pixel position 0.45, colour 0.47).  4 x that, rounded up: 4.  The
# fragile set is then at most 0.09 % of the decisions of a view and at most one or two members of a stratum.
FRAGILE_ULPS = 4.0
# the slack the kernel adds to a half-extent on purpose (0.1 % + 0.05 px), as the widest the issue lets a stored extent be:
# a tight edge closer than this to a tile boundary may legitimately include one more tile than the exact extent asks for
EXT_SLACK_REL, EXT_SLACK_ABS = 0.002, 0.06

KNOBS = dict(near_strict=False, clamp=1.3, sh6_sign=1.0, upper_pad=float(TILE - 1), tau_factor=2.0)

DECISIONS = ("near", "clamp_x", "clamp_y", "radius", "x0", "y0", "x1", "y1", "ch0", "ch1", "ch2")
TIGHT_DECISIONS = ("tx0", "ty0", "tx1", "ty1")


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).astype(np.float64)


def _dot_abs(m, cols, p):
    """(value, sum of |terms|, exact in float32?) of p[0] m[c0] + p[1] m[c1] + p[2] m[c2] + m[c3], summed left to right"""
    terms = [m[cols[0]] * p[:, 0], m[cols[1]] * p[:, 1], m[cols[2]] * p[:, 2], np.full(len(p), m[cols[3]])]
    val, exact, acc = np.zeros(len(p)), np.ones(len(p), bool), np.zeros(len(p))
    for t in terms:
        exact &= t.astype(np.float32).astype(np.float64) == t
        acc = acc + t
        exact &= acc.astype(np.float32).astype(np.float64) == acc
        val = acc
    return val, sum(np.abs(t) for t in terms), exact


def _edge_margin(v, hi):
    """(int) of v clamped to [0, hi]: the result changes where v crosses an integer of 1..hi"""
    k = np.clip(np.round(v), 1, hi)
    return np.abs(v - k)


def _trunc_clamp(v, hi):
    return np.clip(np.nan_to_num(v, nan=0.0, posinf=1e18, neginf=-1e18), 0, hi).astype(np.int64)


def project(*, means3D, scales, rotations, opacities, shs, sh_degree, scale_modifier, viewmatrix, projmatrix, campos, W, H,
            tanfovx, tanfovy, **_unused):
    from oracle import dense_torch
    m, s, q, op, sh = _f64(means3D).reshape(-1, 3), _f64(scales).reshape(-1, 3), _f64(rotations).reshape(-1, 4), \
        _f64(opacities).reshape(-1), _f64(shs)
    P = len(m)
    sh = sh.reshape(P, -1, 3)
    V, F, cp = _f64(viewmatrix).reshape(16), _f64(projmatrix).reshape(16), _f64(campos).reshape(3)
    tx_, ty_, mod = float(np.float32(tanfovx)), float(np.float32(tanfovy)), float(np.float32(scale_modifier))
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    o = {}
    with np.errstate(all="ignore"):
        # view space; row-vector convention: [x y z 1] @ V
        pv, pv_abs, pv_exact = zip(*(_dot_abs(V, (c, 4 + c, 8 + c, 12 + c), m) for c in range(3)))
        x, y, z = pv
        o["pv"] = np.stack(pv, 1)
        o["visible_z"] = (z >= NEAR) if KNOBS["near_strict"] else (z > NEAR)
        o["m_near"], o["s_near"] = np.abs(z - NEAR), np.where(pv_exact[2], 0.0, pv_abs[2])
        # 3D covariance
        cov = dense_torch._cov3d(torch.from_numpy(s), mod, torch.from_numpy(q)).numpy()
        o["cov3D"] = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)
        r_, qx, qy, qz = q.T
        R_abs = np.stack([1 + 2 * (qy * qy + qz * qz), 2 * (np.abs(qx * qy) + np.abs(r_ * qz)), 2 * (np.abs(qx * qz) + np.abs(r_ * qy)),
                          2 * (np.abs(qx * qy) + np.abs(r_ * qz)), 1 + 2 * (qx * qx + qz * qz), 2 * (np.abs(qy * qz) + np.abs(r_ * qx)),
                          2 * (np.abs(qx * qz) + np.abs(r_ * qy)), 2 * (np.abs(qy * qz) + np.abs(r_ * qx)), 1 + 2 * (qx * qx + qy * qy)],
                         1).reshape(P, 3, 3)
        L_abs = R_abs * (mod * s)[:, None, :]
        cov_abs = L_abs @ L_abs.transpose(0, 2, 1)
        # EWA Jacobian with the frustum clamp
        fx, fy = W / (2.0 * tx_), H / (2.0 * ty_)
        limx, limy = KNOBS["clamp"] * tx_, KNOBS["clamp"] * ty_
        rx, ry = x / z, y / z
        o["clamp_x"], o["clamp_y"] = np.abs(rx) > limx, np.abs(ry) > limy
        o["m_clamp_x"], o["m_clamp_y"] = np.abs(np.abs(rx) - limx), np.abs(np.abs(ry) - limy)
        o["s_clamp_x"] = (pv_abs[0] + np.abs(rx) * pv_abs[2]) / np.abs(z)
        o["s_clamp_y"] = (pv_abs[1] + np.abs(ry) * pv_abs[2]) / np.abs(z)
        cx, cy = np.clip(rx, -limx, limx) * z, np.clip(ry, -limy, limy) * z
        Wr = V.reshape(4, 4)[:3, :3].T                      # view = Wr world + t
        J0 = np.stack([fx / z, np.zeros(P), -fx * cx / (z * z)], 1)
        J1 = np.stack([np.zeros(P), fy / z, -fy * cy / (z * z)], 1)
        T0, T1 = J0 @ Wr, J1 @ Wr
        T0a, T1a = np.abs(J0) @ np.abs(Wr), np.abs(J1) @ np.abs(Wr)
        quad = lambda u, S, w: np.einsum("pi,pij,pj->p", u, S, w)  # noqa: E731
        a, b, c = quad(T0, cov, T0) + 0.3, quad(T0, cov, T1), quad(T1, cov, T1) + 0.3
        a_abs, c_abs = quad(T0a, cov_abs, T0a) + 0.3, quad(T1a, cov_abs, T1a) + 0.3
        b_abs = quad(T0a, cov_abs, T1a)
        o["a"], o["b"], o["c"] = a, b, c
        det = a * c - b * b
        o["conic"] = np.stack([c / det, -b / det, a / det], 1)
        mid = 0.5 * (a + c)
        disc2 = mid * mid - det
        disc = np.sqrt(np.maximum(0.1, disc2))
        lam = mid + disc
        rad3 = 3.0 * np.sqrt(lam)
        o["rad_f"] = np.ceil(rad3)
        o["m_radius"] = np.minimum(rad3 - np.floor(rad3), np.ceil(rad3) - rad3)
        # d lam: the entries' own rounding, and through the discriminant (mid^2 - det = ((a - c) / 2)^2 + b^2)
        d_disc = np.where(disc2 > 0.1, (np.abs(a - c) * 0.5 * (a_abs + c_abs) * 0.5 + 2 * np.abs(b) * b_abs + disc2) / (2 * disc), 0.0)
        o["s_radius"] = 1.5 / np.sqrt(lam) * (0.5 * (a_abs + c_abs) + d_disc + lam) + rad3
        # pixel position
        hx, hx_abs, _ = _dot_abs(F, (0, 4, 8, 12), m)
        hy, hy_abs, _ = _dot_abs(F, (1, 5, 9, 13), m)
        hw, hw_abs, _ = _dot_abs(F, (3, 7, 11, 15), m)
        pw = 1.0 / (hw + 0.0000001)
        ndx, ndy = hx * pw, hy * pw
        mx, my = ((ndx + 1.0) * W - 1.0) * 0.5, ((ndy + 1.0) * H - 1.0) * 0.5
        o["mx"], o["my"] = mx, my
        s_mx = 0.5 * W * (np.abs(pw) * (hx_abs + np.abs(ndx) * hw_abs) + 2 * np.abs(ndx) + 2)
        s_my = 0.5 * H * (np.abs(pw) * (hy_abs + np.abs(ndy) * hw_abs) + 2 * np.abs(ndy) + 2)
        o["s_mx"], o["s_my"], o["s_z"] = s_mx, s_my, pv_abs[2]
        # the reference rect: the tiles of the square (mx, my) +- radius
        rad = o["rad_f"]
        pad = KNOBS["upper_pad"]
        ev = dict(x0=(mx - rad) / TILE, y0=(my - rad) / TILE, x1=(mx + rad + pad) / TILE, y1=(my + rad + pad) / TILE)
        for k, v in ev.items():
            hi, sm, ctr = (gx, s_mx, mx) if k[0] == "x" else (gy, s_my, my)
            o["m_" + k], o["s_" + k] = _edge_margin(v, hi), (sm + np.abs(ctr) + rad + TILE) / TILE
        rect = np.stack([_trunc_clamp(ev["x0"], gx), _trunc_clamp(ev["y0"], gy), _trunc_clamp(ev["x1"], gx), _trunc_clamp(ev["y1"], gy)], 1)
        area = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
        vis = o["visible_z"] & (det != 0) & (area > 0)
        o["visible"] = vis
        o["radius"] = np.where(vis, np.minimum(rad, 2147483520.0), 0).astype(np.int64)
        rect[~vis] = 0
        o["rect"] = rect
        # colour
        d_ = m - cp
        d_ = d_ / np.linalg.norm(d_, axis=1, keepdims=True)
        sh_m = sh.copy()
        if sh.shape[1] > 6:
            sh_m[:, 6] *= KNOBS["sh6_sign"]
        col = dense_torch._sh_rgb(int(sh_degree), torch.from_numpy(sh_m), torch.from_numpy(d_)).numpy() + 0.5
        nb = (int(sh_degree) + 1) ** 2
        # |basis| <= 1.1 for a unit direction up to degree 3; the direction itself carries a few roundings (factor degree + 1)
        col_abs = 0.5 + 1.1 * (int(sh_degree) + 1) * np.abs(sh[:, :nb]).sum(1)
        o["colour_raw"], o["colour"] = col, np.maximum(col, 0.0)
        o["clamp_bits"] = ((col < 0) * np.array([1, 2, 4])).sum(1)
        for ch in range(3):
            o[f"m_ch{ch}"], o[f"s_ch{ch}"] = np.abs(col[:, ch]), col_abs[:, ch]
        # footprint half-extents: op exp(-d^2 / (2 a)) >= 1/255 along x needs |d| <= sqrt(2 ln(255 op) a)
        o["opacity"] = op
        o["gate"] = op >= OP_GATE                      # compared in float32 on the same bits: exact
        o["m_gate"] = np.abs(op - OP_GATE)
        tau2 = KNOBS["tau_factor"] * np.log(np.maximum(255.0 * op, 1.0))
        ext_x, ext_y = np.sqrt(tau2 * a), np.sqrt(tau2 * c)
        o["ext_x"], o["ext_y"] = np.where(o["gate"], ext_x, -1.0e30), np.where(o["gate"], ext_y, -1.0e30)
        # the tight rect: tile t holds the pixel centres 16 t .. 16 t + 15
        tv = dict(tx0=(mx - ext_x - (TILE - 1)) / TILE, ty0=(my - ext_y - (TILE - 1)) / TILE, tx1=(mx + ext_x) / TILE, ty1=(my + ext_y) / TILE)
        t0x, t0y = _trunc_clamp(np.ceil(tv["tx0"]), gx), _trunc_clamp(np.ceil(tv["ty0"]), gy)
        t1x, t1y = _trunc_clamp(np.floor(tv["tx1"]) + 1.0, gx), _trunc_clamp(np.floor(tv["ty1"]) + 1.0, gy)
        x0 = np.maximum(rect[:, 0], t0x)
        x1 = np.maximum(x0, np.minimum(rect[:, 2], t1x))
        y0 = np.maximum(rect[:, 1], t0y)
        y1 = np.maximum(y0, np.minimum(rect[:, 3], t1y))
        x1 = np.where(o["gate"], x1, x0)
        tight = np.stack([x0, y0, x1, y1], 1)
        tight[~vis] = 0
        o["tight"] = tight
        d_tau = 2.0 + tau2
        for k, v in tv.items():
            e, aa, a_s, sm, ctr, hi = (ext_x, a, a_abs, s_mx, mx, gx) if k[1] == "x" else (ext_y, c, c_abs, s_my, my, gy)
            o["m_" + k] = np.abs(v - np.round(v))
            rounding = (sm + np.abs(ctr) + e + TILE + 0.5 * e * (a_s / aa + d_tau / np.maximum(tau2, 1e-300))) / TILE
            o["s_" + k] = rounding
            o["slack_" + k] = (EXT_SLACK_REL * e + EXT_SLACK_ABS) / TILE
    return o


def fragile(o, name, ulps=None):
    """The decisions `name` whose margin is within `ulps` float32 roundings of the threshold.  A rect edge is also fragile
    where the radius is; a tight edge also inside the kernel's deliberate slack."""
    ulps = FRAGILE_ULPS if ulps is None else ulps
    f = o["m_" + name] < ulps * EPS32 * o["s_" + name]
    if name in ("x0", "y0", "x1", "y1") or name in TIGHT_DECISIONS:
        f = f | fragile(o, "radius", ulps)
    if name in TIGHT_DECISIONS:
        f = f | (o["m_" + name] < ulps * EPS32 * o["s_" + name] + o["slack_" + name]) | fragile(o, name[1:], ulps)
    return f


def any_fragile(o, names=DECISIONS, ulps=None):
    return np.any([fragile(o, k, ulps) for k in names], 0)


def rect_area(rect):
    rect = np.asarray(rect)
    return (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])


def rect_tiles(rect, gx):
    """-> per Gaussian the sorted array of tile ids of its rect"""
    out = []
    for x0, y0, x1, y1 in np.asarray(rect):
        ys, xs = np.mgrid[y0:y1, x0:x1]
        out.append(np.sort((ys * gx + xs).ravel()))
    return out


def footprint_reach(op, conic, mx, my, tile, W, H):
    """float64 maximum of op exp(-1/2 d^T conic d) over the pixel centres of tile (tx, ty), clipped to the image; evaluated on
    the pixel grid.  Arguments broadcast over a leading axis: op [n], conic [n, 3] (xx, xy, yy), mx, my [n], tile [n, 2]."""
    op, mx, my = (np.atleast_1d(np.asarray(v, np.float64)) for v in (op, mx, my))
    conic, tile = np.asarray(conic, np.float64).reshape(-1, 3), np.asarray(tile, np.int64).reshape(-1, 2)
    ly, lx = np.mgrid[0:TILE, 0:TILE]
    px = tile[:, 0, None, None] * TILE + lx
    py = tile[:, 1, None, None] * TILE + ly
    inside = (px < W) & (py < H)
    dx, dy = mx[:, None, None] - px, my[:, None, None] - py
    power = -0.5 * (conic[:, 0, None, None] * dx * dx + conic[:, 2, None, None] * dy * dy) - conic[:, 1, None, None] * dx * dy
    alpha = np.where(inside, op[:, None, None] * np.exp(np.minimum(power, 0.0)), 0.0)
    return alpha.reshape(len(op), -1).max(1)


def dropped_reach(o, W, H, records=None):
    """Every (Gaussian, tile) of the reference rect that the tight rect leaves out, and the footprint's reach there -- from
    this reference's own quantities, or from [P, >= 6] records (mx, my, conic xx, xy, yy, opacity) of an implementation.
    -> (Gaussian ids, tiles [n, 2], reach [n])"""
    ids, tiles = [], []
    for g in np.nonzero(o["visible"])[0]:
        x0, y0, x1, y1 = o["rect"][g]
        a0, b0, a1, b1 = o["tight"][g]
        for ty in range(y0, y1):
            for tx in range(x0, x1):
                if not (a0 <= tx < a1 and b0 <= ty < b1):
                    ids.append(g)
                    tiles.append((tx, ty))
    ids, tiles = np.asarray(ids, np.int64), np.asarray(tiles, np.int64).reshape(-1, 2)
    if len(ids) == 0:
        return ids, tiles, np.zeros(0)
    if records is None:
        reach = footprint_reach(o["opacity"][ids], o["conic"][ids], o["mx"][ids], o["my"][ids], tiles, W, H)
    else:
        r = np.asarray(records, np.float64)[ids]
        reach = footprint_reach(r[:, 5], r[:, 2:5], r[:, 0], r[:, 1], tiles, W, H)
    return ids, tiles, reach


INT_DECISIONS = ("visible", "radius", "x0", "y0", "x1", "y1", "ch0", "ch1", "ch2")


def implementation_view(radii, rect, clamped, records, near=None):
    """What an implementation decided, in one shape for oracle/tile_ref.c and the device: radii [P], rect [P, 4] tiles (None:
    not observed), clamped [P, 3] booleans, records [P, >= 10] (mx, my, conic xx xy yy, opacity, r g b, depth), near [P]
    (passed the near plane; None: not observed)."""
    return dict(radius=np.asarray(radii).astype(np.int64), rect=None if rect is None else np.asarray(rect).astype(np.int64),
                clamped=np.asarray(clamped).astype(bool), records=np.asarray(records, np.float64),
                near=None if near is None else np.asarray(near).astype(bool))


def disagreements(o, impl, ulps=None):
    """-> {decision: (differs [P] bool, fragile [P] bool, counted [P] bool)} of the integer and boolean decisions.  visible:
    radius > 0 on both sides (fragile where the near verdict, the radius or a rect edge is); the others where both sides see
    the Gaussian.  near (when observed): the near-plane verdict alone."""
    both = o["visible"] & (impl["radius"] > 0)
    edges_fragile = np.any([fragile(o, k, ulps) for k in ("x0", "y0", "x1", "y1")], 0)
    out = {"visible": (o["visible"] != (impl["radius"] > 0), fragile(o, "near", ulps) | edges_fragile, np.ones(len(both), bool)),
           "radius": (o["radius"] != impl["radius"], fragile(o, "radius", ulps), both)}
    if impl["near"] is not None:
        out["near"] = (o["visible_z"] != impl["near"], fragile(o, "near", ulps), np.ones(len(both), bool))
    if impl["rect"] is not None:
        for k, name in enumerate(("x0", "y0", "x1", "y1")):
            out[name] = (o["rect"][:, k] != impl["rect"][:, k], fragile(o, name, ulps), both)
    for ch in range(3):
        out[f"ch{ch}"] = ((o["colour_raw"][:, ch] < 0) != impl["clamped"][:, ch], fragile(o, f"ch{ch}", ulps), both)
    return {k: (d & c, f, c) for k, (d, f, c) in out.items()}


def needed_ulps(o, impl):
    """For every disagreement, margin / (EPS32 * scale) of the decision that differs: the multiple that would have made it
    fragile (inf where the scale is 0: an exact decision that differs) -> {decision: array}"""
    out = {}
    for k, (differs, _f, _c) in disagreements(o, impl, 0.0).items():
        names = ("near", "x0", "y0", "x1", "y1", "radius") if k == "visible" else ((k, "radius") if k in ("x0", "y0", "x1", "y1") else (k,))
        with np.errstate(all="ignore"):
            need = np.min([o["m_" + n][differs] / (EPS32 * o["s_" + n][differs]) for n in names], 0)
        out[k] = need
    return out


def rounding_ratios(o, impl):
    """|float32 value - float64 value| / (EPS32 * scale) of the decided quantities an implementation stores: pixel position,
    view depth, unclamped colour -- how many of its own `scale` units a float32 evaluation really moves -> {name: array}"""
    both = np.nonzero(o["visible"] & (impl["radius"] > 0))[0]
    r = impl["records"][both]
    out = dict(mx=np.abs(r[:, 0] - o["mx"][both]) / (EPS32 * o["s_mx"][both]), my=np.abs(r[:, 1] - o["my"][both]) / (EPS32 * o["s_my"][both]),
               z=np.abs(r[:, 9] - o["pv"][both, 2]) / (EPS32 * o["s_z"][both]))
    for ch in range(3):
        ok = o["colour_raw"][both, ch] > 0
        out[f"ch{ch}"] = (np.abs(r[:, 6 + ch] - o["colour_raw"][both, ch]) / (EPS32 * o[f"s_ch{ch}"][both]))[ok]
    return out


def word_errors(o, impl):
    """Errors of the float record words where both sides see the Gaussian: pos (mx, my), rgb, depth as |err| / (1 + |x|), conic
    against the largest conic entry of its Gaussian -> ({word: [n, ...] errors}, the Gaussians compared)"""
    both = np.nonzero(o["visible"] & (impl["radius"] > 0))[0]
    r = impl["records"][both]
    rel = lambda got, ref: np.abs(got - ref) / (1 + np.abs(ref))  # noqa: E731
    cn = o["conic"][both]
    err = dict(pos=rel(r[:, 0:2], np.stack([o["mx"], o["my"]], 1)[both]), conic=np.abs(r[:, 2:5] - cn) / np.abs(cn).max(1, keepdims=True),
               rgb=rel(r[:, 6:9], o["colour"][both]), depth=rel(r[:, 9], o["pv"][both, 2]))
    return err, both
