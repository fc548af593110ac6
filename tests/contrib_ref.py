"""Per-Gaussian render contribution restated in numpy -- TEST INFRASTRUCTURE, the reference of tests/test_gpu_contrib.py.

Built on a float64 blend_ref.forward() State: State.blended says which (tile, list entry, pixel) the forward blended; the weight
of each is w = alpha * T, T restarted from 1 and multiplied by (1 - alpha) at every blended entry.  contributions() recomputes
w twice -- in float64 (the reference) and in float32 in the kernels' operation order (blend_ref._eval: the exponent as
blend_power() forms it; the noise yardstick the GPU bounds are derived from) -- and accumulates, per Gaussian and under an
optional pixel mask, what b3gs_blend_contribution_batch accumulates:

  weight_q   sum of rint(w 2^32) (round to nearest, ties to even, as the header states), an integer; weight = weight_q / 2^32
  hits       number of pixels the Gaussian was blended into
  wmax       largest w
  dominant   number of pixels at which it holds the largest w; ties: the first in list order

and per pixel the dominance margin (w_best - w_second) / w_best, infinity with fewer than two blended entries.
"""
import numpy as np

import blend_ref

Q32 = 4294967296.0


def contributions(st, mask=None):
    """st: float64 State; mask: [H, W], nonzero = count the pixel (None: every pixel).  -> dict of
    weight_q (int64), weight, hits (int64), wmax, dominant (int64)   [P], from float64 w
    weight32, wmax32                                                 [P], from float32 w, the same entries
    dom_margin [H, W]   (all pixels, whatever the mask)
    entry_w64, entry_w32   flat arrays of every blended (entry, pixel) weight, the same order in both"""
    assert st.dtype is np.float64
    W, H, (gx, gy) = st.W, st.H, st.grid
    P = np.asarray(st.records).shape[0]
    R64 = np.asarray(st.records)[:, :10].astype(np.float64)
    R32 = np.asarray(st.records)[:, :10].astype(np.float32)
    counted = np.ones((H, W), bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    out = dict(weight_q=np.zeros(P, np.int64), hits=np.zeros(P, np.int64), wmax=np.zeros(P), dominant=np.zeros(P, np.int64),
               weight_q32=np.zeros(P, np.int64), wmax32=np.zeros(P), dom_margin=np.full((H, W), np.inf))
    e64, e32 = [], []
    for t in range(gx * gy):
        ids, blended = st.ids[t], st.blended[t]
        if len(ids) == 0 or not blended.any():
            continue
        px, py, inside, _q = blend_ref._tile_pixels(t, gx, W, H)
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        cnt_pix = inside & counted[cy, cx]
        T64, T32 = np.ones(256), np.ones(256, np.float32)
        best, second, best_g = np.full(256, -1.0), np.full(256, -1.0), np.zeros(256, np.int64)
        for k in np.nonzero(blended.any(1))[0]:
            b = blended[k]
            g = int(ids[k])
            a64 = blend_ref._eval(R64[g], px.astype(np.float64), py.astype(np.float64), np.float64)[5]
            a32 = blend_ref._eval(R32[g], px.astype(np.float32), py.astype(np.float32), np.float32)[5]
            w64 = np.where(b, a64 * T64, 0.0)
            w32 = np.where(b, a32 * T32, np.float32(0.0))
            T64 = np.where(b, T64 * (1.0 - a64), T64)
            T32 = np.where(b, T32 * (np.float32(1.0) - a32), T32)
            e64.append(w64[b]); e32.append(w32[b].astype(np.float64))
            up = b & (w64 > best)
            second = np.where(up, best, np.where(b & (w64 > second), w64, second))
            best_g = np.where(up, g, best_g)
            best = np.where(up, w64, best)
            c = b & cnt_pix
            if c.any():
                out["weight_q"][g] += int(np.rint(w64[c] * Q32).astype(np.int64).sum())
                out["weight_q32"][g] += int(np.rint(w32[c].astype(np.float64) * Q32).astype(np.int64).sum())
                out["hits"][g] += int(c.sum())
                out["wmax"][g] = max(out["wmax"][g], w64[c].max())
                out["wmax32"][g] = max(out["wmax32"][g], float(w32[c].max()))
        won = cnt_pix & (best >= 0.0)
        np.add.at(out["dominant"], best_g[won], 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(second >= 0.0, (best - second) / best, np.inf)
        out["dom_margin"][py[inside], px[inside]] = m[inside]
    out["weight"] = out["weight_q"] / Q32
    out["weight32"] = out.pop("weight_q32") / Q32
    out["entry_w64"] = np.concatenate(e64) if e64 else np.zeros(0)
    out["entry_w32"] = np.concatenate(e32) if e32 else np.zeros(0)
    return out


def noise(c):
    """99th percentiles of the float32-against-float64 relative error of one contributions() result ->
    (weight over Gaussians with hits > 0, wmax over the same, per-entry w)."""
    h = c["hits"] > 0
    ew = np.abs(c["weight32"][h] - c["weight"][h]) / c["weight"][h]
    em = np.abs(c["wmax32"][h] - c["wmax"][h]) / c["wmax"][h]
    ee = np.abs(c["entry_w32"] - c["entry_w64"]) / c["entry_w64"]
    return float(np.percentile(ew, 99)), float(np.percentile(em, 99)), float(np.percentile(ee, 99))


# Bounds of tests/test_gpu_contrib.py: 10 x the largest 99th percentile over the scenes of tests/test_contrib_ref_cpu.py (which
# measures and pins them; the table is in its docstring), rounded up by less than 10 %.  Relative; never taken from the kernel.
WEIGHT_BOUND, WMAX_BOUND = 1.3e-5, 1.33e-4
# a pixel whose two largest weights are closer than this (relative) is a near-tie: 10 x the per-entry figure
TIE_THRESHOLD = 1.34e-4
MASKED_CAP = 0.02       # fragile + near-tie pixels of a scene: at most this share (a condition on the scenes, not a measurement)


def solid_mask(st, c, fragile_margin):
    """[H, W] bool: the pixels the GPU comparison counts -- decisions not fragile, dominance not a near-tie."""
    return (st.margin >= fragile_margin) & (c["dom_margin"] >= TIE_THRESHOLD)
