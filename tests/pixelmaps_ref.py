"""Per-pixel geometry maps restated in numpy -- TEST INFRASTRUCTURE, the reference of tests/test_gpu_pixelmaps.py.

Built on a float64 blend_ref.forward() State, as tests/contrib_ref.py is: State.blended says which (tile, list entry, pixel) the
forward blended; T restarts from 1 and is multiplied by (1 - alpha) at every blended entry, w = alpha * T with T in front of
the entry, d = the record's depth (column 9, a float32 number).  maps() walks the blended entries twice -- in float64 (the
reference) and in float32 in the kernel's operation order (alpha from blend_ref._eval, w = alpha * T, m1 = fma(d, w, m1),
m2 = fma(w * d, d, m2), T = T * (1 - alpha): the noise yardstick the GPU bounds are derived from) -- and returns what
b3gs_blend_pixel_maps_batch writes:

  median_depth  d of the last blended entry whose T before the blend was > 0.5 (0: nothing blended)
  depth_m1      sum of w d
  depth_m2      sum of w d d
  dominant      Gaussian index of the largest w, ties to the first in list order (-1: nothing blended)
  count         number of blended entries

and two margins per pixel: median_margin, the smallest |T_before - 0.5| / 0.5 over the pixel's blended entries (infinity
without any): below the float32 noise of T the median decision may fall either way; and dom_margin of contrib_ref.
"""
import numpy as np

import blend_ref
import contrib_ref
import helpers

PLANES = ("median_depth", "depth_m1", "depth_m2", "dominant", "count")


def maps(st, contrib=None):
    """st: float64 State; contrib: contrib_ref.contributions(st) when the caller has it.  -> dict of [H, W] arrays
    median_depth, depth_m1, depth_m2 (float64), dominant, count (int64)      from float64
    the same names + "32"                                                    from float32 in the kernel's operation order
    median_margin, dom_margin
    and entry_T64, entry_T32: T in front of every blended (entry, pixel), flat, the same order in both."""
    assert st.dtype is np.float64
    W, H, (gx, gy) = st.W, st.H, st.grid
    R64 = np.asarray(st.records)[:, :10].astype(np.float64)
    R32 = np.asarray(st.records)[:, :10].astype(np.float32)
    f32 = np.float32
    out = {}
    for k in ("median_depth", "depth_m1", "depth_m2"):
        out[k], out[k + "32"] = np.zeros((H, W)), np.zeros((H, W))
    for k, fill in (("dominant", -1), ("count", 0)):
        out[k], out[k + "32"] = np.full((H, W), fill, np.int64), np.full((H, W), fill, np.int64)
    out["median_margin"] = np.full((H, W), np.inf)
    t64, t32 = [], []
    for t in range(gx * gy):
        ids, blended = st.ids[t], st.blended[t]
        if len(ids) == 0 or not blended.any():
            continue
        px, py, inside, _q = blend_ref._tile_pixels(t, gx, W, H)
        T64, T32 = np.ones(256), np.ones(256, f32)
        a1, a2, med, best, dom, cnt = np.zeros(256), np.zeros(256), np.zeros(256), np.full(256, -1.0), np.full(256, -1, np.int64), np.zeros(256, np.int64)
        b1, b2, med32, best32, dom32 = np.zeros(256, f32), np.zeros(256, f32), np.zeros(256), np.full(256, -1.0, f32), np.full(256, -1, np.int64)
        margin = np.full(256, np.inf)
        for k in np.nonzero(blended.any(1))[0]:
            b = blended[k]
            g = int(ids[k])
            d64, d32 = R64[g, 9], R32[g, 9]
            al64 = blend_ref._eval(R64[g], px.astype(np.float64), py.astype(np.float64), np.float64)[5]
            al32 = blend_ref._eval(R32[g], px.astype(f32), py.astype(f32), f32)[5]
            w64 = al64 * T64
            w32 = (al32 * T32).astype(f32)
            t64.append(T64[b]); t32.append(T32[b].astype(np.float64))
            margin = np.where(b, np.minimum(margin, np.abs(T64 - 0.5) / 0.5), margin)
            med = np.where(b & (T64 > 0.5), d64, med)
            med32 = np.where(b & (T32 > f32(0.5)), d64, med32)
            a1 = np.where(b, d64 * w64 + a1, a1)
            a2 = np.where(b, (w64 * d64) * d64 + a2, a2)
            b1 = np.where(b, blend_ref._fma(d32, w32, b1, f32), b1)
            b2 = np.where(b, blend_ref._fma((w32 * d32).astype(f32), d32, b2, f32), b2)
            up, up32 = b & (w64 > best), b & (w32 > best32)
            dom, best = np.where(up, g, dom), np.where(up, w64, best)
            dom32, best32 = np.where(up32, g, dom32), np.where(up32, w32, best32)
            cnt = cnt + b
            T64 = np.where(b, T64 * (1.0 - al64), T64)
            T32 = np.where(b, (T32 * (f32(1.0) - al32)).astype(f32), T32)
        yy, xx = py[inside], px[inside]
        for name, a, a32 in (("median_depth", med, med32), ("depth_m1", a1, b1), ("depth_m2", a2, b2), ("dominant", dom, dom32),
                             ("count", cnt, cnt)):
            out[name][yy, xx], out[name + "32"][yy, xx] = a[inside], a32[inside]
        out["median_margin"][yy, xx] = margin[inside]
    out["dom_margin"] = (contrib_ref.contributions(st) if contrib is None else contrib)["dom_margin"]
    out["entry_T64"] = np.concatenate(t64) if t64 else np.zeros(0)
    out["entry_T32"] = np.concatenate(t32) if t32 else np.zeros(0)
    return out


def noise(m):
    """99th percentiles of the float32-against-float64 relative error of one maps() result -> (depth_m1 and depth_m2 over the
    pixels with count > 0, T_before over the blended entries with T_before >= 0.25: the only region where the median decision
    is taken)."""
    h = m["count"] > 0
    e1 = np.abs(m["depth_m132"][h] - m["depth_m1"][h]) / m["depth_m1"][h]
    e2 = np.abs(m["depth_m232"][h] - m["depth_m2"][h]) / m["depth_m2"][h]
    r = m["entry_T64"] >= 0.25
    eT = np.abs(m["entry_T32"][r] - m["entry_T64"][r]) / m["entry_T64"][r]
    return float(np.percentile(e1, 99)), float(np.percentile(e2, 99)), float(np.percentile(eT, 99))


# Bounds of tests/test_gpu_pixelmaps.py: 10 x the largest 99th percentile over the scenes of tests/test_pixelmaps_ref_cpu.py
# (which measures and pins them; the table is in its docstring), rounded up by less than 10 %.  Relative; never taken from the
# kernel.
M1_BOUND, M2_BOUND = 5.3e-5, 6.2e-5
# a pixel with a blended entry whose T_before is closer to one half than this (relative) may take either median: 10 x the
# float32 noise of T_before >= 0.25
MEDIAN_THRESHOLD = 6.8e-5


def solid_mask(st, m, fragile_margin):
    """[H, W] bool: the pixels the GPU comparison counts -- blend decisions not fragile, dominance not a near-tie, no entry
    whose T_before sits on one half."""
    return (st.margin >= fragile_margin) & (m["dom_margin"] >= contrib_ref.TIE_THRESHOLD) & (m["median_margin"] >= MEDIAN_THRESHOLD)


# ---- the two-layer scene ----------------------------------------------------------------------------------------------
TWO_LAYER_SIZE = (32, 32)
TWO_LAYER_D1, TWO_LAYER_D2 = 2.0, 4.0


def two_layer_scene(front_opacity=0.3):
    """32 x 32: one splat of sigma 200 pixels and `front_opacity` at depth 2 -- a sheet of nearly constant alpha over the whole
    image -- in front of a 4 x 4 grid of opaque splats (sigma 6, 8 pixels apart, alpha clamped to 0.99 at their centres) at the
    depths 4.00, 4.02 .. 4.30: the back sheet.  With the front sheet at 0.3, T in front of the back sheet is 0.7 and the median
    lies on the back sheet, while depth_m1 / alpha lies between the two; at 0.7, T is 0.3 there and the median is the front
    sheet's depth."""
    W, H = TWO_LAYER_SIZE
    gx, gy = np.meshgrid(np.arange(4), np.arange(4))
    n = 16
    rng = np.random.RandomState(helpers.hash_name("two_layer"))
    front = dict(x=[15.5], y=[15.5], sig_a=[200.0], sig_b=[200.0], theta=[0.0], opacity=[front_opacity], colour=[[0.8, 0.3, 0.5]],
                 z=[TWO_LAYER_D1])
    back = dict(x=3.5 + 8.0 * gx.ravel(), y=3.5 + 8.0 * gy.ravel(), sig_a=np.full(n, 6.0), sig_b=np.full(n, 6.0), theta=np.zeros(n),
                opacity=np.full(n, 0.9999), colour=rng.uniform(0.05, 0.95, (n, 3)), z=TWO_LAYER_D2 + 0.02 * np.arange(n))
    return helpers.splat_scene(W, H, **helpers._cat(front, back))
