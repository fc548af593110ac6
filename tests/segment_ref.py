"""Label votes and label renders restated in numpy -- TEST INFRASTRUCTURE, the reference of tests/test_gpu_segment.py.

Built on a float64 blend_ref.forward() State and on contrib_ref, as tests/pixelmaps_ref.py is: State.blended says which (tile,
list entry, pixel) the forward blended; T restarts from 1 and is multiplied by (1 - alpha) at every blended entry, w = alpha * T
with T in front of the entry.

  votes(st, labels, L)               [P, L] int64: column l is contrib_ref.contributions(st, labels == l)["weight_q"] -- what
                                     b3gs_label_votes_batch sums, by the reference of the kernel it must equal
  label_render(st, gaussian_label, L)   per pixel and label l the sum S_l of w over the blended entries whose Gaussian carries l
                                     (a byte >= L adds to no sum), in float64 and, restated, in float32 in the kernel's operation
                                     order (alpha from blend_ref._eval, w = alpha * T, S_l = S_l + w, T = T * (1 - alpha)); the
                                     winner -- the smallest l of the largest S_l > 0, otherwise 255 --, its sum, and the margin
                                     (S_best - S_second) / S_best, infinity with fewer than two nonzero sums.

Two mutants the tests must catch (label_render(..., mutant=...)): "ties_high" resolves equal sums to the HIGHEST label,
"unlabelled_as_0" counts a Gaussian whose byte is >= L as label 0.
"""
import numpy as np

import blend_ref
import contrib_ref

NO_LABEL = 255
MUTANTS = ("ties_high", "unlabelled_as_0")


def votes(st, labels, L):
    labels = np.asarray(labels).reshape(st.H, st.W)
    return np.stack([contrib_ref.contributions(st, labels == l)["weight_q"] for l in range(L)], 1)


def pick(S, mutant=None):
    """S: [L, n] sums -> (label [n] int64, the winning sum [n]): the smallest l of the largest S_l when that is > 0, else 255
    and 0.  (numpy's argmax returns the first of several equal maxima.)"""
    L = S.shape[0]
    win = (L - 1 - np.argmax(S[::-1], 0)) if mutant == "ties_high" else np.argmax(S, 0)
    best = S.max(0)
    return np.where(best > 0, win, NO_LABEL).astype(np.int64), np.where(best > 0, best, 0.0)


def label_render(st, gaussian_label, L, mutant=None):
    """st: float64 State; gaussian_label: [P] bytes.  -> dict of [H, W] arrays
    label (int64), weight (float64), sums [L, H, W]       from float64
    label32, weight32                                     from float32 in the kernel's operation order
    margin                                                (S_best - S_second) / S_best of the float64 sums"""
    assert st.dtype is np.float64 and mutant in (None,) + MUTANTS
    W, H, (gx, gy) = st.W, st.H, st.grid
    R64 = np.asarray(st.records)[:, :10].astype(np.float64)
    R32 = np.asarray(st.records)[:, :10].astype(np.float32)
    f32 = np.float32
    gl = np.asarray(gaussian_label).astype(np.int64)
    assert gl.shape == (R64.shape[0],)
    gl = np.where(gl < L, gl, 0 if mutant == "unlabelled_as_0" else NO_LABEL)
    out = dict(label=np.full((H, W), NO_LABEL, np.int64), weight=np.zeros((H, W)), label32=np.full((H, W), NO_LABEL, np.int64),
               weight32=np.zeros((H, W)), margin=np.full((H, W), np.inf), sums=np.zeros((L, H, W)))
    for t in range(gx * gy):
        ids, blended = st.ids[t], st.blended[t]
        if len(ids) == 0 or not blended.any():
            continue
        px, py, inside, _q = blend_ref._tile_pixels(t, gx, W, H)
        T64, T32 = np.ones(256), np.ones(256, f32)
        S64, S32 = np.zeros((L, 256)), np.zeros((L, 256), f32)
        for k in np.nonzero(blended.any(1))[0]:
            b = blended[k]
            g = int(ids[k])
            a64 = blend_ref._eval(R64[g], px.astype(np.float64), py.astype(np.float64), np.float64)[5]
            a32 = blend_ref._eval(R32[g], px.astype(f32), py.astype(f32), f32)[5]
            if gl[g] < L:
                S64[gl[g]] = np.where(b, S64[gl[g]] + a64 * T64, S64[gl[g]])
                S32[gl[g]] = np.where(b, (S32[gl[g]] + (a32 * T32).astype(f32)).astype(f32), S32[gl[g]])
            T64 = np.where(b, T64 * (1.0 - a64), T64)
            T32 = np.where(b, (T32 * (f32(1.0) - a32)).astype(f32), T32)
        lab, wgt = pick(S64, mutant)
        lab32, wgt32 = pick(S32.astype(np.float64), mutant)
        top = np.sort(S64, 0)[::-1]
        second = top[1] if L > 1 else np.zeros(256)
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = np.where(second > 0, (top[0] - second) / top[0], np.inf)
        yy, xx = py[inside], px[inside]
        out["label"][yy, xx], out["weight"][yy, xx] = lab[inside], wgt[inside]
        out["label32"][yy, xx], out["weight32"][yy, xx] = lab32[inside], wgt32[inside]
        out["margin"][yy, xx] = margin[inside]
        out["sums"][:, yy, xx] = S64[:, inside]
    return out


def noise(r):
    """99th percentile of the float32-against-float64 relative error of the winning sum over the pixels that have a winner in
    both and agree on it."""
    h = (r["label"] != NO_LABEL) & (r["label"] == r["label32"])
    if not h.any():
        return 0.0
    return float(np.percentile(np.abs(r["weight32"][h] - r["weight"][h]) / r["weight"][h], 99))


# Bound of tests/test_gpu_segment.py on the winning sum: 10 x the largest 99th percentile over the scenes and labelings of
# tests/test_segment_ref_cpu.py (which measures and pins it; the table is in its docstring), rounded up by less than 10 %.
# Relative; never taken from the kernel.
LABEL_WEIGHT_BOUND = 4.7e-5
# Absolute floor next to it: a sum of weights is a part of the pixel's alpha, so it is <= 1 and every one of its float32 adds
# rounds by at most half an ulp of 1; one ulp of 1 is the resolution of the sum itself.
LABEL_WEIGHT_FLOOR = float(np.finfo(np.float32).eps)


def solid_mask(st, r, fragile_margin):
    """[H, W] bool: the pixels the GPU comparison counts -- blend decisions not fragile, the two largest sums no near-tie."""
    return (st.margin >= fragile_margin) & (r["margin"] >= contrib_ref.TIE_THRESHOLD)


# ---- the label planes and the Gaussian labelings of the tests ----------------------------------------------------------------
PLANES = ("constant", "checker", "stripes", "draw16", "draw5")
LABELINGS = ("mod16", "mod3_holes", "single")
# Index mod 3 with every SEVENTH Gaussian unlabelled repeats after 21 indices, and in every period the three labels hold six
# indices each with the SAME index sum (0+3+9+12+15+18 = 1+4+7+10+16+19 = 2+5+8+11+14+17 = 57).  On a stack of identical
# splats, whose weights fall geometrically with the index, the three sums then agree to first order in alpha: whole tiles of
# near-ties, far above contrib_ref.MASKED_CAP, on the stacks whose length is a multiple of 21 plus a little and on the ladder.
# The cap is a condition on the inputs: those scenes take every FIFTH Gaussian unlabelled instead (index sums 21, 31, 26 per
# period of 15); tests/test_segment_ref_cpu.py asserts both halves of this.
SEVENTH_BREAKS_CAP = ("stack63", "stack255", "stack257", "ladder_b")


def labelings_for(name):
    """The three Gaussian labelings scene `name` runs under."""
    return ("mod16", "mod3_holes5" if name in SEVENTH_BREAKS_CAP else "mod3_holes", "single")


def label_plane(kind, W, H):
    """-> (uint8 [H, W], L).  constant: 0 everywhere, L = 1; checker: an 8x8 checker of 0 / 1 aligned to the quadrants;
    stripes: vertical stripes one pixel wide of 0 / 1; draw16: a seeded per-pixel draw from {0 .. 15, 255}, L = 16; draw5: the
    same draw with L = 5, so that the bytes 5 .. 15 are no label."""
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "constant":
        return np.zeros((H, W), np.uint8), 1
    if kind == "checker":
        return (((xx // 8) + (yy // 8)) & 1).astype(np.uint8), 2
    if kind == "stripes":
        return (xx & 1).astype(np.uint8), 2
    if kind in ("draw16", "draw5"):
        rng = np.random.RandomState(1234 + 7 * W + H)
        draw = rng.randint(0, 17, size=(H, W))
        return np.where(draw == 16, NO_LABEL, draw).astype(np.uint8), 16 if kind == "draw16" else 5
    raise KeyError(kind)


def gaussian_labeling(kind, P):
    """-> (uint8 [P], L).  mod16: index mod 16; mod3_holes: index mod 3 with every seventh Gaussian 255 (mod3_holes5: every
    fifth, see SEVENTH_BREAKS_CAP); single: all 0, L = 1."""
    i = np.arange(P)
    if kind == "mod16":
        return (i % 16).astype(np.uint8), 16
    if kind == "mod3_holes":
        return np.where(i % 7 == 6, NO_LABEL, i % 3).astype(np.uint8), 3
    if kind == "mod3_holes5":
        return np.where(i % 5 == 4, NO_LABEL, i % 3).astype(np.uint8), 3
    if kind == "single":
        return np.zeros(P, np.uint8), 1
    raise KeyError(kind)


def tie_records():
    """Two records centred on pixel (3, 3) of a 16 x 16 image whose float32 weights tie exactly: opacity 0.25 in front
    (w = 0.25, T = 0.75), float32(1/3) behind: 0.75 * float32(1/3) rounds to 0.25 in float32 and is 0.25 + 7.5e-9 in float64.
    -> (records [2, 10] float32, lists)."""
    rec = np.zeros((2, 10), np.float32)
    rec[:, 0], rec[:, 1] = 3.0, 3.0
    rec[:, 2], rec[:, 4] = 0.5, 0.5          # conic: sigma^2 = 2 pixels
    rec[0, 5], rec[1, 5] = 0.25, np.float32(1.0) / np.float32(3.0)
    rec[:, 6:9] = 0.5
    rec[:, 9] = (2.0, 3.0)
    return rec, [np.array([0, 1])]
