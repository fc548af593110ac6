"""Feature render and feature lift restated in numpy -- TEST INFRASTRUCTURE, the reference of tests/test_gpu_features.py.

Built on a float64 blend_ref.forward() State, next to contrib_ref.py: State.blended says which (tile, list entry, pixel) the
forward blended; T restarts from 1 and is multiplied by (1 - alpha) at every blended entry, w = alpha * T with T in front of the
entry.  Both functions recompute w twice -- in float64 (the reference) and in float32 in the kernels' operation order
(blend_ref._eval; the noise yardstick the GPU bounds are derived from).

  render(st, f)                    per pixel and channel the sum of w f[g, c] over the blended entries: "out" float64, "out32"
                                   float32 as csrc/features.hip forms it (acc = fma(f, w, acc) in list order), "absw" the sum
                                   of w |f[g, c]| (float64) that errors are taken relative to
  lift(st, maps, scale, mask)      per Gaussian and channel the sum over the blended (pixel, entry) at the counted pixels of
                                   w Fn, Fn = clip(maps / scale, -1, 1): "sums_q" the integers sum rint(w Fn 2^32) from float64,
                                   "sums_q32" the kernel's integers (Fn by a float32 division, p = w * Fn one float32 rounding,
                                   rint(p 2^32)), "sums" the unquantised float64 sum of w Fn scale, "absw" the sum of w |Fn|,
                                   "hits", and "weight_q" (contrib_ref's)

Two mutants the checks of the GPU tests must reject (MUTANTS): lift(..., mutant="unsigned_high") forgets the sign of the high
half when an entry's integer is split in 16 low bits and the rest; render(..., mutant="ragged_last") skips the last channel of
a channel count that is no multiple of 8.
"""
import numpy as np

import blend_ref

Q32 = 4294967296.0
GROUP = 8
MUTANTS = ("unsigned_high", "ragged_last")

# Bounds of tests/test_gpu_features.py: 10 x the largest 99th percentile over the scenes of tests/test_features_ref_cpu.py
# (which measures and pins them; the table is in its docstring), rounded up by less than 10 %.  RENDER_BOUND is relative to the
# sum of w |f| of the pixel and channel, LIFT_BOUND to the sum of w |Fn| of the Gaussian and channel (so that cancellation does
# not inflate either).  Never taken from the kernel.
RENDER_BOUND, LIFT_BOUND = 7.5e-6, 4.8e-6


def _entries(st):
    """Per tile and blended list entry: (tile pixels px, py, inside, Gaussian g, blended [256], w64 [256], w32 [256])."""
    assert st.dtype is np.float64
    W, H, (gx, gy) = st.W, st.H, st.grid
    R64 = np.asarray(st.records)[:, :10].astype(np.float64)
    R32 = np.asarray(st.records)[:, :10].astype(np.float32)
    f32 = np.float32
    for t in range(gx * gy):
        ids, blended = st.ids[t], st.blended[t]
        if len(ids) == 0 or not blended.any():
            continue
        px, py, inside, _q = blend_ref._tile_pixels(t, gx, W, H)
        T64, T32 = np.ones(256), np.ones(256, f32)
        for k in np.nonzero(blended.any(1))[0]:
            b = blended[k]
            g = int(ids[k])
            a64 = blend_ref._eval(R64[g], px.astype(np.float64), py.astype(np.float64), np.float64)[5]
            a32 = blend_ref._eval(R32[g], px.astype(f32), py.astype(f32), f32)[5]
            w64 = np.where(b, a64 * T64, 0.0)
            w32 = np.where(b, (a32 * T32).astype(f32), f32(0.0))
            T64 = np.where(b, T64 * (1.0 - a64), T64)
            T32 = np.where(b, (T32 * (f32(1.0) - a32)).astype(f32), T32)
            yield t, px, py, inside, g, b, w64, w32


def render(st, f, mutant=None):
    """st: float64 State; f: [P, C].  -> dict of [C, H, W] arrays out, out32 (float64 of the float32 result), absw."""
    assert mutant in (None, "ragged_last")
    f = np.asarray(f)
    P, C = f.shape
    assert P == np.asarray(st.records).shape[0]
    f64, f32 = f.astype(np.float64), f.astype(np.float32)
    H, W = st.H, st.W
    out = dict(out=np.zeros((C, H, W)), out32=np.zeros((C, H, W)), absw=np.zeros((C, H, W)))
    cur, acc64, acc32, accabs = None, None, None, None

    def flush():
        yy, xx = cur[2][cur[3]], cur[1][cur[3]]
        out["out"][:, yy, xx], out["out32"][:, yy, xx], out["absw"][:, yy, xx] = acc64[:, cur[3]], acc32[:, cur[3]], accabs[:, cur[3]]

    for t, px, py, inside, g, b, w64, w32 in _entries(st):
        if cur is None or cur[0] != t:
            if cur is not None:
                flush()
            cur = (t, px, py, inside)
            acc64, acc32, accabs = np.zeros((C, 256)), np.zeros((C, 256), np.float32), np.zeros((C, 256))
        acc64 += f64[g][:, None] * w64[None, :]
        accabs += np.abs(f64[g])[:, None] * w64[None, :]
        acc32 = blend_ref._fma(f32[g][:, None], w32[None, :], acc32, np.float32)
    if cur is not None:
        flush()
    if mutant == "ragged_last" and C % GROUP:
        out["out32"][C - 1] = 0.0
    return out


def split_sum(s, mutant=None):
    """The integer the kernel adds for an entry's s (int64 array, |s| < 2^32): 16 low bits plus the arithmetically shifted rest
    times 2^16 -- s itself; the mutant takes the rest as an unsigned 32-bit word."""
    lo, hi = s & 0xFFFF, s >> 16
    if mutant == "unsigned_high":
        hi = hi & 0xFFFFFFFF
    return lo + hi * 65536


def lift(st, maps, scale, mask=None, mutant=None):
    """st: float64 State; maps: [C, H, W]; scale: [C] > 0; mask: [H, W], nonzero = count the pixel (None: every pixel).
    -> dict of sums_q, sums_q32 (int64 [P, C]), sums, absw (float64 [P, C]), hits (int64 [P]), weight_q (int64 [P])."""
    assert mutant in (None, "unsigned_high")
    maps = np.asarray(maps)
    C, H, W = maps.shape
    assert (H, W) == (st.H, st.W)
    scale = np.asarray(scale).reshape(C)
    assert (scale > 0).all()
    P = np.asarray(st.records).shape[0]
    counted = np.ones((H, W), bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    f32 = np.float32
    Fn64 = np.clip(maps.astype(np.float64) / scale.astype(np.float64)[:, None, None], -1.0, 1.0)
    Fn32 = np.clip((maps.astype(f32) / scale.astype(f32)[:, None, None]).astype(f32), f32(-1.0), f32(1.0))
    out = dict(sums_q=np.zeros((P, C), np.int64), sums_q32=np.zeros((P, C), np.int64), sums=np.zeros((P, C)), absw=np.zeros((P, C)),
               hits=np.zeros(P, np.int64), weight_q=np.zeros(P, np.int64))
    for t, px, py, inside, g, b, w64, w32 in _entries(st):
        cx, cy = np.minimum(px, W - 1), np.minimum(py, H - 1)
        c = b & inside & counted[cy, cx]
        if not c.any():
            continue
        F64, F32 = Fn64[:, cy[c], cx[c]], Fn32[:, cy[c], cx[c]]
        p64 = F64 * w64[c][None, :]
        p32 = (F32 * w32[c][None, :]).astype(f32)
        out["sums_q"][g] += np.rint(p64 * Q32).astype(np.int64).sum(1)
        out["sums_q32"][g] += split_sum(np.rint(p32.astype(np.float64) * Q32).astype(np.int64), mutant).sum(1)
        out["sums"][g] += (p64 * scale.astype(np.float64)[:, None]).sum(1)
        out["absw"][g] += np.abs(p64).sum(1)
        out["hits"][g] += int(c.sum())
        out["weight_q"][g] += int(np.rint(w64[c] * Q32).astype(np.int64).sum())
    return out


# ---- the checks of the GPU tests (run against the mutants in tests/test_features_ref_cpu.py) ------------------------------------
def render_error(got, r):
    """|got - reference| relative to the sum of w |f|, [C, H, W]; 0 where both the error and that sum are 0."""
    err = np.abs(np.asarray(got, np.float64) - r["out"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / r["absw"])


def check_render(name, got, r, solid):
    """got: [C, H, W] (the device's planes, or out32 of a mutant) against render()'s float64 on the pixels of `solid`."""
    assert got.shape == r["out"].shape
    e = render_error(got, r)[:, solid]
    assert (r["absw"][:, solid] > 0).any(), f"{name}: nothing was rendered"
    print(f"{name}: largest error relative to sum w|f| {e.max():.2e}")
    assert (e <= RENDER_BOUND).all(), f"{name}: render off by {e.max():.2e} (relative to sum w|f|) in channel {np.argmax(e.max(1))}"


def lift_error(got_q, r):
    """(|got - reference| - the quantisation floor of 2^-32 per hit) relative to the sum of w |Fn|, [P, C]."""
    err = np.maximum(np.abs(np.asarray(got_q, np.float64) - r["sums_q"]) / Q32 - r["hits"][:, None] * 2.0 ** -32, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / r["absw"])


def check_lift(name, got_q, r):
    """got_q: int64 [P, C] (the device's sums, or sums_q32 of a mutant) against lift()'s float64 integers."""
    assert got_q.shape == r["sums_q"].shape
    e = lift_error(got_q, r)
    assert (r["absw"] > 0).any(), f"{name}: nothing was lifted"
    print(f"{name}: largest error relative to sum w|Fn| {e.max():.2e}")
    assert (e <= LIFT_BOUND).all(), f"{name}: lift off by {e.max():.2e} (relative to sum w|Fn|) in channel {np.argmax(e.max(0))}"
    assert not np.asarray(got_q)[r["hits"] == 0].any()


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------
def random_features(P, C, seed=0):
    """float32 [P, C], uniform in [-1, 1), seeded."""
    return np.random.RandomState(9176 + 31 * C + seed).uniform(-1.0, 1.0, (P, C)).astype(np.float32)


def random_maps(C, W, H, seed=0):
    """float32 [C, H, W]: uniform in [-1, 1) times a per-channel amplitude between 0.25 and 4, seeded."""
    rng = np.random.RandomState(5573 + 131 * C + 7 * W + H + seed)
    amp = rng.uniform(0.25, 4.0, (C, 1, 1))
    return (rng.uniform(-1.0, 1.0, (C, H, W)) * amp).astype(np.float32)


def amax_scale(maps):
    """float32 [C]: the largest |F| of every channel, 1 where that is 0 (features.default_scale)."""
    a = np.abs(np.asarray(maps, np.float32)).reshape(maps.shape[0], -1).max(1)
    return np.where(a > 0, a, np.float32(1.0)).astype(np.float32)
