"""tests/contrib_ref.py pinned to the blend reference it is built on, on the scenes of tests/test_gpu_contrib.py (through
oracle/tile_ref.c: with reference binning the device's lists and records are these); the float32-against-float64 noise of the
weights measured on exactly those scenes -- the GPU bounds (contrib_ref.WEIGHT_BOUND / WMAX_BOUND / TIE_THRESHOLD) are 10 x the
largest 99th percentile found here, never taken from the kernel; the cap on the pixels the GPU comparison leaves out; and the
argument errors of b3gs_blend_contribution_batch, which need no device.  No GPU.

Measured (99th percentile of the relative float32 error of weight and wmax over the Gaussians with hits > 0, and of the
per-entry w):
    stack1    1.6e-8  7.2e-9  1.3e-7     stack63   1.1e-7  6.1e-7  1.8e-6     stack64   1.1e-7  6.4e-7  1.8e-6
    stack65   1.1e-7  6.7e-7  1.8e-6     stack255  4.2e-7  6.7e-6  6.7e-6     stack256  4.2e-7  7.0e-6  6.7e-6
    stack257  4.3e-7  7.0e-6  6.7e-6     stack513  8.3e-7  1.3e-5  1.3e-5     ladder_b  3.4e-7  5.8e-6  5.6e-6
    cull 96x64 2.2e-7 3.8e-7  2.4e-6     cull 72x41 3.4e-7 7.0e-7  2.5e-6     cull 75x33 1.3e-6 1.6e-6  2.0e-6
    wide      1.2e-7  8.2e-7  1.9e-6
  largest: weight 1.289e-6, wmax 1.322e-5, per-entry w 1.330e-5  ->  WEIGHT_BOUND 1.3e-5, WMAX_BOUND 1.33e-4, TIE_THRESHOLD
  1.34e-4.  (A Gaussian's weight sums many pixels whose rounding errors are independent; its largest w is one entry deep in a
  list and carries the error of every factor of T in front of it -- hence the larger figure.)
Masked pixels: no scene holds a near-tie of dominance (the identical splats of a stack have falling weights, alpha (1 - alpha)^k,
a relative step of alpha >= 1/255 between neighbours); the masked pixels are the fragile ones: ladder_b 1 of 1024, cull 96x64 7 of
6144, cull 72x41 5 of 2952, cull 75x33 12 of 2475 (0.485 %), every other scene none.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import blend_ref
import contrib_ref
import helpers
from helpers import FRAGILE_MARGIN
from oracle import tile_ref

CASES = tuple(("stack%d" % L, None, None) for L in (1, 63, 64, 65, 255, 256, 257, 513)) + (
    ("ladder_b", None, None), ("cull", 96, 64), ("cull", 72, 41), ("cull", 75, 33), ("wide", None, None))


@functools.lru_cache(maxsize=None)
def _case(name, W, H):
    d = helpers.blend_scene(name, W, H)
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
    return st, contrib_ref.contributions(st)


@pytest.mark.parametrize("name,W,H", CASES)
def test_sums_of_the_statistics_equal_the_blend_reference(name, W, H):
    st, c = _case(name, W, H)
    hits_total = int(sum(b.sum() for b in st.blended))
    assert hits_total > 0
    # alpha sum: every w is quantised once, off by at most half a unit of 2^-32
    assert abs(c["weight"].sum() - st.alpha.sum()) <= hits_total * 2.0 ** -32
    assert int(c["hits"].sum()) == hits_total
    assert int(c["dominant"].sum()) == int((st.n_contrib > 0).sum())
    assert (c["wmax"][c["hits"] > 0] > 0).all() and not c["wmax"][c["hits"] == 0].any()
    assert (c["dominant"] <= c["hits"]).all()
    assert (c["weight"] <= c["hits"] * c["wmax"] * (1 + 1e-12) + c["hits"] * 2.0 ** -33).all()


def test_a_mask_counts_only_its_pixels_and_an_empty_one_nothing():
    st, c = _case("cull", 75, 33)
    none = contrib_ref.contributions(st, np.zeros((st.H, st.W), np.uint8))
    assert not none["weight_q"].any() and not none["hits"].any() and not none["wmax"].any() and not none["dominant"].any()
    left = np.zeros((st.H, st.W), np.uint8)
    left[:, :40] = 1
    a, b = contrib_ref.contributions(st, left), contrib_ref.contributions(st, 1 - left)
    for k in ("weight_q", "hits", "dominant"):
        assert np.array_equal(a[k] + b[k], c[k]), k
    assert np.array_equal(np.maximum(a["wmax"], b["wmax"]), c["wmax"])
    assert np.array_equal(a["dom_margin"], c["dom_margin"])


def test_float32_noise_pins_the_gpu_bounds_and_the_masked_share_stays_under_its_cap():
    worst = [0.0, 0.0, 0.0]
    for name, W, H in CASES:
        st, c = _case(name, W, H)
        fig = contrib_ref.noise(c)
        frag = st.margin < FRAGILE_MARGIN
        tie = c["dom_margin"] < contrib_ref.TIE_THRESHOLD
        masked = frag | tie
        print(f"{name:9s} {st.W}x{st.H}: 99th percentile weight {fig[0]:.2e}  wmax {fig[1]:.2e}  entry w {fig[2]:.2e}   fragile "
              f"{int(frag.sum())} near-tie {int(tie.sum())} masked {int(masked.sum())} of {masked.size} ({100 * masked.mean():.3f} %)")
        worst = [max(a, b) for a, b in zip(worst, fig)]
        assert masked.mean() <= contrib_ref.MASKED_CAP, f"{name}: {masked.sum()} of {masked.size} pixels left out"
    print("largest 99th percentiles: weight %.3e  wmax %.3e  entry w %.3e" % tuple(worst))
    assert 10 * worst[0] <= contrib_ref.WEIGHT_BOUND <= 11 * worst[0]
    assert 10 * worst[1] <= contrib_ref.WMAX_BOUND <= 11 * worst[1]
    assert 10 * worst[2] <= contrib_ref.TIE_THRESHOLD <= 11 * worst[2]
    assert contrib_ref.MASKED_CAP == 0.02


def test_argument_errors_of_the_entry_point_need_no_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    fn = L.b3gs_blend_contribution_batch
    sc = _lib.B3gsScene()
    sc.P, sc.W, sc.H = 10, 32, 16
    buf = (C.c_uint8 * 64)()                      # host bytes: never read, the call must fail before any HIP call
    p = C.addressof(buf)
    view = _lib.B3gsContribView(C.pointer(sc), p, p, p, None)
    views = (_lib.B3gsContribView * 9)(*([view] * 9))
    out = _lib.B3gsContribOut(p, p, p, p)
    for n in (0, 9, -1):
        assert fn(n, views, C.byref(out), None) == -1 and b"1..8 views" in L.b3gs_last_error()
    assert fn(1, None, C.byref(out), None) == -1 and b"NULL view table" in L.b3gs_last_error()
    assert fn(1, views, None, None) == -1 and b"NULL view table or output table" in L.b3gs_last_error()
    for k in ("weight_q32", "hits", "wmax_bits", "dominant"):
        bad = _lib.B3gsContribOut(p, p, p, p)
        setattr(bad, k, None)
        assert fn(1, views, C.byref(bad), None) == -1 and b"NULL output array" in L.b3gs_last_error()
    for k in ("geometry", "binning", "image"):
        v = (_lib.B3gsContribView * 1)(_lib.B3gsContribView(C.pointer(sc), p, p, p, None))
        setattr(v[0], k, None)
        assert fn(1, v, C.byref(out), None) == -1 and b"NULL state buffer" in L.b3gs_last_error()
    v = (_lib.B3gsContribView * 1)(_lib.B3gsContribView(None, p, p, p, None))
    assert fn(1, v, C.byref(out), None) == -1 and b"B3gsScene" in L.b3gs_last_error()
    for W, H in ((0, 16), (32, 0), (-1, 16)):
        z = _lib.B3gsScene()
        z.P, z.W, z.H = 10, W, H
        v = (_lib.B3gsContribView * 1)(_lib.B3gsContribView(C.pointer(z), p, p, p, None))
        assert fn(1, v, C.byref(out), None) == -1 and b"W/H" in L.b3gs_last_error()
    other = _lib.B3gsScene()
    other.P, other.W, other.H = 11, 32, 16
    v = (_lib.B3gsContribView * 2)(view, _lib.B3gsContribView(C.pointer(other), p, p, p, None))
    assert fn(2, v, C.byref(out), None) == -1 and b"share P" in L.b3gs_last_error()
    with pytest.raises(_lib.B3gsError, match="b3gs_blend_contribution_batch failed: B3GS_ERR_ARG"):
        _lib.check(fn(0, views, C.byref(out), None), "b3gs_blend_contribution_batch")


def test_the_compiled_module_refuses_host_tensors():
    import torch
    from binocular3dgs_amd import _C, _lib
    z = torch.zeros
    u8 = z(64, dtype=torch.uint8)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.blend_contribution([(u8, u8, u8, 16, 16, None)], z(4, dtype=torch.int64), z(4, dtype=torch.int32), z(4, dtype=torch.int32),
                              z(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        _C.blend_contribution([], z(4, dtype=torch.int64), z(4, dtype=torch.int32), z(4, dtype=torch.int32), z(4, dtype=torch.int32))
