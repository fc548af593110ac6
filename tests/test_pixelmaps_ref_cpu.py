"""tests/pixelmaps_ref.py pinned to the blend reference it is built on, on the scenes of tests/test_gpu_contrib.py (through
oracle/tile_ref.c: with reference binning the device's lists and records are these; the States are those of
tests/test_contrib_ref_cpu.py, computed once); the float32-against-float64 noise of depth_m1, depth_m2 and of T in front of an
entry measured on exactly those scenes -- the GPU bounds (pixelmaps_ref.M1_BOUND / M2_BOUND / MEDIAN_THRESHOLD) are 10 x the
largest 99th percentile found here, never taken from the kernel; the cap on the pixels the GPU comparison leaves out; the
two-layer scene; and the argument errors of b3gs_blend_pixel_maps_batch, which need no device.  No GPU.

Measured (99th percentile of the relative float32 error of depth_m1 and depth_m2 over the pixels with count > 0, and of T in
front of a blended entry over the entries with T >= 0.25, the only region where the median decision is taken; then the number
of distinct median depths):
    stack1    1.3e-7  1.3e-7  0       1     stack63   9.8e-7  1.0e-6  1.8e-6  1     stack64   9.8e-7  1.0e-6  1.8e-6  1
    stack65   9.9e-7  1.1e-6  1.8e-6  1     stack255  3.1e-6  3.6e-6  6.0e-6  55    stack256  3.1e-6  3.6e-6  6.0e-6  55
    stack257  3.1e-6  3.6e-6  6.0e-6  55    stack513  5.3e-6  6.2e-6  6.8e-6  55    ladder_b  2.7e-6  3.1e-6  5.7e-6  115
    cull 96x64 6.6e-7 7.6e-7  2.1e-7  317   cull 72x41 2.9e-7 3.4e-7  3.3e-7  286   cull 75x33 2.8e-7 3.5e-7  2.5e-7  227
    wide      7.7e-7  8.7e-7  1.8e-6  22
  largest: depth_m1 5.284e-6, depth_m2 6.191e-6, T 6.797e-6  ->  M1_BOUND 5.3e-5, M2_BOUND 6.2e-5, MEDIAN_THRESHOLD 6.8e-5.
The stacks of up to 65 splats never bring T to one half: every pixel's median is the last entry of the one list, a single
depth.  They stay for the chunk and wave seams; the scenes that discriminate depths (MEDIAN_SCENES, at least 8 distinct medians
each) are the longer stacks, ladder_b, the cull fields, wide and the two-layer scene.
Masked pixels (fragile, near-tie of dominance, or an entry with |T - 0.5| / 0.5 below MEDIAN_THRESHOLD): no scene holds one of
the last kind at 6.8e-5 (at 1e-4: 14 of 1024 on stack255 .. stack513, 12 on wide, 8 on ladder_b, at most 2 on a cull field), so
the masked pixels are those of tests/test_contrib_ref_cpu.py: at most 12 of 2475 (0.485 %, cull 75x33).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import blend_ref
import contrib_ref
import helpers
import pixelmaps_ref
import test_contrib_ref_cpu
import test_gpu_contrib
from helpers import FRAGILE_MARGIN
from oracle import tile_ref

CASES = test_gpu_contrib.CASES
MEDIAN_SCENES = tuple(c for c in CASES if c[0] not in ("stack1", "stack63", "stack64", "stack65"))


@functools.lru_cache(maxsize=None)
def _case(name, W, H):
    st, c = test_contrib_ref_cpu._case(name, W, H)
    return st, pixelmaps_ref.maps(st, c)


@functools.lru_cache(maxsize=None)
def _two_layer(front_opacity):
    d = pixelmaps_ref.two_layer_scene(front_opacity)
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
    return st, pixelmaps_ref.maps(st)


def test_the_cases_are_the_thirteen_of_the_contribution_tests():
    assert len(CASES) == 13 and CASES == test_contrib_ref_cpu.CASES


@pytest.mark.parametrize("name,W,H", CASES)
def test_planes_agree_with_the_blend_reference(name, W, H):
    st, m = _case(name, W, H)
    blended_total = int(sum(b.sum() for b in st.blended))
    assert blended_total > 0 and int(m["count"].sum()) == blended_total
    assert np.array_equal(m["count"] > 0, st.n_contrib > 0) and (m["count"] <= st.n_contrib).all()
    assert (np.abs(m["depth_m1"] - st.depth) <= 1e-12 * np.abs(st.depth)).all()
    assert np.array_equal(m["dominant"] >= 0, st.n_contrib > 0) and (m["dominant"][m["count"] == 0] == -1).all()
    assert np.array_equal(m["median_depth"] == 0.0, m["count"] == 0)
    assert (m["depth_m2"] * st.alpha >= m["depth_m1"] ** 2 * (1 - 1e-12)).all()
    # the median is the depth of an entry of the pixel's tile list, and T crosses one half no later than the last contributor
    P = np.asarray(st.records).shape[0]
    assert (m["dominant"] < P).all()
    depths = np.asarray(st.records)[:, 9].astype(np.float64)
    assert np.isin(m["median_depth"][m["count"] > 0], depths).all()
    # the float32 restatement takes the same integer decisions wherever no margin is small
    solid = pixelmaps_ref.solid_mask(st, m, FRAGILE_MARGIN)
    for k in ("median_depth", "dominant", "count"):
        assert np.array_equal(m[k + "32"][solid], m[k][solid]), k


@pytest.mark.parametrize("name,W,H", MEDIAN_SCENES)
def test_median_scenes_discriminate_depths(name, W, H):
    st, m = _case(name, W, H)
    solid = pixelmaps_ref.solid_mask(st, m, FRAGILE_MARGIN) & (m["count"] > 0)
    assert len(np.unique(m["median_depth"][solid])) >= 8
    # somewhere T does cross one half before the last contributor: the median is not simply the last entry's depth
    assert (m["median_margin"] < 1.0).any()


def test_two_layers_median_on_the_back_sheet_mean_between():
    d1, d2 = pixelmaps_ref.TWO_LAYER_D1, pixelmaps_ref.TWO_LAYER_D2
    st, m = _two_layer(0.3)
    covered = st.alpha > 0.95
    assert covered.mean() > 0.9
    med = m["median_depth"][covered]
    assert (med >= d2).all() and (med <= d2 + 0.31).all() and len(np.unique(med)) >= 8
    mean = m["depth_m1"][covered] / st.alpha[covered]
    assert (mean > d1 + 0.5).all() and (mean < med - 0.2).all(), "the mean lies strictly between the sheets, at no surface"
    # (row 0 is the front sheet: it holds the largest single weight only between the splats of the back sheet)
    assert (m["dominant"][covered] > 0).mean() > 0.5 and (m["dominant"][covered] == 0).any()
    std = np.sqrt(np.maximum(m["depth_m2"][covered] / st.alpha[covered] - mean ** 2, 0.0))
    assert (std > 0.5).all()
    assert (pixelmaps_ref.solid_mask(st, m, FRAGILE_MARGIN)).mean() >= 1.0 - contrib_ref.MASKED_CAP
    st7, m7 = _two_layer(0.7)
    covered = st7.alpha > 0.9
    assert covered.mean() > 0.9
    assert (m7["median_depth"][covered] == np.float64(np.float32(d1))).all()
    assert (m7["dominant"][covered] == 0).all()
    mean7 = m7["depth_m1"][covered] / st7.alpha[covered]
    assert (mean7 > d1 + 0.3).all() and (mean7 < d2).all()


def test_float32_noise_pins_the_gpu_bounds_and_the_masked_share_stays_under_its_cap():
    worst = [0.0, 0.0, 0.0]
    for name, W, H in CASES:
        st, m = _case(name, W, H)
        fig = pixelmaps_ref.noise(m)
        frag = st.margin < FRAGILE_MARGIN
        tie = m["dom_margin"] < contrib_ref.TIE_THRESHOLD
        med = m["median_margin"] < pixelmaps_ref.MEDIAN_THRESHOLD
        masked = frag | tie | med
        print(f"{name:9s} {st.W}x{st.H}: 99th percentile m1 {fig[0]:.2e}  m2 {fig[1]:.2e}  T (>= 0.25) {fig[2]:.2e}   fragile "
              f"{int(frag.sum())} near-tie {int(tie.sum())} median {int(med.sum())} masked {int(masked.sum())} of {masked.size} "
              f"({100 * masked.mean():.3f} %)   distinct medians {len(np.unique(m['median_depth'][m['count'] > 0]))}")
        worst = [max(a, b) for a, b in zip(worst, fig)]
        assert masked.mean() <= contrib_ref.MASKED_CAP, f"{name}: {masked.sum()} of {masked.size} pixels left out"
    print("largest 99th percentiles: m1 %.3e  m2 %.3e  T %.3e" % tuple(worst))
    assert 10 * worst[0] <= pixelmaps_ref.M1_BOUND <= 11 * worst[0]
    assert 10 * worst[1] <= pixelmaps_ref.M2_BOUND <= 11 * worst[1]
    assert 10 * worst[2] <= pixelmaps_ref.MEDIAN_THRESHOLD <= 11 * worst[2]
    assert contrib_ref.MASKED_CAP == 0.02


def test_argument_errors_of_the_entry_point_need_no_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    fn = L.b3gs_blend_pixel_maps_batch
    View = _lib.B3gsPixelMapView
    sc = _lib.B3gsScene()
    sc.P, sc.W, sc.H = 10, 32, 16
    buf = (C.c_uint8 * 64)()                      # host bytes: never read, the call must fail before any HIP call
    p = C.addressof(buf)
    view = View(C.pointer(sc), p, p, p, p, p, p, p, p)
    views = (View * 9)(*([view] * 9))
    for n in (0, 9, -1):
        assert fn(n, views, None) == -1 and b"1..8 views" in L.b3gs_last_error()
    assert fn(1, None, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    for k in ("geometry", "binning", "image"):
        v = (View * 1)(View(C.pointer(sc), p, p, p, p, p, p, p, p))
        setattr(v[0], k, None)
        assert fn(1, v, None) == -1 and b"NULL state buffer" in L.b3gs_last_error()
    v = (View * 1)(View(None, p, p, p, p, p, p, p, p))
    assert fn(1, v, None) == -1 and b"B3gsScene" in L.b3gs_last_error()
    for W, H in ((0, 16), (32, 0), (-1, 16)):
        z = _lib.B3gsScene()
        z.P, z.W, z.H = 10, W, H
        v = (View * 1)(View(C.pointer(z), p, p, p, p, p, p, p, p))
        assert fn(1, v, None) == -1 and b"W/H" in L.b3gs_last_error()
    other = _lib.B3gsScene()
    other.P, other.W, other.H = 11, 32, 16
    v = (View * 2)(view, View(C.pointer(other), p, p, p, p, p, p, p, p))
    assert fn(2, v, None) == -1 and b"share P" in L.b3gs_last_error()
    empty = _lib.B3gsScene()
    empty.P, empty.W, empty.H = 0, 32, 16
    v = (View * 1)(View(C.pointer(empty), p, p, p, p, p, p, p, p))
    assert fn(1, v, None) == 0, "P == 0: nothing to do, and no HIP call"
    with pytest.raises(_lib.B3gsError, match="b3gs_blend_pixel_maps_batch failed: B3GS_ERR_ARG"):
        _lib.check(fn(0, views, None), "b3gs_blend_pixel_maps_batch")


def test_the_compiled_module_refuses_host_tensors_and_wrong_shapes():
    import torch
    from binocular3dgs_amd import _C, _lib
    u8 = torch.zeros(64, dtype=torch.uint8)
    f = torch.zeros(16, 16)
    i = torch.zeros(16, 16, dtype=torch.int32)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.blend_pixel_maps([(u8, u8, u8, 4, 16, 16)], [(f, f, f, i, i)])
    with pytest.raises(ValueError):
        _C.blend_pixel_maps([], [])
    with pytest.raises(ValueError):
        _C.blend_pixel_maps([(u8, u8, u8, 4, 16, 16)], [])
