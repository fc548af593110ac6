"""tests/features_ref.py on the scenes of tests/test_gpu_contrib.py (through oracle/tile_ref.c: with reference binning the device's
lists and records are these): the float32-against-float64 noise of the feature render and the feature lift measured on exactly
those scenes -- the GPU bounds (features_ref.RENDER_BOUND / LIFT_BOUND) are 10 x the largest 99th percentile found here, never
taken from the kernel; the cap on the pixels the GPU comparison leaves out; the adjoint identity of the pair in float64; the
two mutants against the checks of the GPU tests; and the argument errors of the two entry points, which need no device.  No GPU.

Inputs: C = 19 channels (two full groups and a ragged one), features_ref.random_features / random_maps, scale = the largest |F|
of every channel, the pixels with fragile blend decisions (helpers.FRAGILE_MARGIN) left out of both figures.

Measured (99th percentile of the float32 error of the render relative to sum w|f| over pixels x channels, and of the lift
relative to sum w|Fn| over Gaussians x channels, beyond the quantisation floor of 2^-32 per hit):
    stack1    1.5e-7  0          stack63   2.9e-7  1.5e-8     stack64   3.0e-7  1.5e-8     stack65   3.0e-7  1.9e-8
    stack255  3.4e-7  2.3e-7     stack256  3.4e-7  2.3e-7     stack257  3.3e-7  2.3e-7     stack513  5.0e-7  2.2e-7
    ladder_b  2.6e-7  2.7e-7     cull 96x64 7.4e-7 1.7e-7     cull 72x41 5.1e-7 2.1e-7     cull 75x33 3.8e-7 4.7e-7
    wide      2.5e-7  6.9e-9
  largest: render 7.440e-7, lift 4.698e-7  ->  RENDER_BOUND 7.5e-6, LIFT_BOUND 4.8e-6.  (stack1: every Gaussian's only error is
  below its quantisation floor.)
Masked pixels (fragile decisions; contrib_ref.MASKED_CAP = 0.02): ladder_b 1 of 1024, cull 96x64 7 of 6144, cull 72x41 5 of 2952,
cull 75x33 12 of 2475 (0.485 %), every other scene none.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import blend_ref
import contrib_ref
import features_ref
import helpers
from helpers import FRAGILE_MARGIN
from oracle import tile_ref

CASES = tuple(("stack%d" % L, None, None) for L in (1, 63, 64, 65, 255, 256, 257, 513)) + (
    ("ladder_b", None, None), ("cull", 96, 64), ("cull", 72, 41), ("cull", 75, 33), ("wide", None, None))
NCH = 19


@functools.lru_cache(maxsize=None)
def _case(name, W, H):
    d = helpers.blend_scene(name, W, H)
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
    P = np.asarray(st.records).shape[0]
    f = features_ref.random_features(P, NCH)
    maps = features_ref.random_maps(NCH, st.W, st.H)
    solid = st.margin >= FRAGILE_MARGIN
    return st, f, maps, solid, features_ref.render(st, f), features_ref.lift(st, maps, features_ref.amax_scale(maps), solid)


def _noise(st, solid, r, l):
    er = features_ref.render_error(r["out32"], r)[:, solid][r["absw"][:, solid] > 0]
    el = features_ref.lift_error(l["sums_q32"], l)[l["absw"] > 0]
    return float(np.percentile(er, 99)), float(np.percentile(el, 99))


def test_float32_noise_pins_the_gpu_bounds_and_the_masked_share_stays_under_its_cap():
    worst = [0.0, 0.0]
    for name, W, H in CASES:
        st, f, maps, solid, r, l = _case(name, W, H)
        fig = _noise(st, solid, r, l)
        print(f"{name:9s} {st.W}x{st.H}: 99th percentile render {fig[0]:.2e}  lift {fig[1]:.2e}   fragile {int((~solid).sum())} of "
              f"{solid.size} ({100 * (~solid).mean():.3f} %)")
        worst = [max(a, b) for a, b in zip(worst, fig)]
        assert (~solid).mean() <= contrib_ref.MASKED_CAP, f"{name}: {(~solid).sum()} of {solid.size} pixels left out"
    print("largest 99th percentiles: render %.3e  lift %.3e" % tuple(worst))
    assert 10 * worst[0] <= features_ref.RENDER_BOUND <= 11 * worst[0]
    assert 10 * worst[1] <= features_ref.LIFT_BOUND <= 11 * worst[1]
    assert contrib_ref.MASKED_CAP == 0.02


@pytest.mark.parametrize("name,W,H", CASES)
def test_render_and_lift_are_adjoint_in_float64(name, W, H):
    st, f, maps, solid, r, _l = _case(name, W, H)
    l = features_ref.lift(st, maps, features_ref.amax_scale(maps))      # every pixel, as the render
    lhs = float((r["out"] * maps.astype(np.float64)).sum())
    rhs = float((f.astype(np.float64) * l["sums"]).sum())
    size = float((r["absw"] * np.abs(maps.astype(np.float64))).sum())
    assert size > 0 and abs(lhs - rhs) <= 1e-12 * size, (lhs, rhs)
    # the quantised sums are the unquantised ones to 2^-32 per hit, and the weight is contrib_ref's
    sc = features_ref.amax_scale(maps).astype(np.float64)
    assert (np.abs(l["sums_q"] / features_ref.Q32 * sc - l["sums"]) <= l["hits"][:, None] * 2.0 ** -32 * sc).all()
    c = contrib_ref.contributions(st)
    assert np.array_equal(l["weight_q"], c["weight_q"]) and np.array_equal(l["hits"], c["hits"])


def test_an_indicator_plane_lifts_to_the_contribution_and_its_negative_to_the_negative():
    st = _case("cull", 75, 33)[0]
    plane = (np.arange(st.W)[None, :] + np.arange(st.H)[:, None]) % 3 == 0
    want = contrib_ref.contributions(st, plane)["weight_q"]
    for amp, scale in ((1.0, 1.0), (3.0, 3.0), (0.25, 0.25)):
        l = features_ref.lift(st, (amp * plane)[None].astype(np.float32), [scale])
        assert np.array_equal(l["sums_q"][:, 0], want) and want.sum() > 0
    l = features_ref.lift(st, -plane[None].astype(np.float32), [1.0])
    assert np.array_equal(l["sums_q"][:, 0], -want)
    assert np.array_equal(l["sums_q32"][:, 0], -features_ref.lift(st, plane[None].astype(np.float32), [1.0])["sums_q32"][:, 0])


def test_three_colour_channels_render_the_colour_planes_of_the_blend_reference():
    st = _case("cull", 96, 64)[0]
    rec = np.asarray(st.records)[:, :10].astype(np.float64)
    r = features_ref.render(st, rec[:, 6:10])
    want = np.concatenate([st.color - st.final_T[None] * st.bg[:, None, None], st.depth[None]])
    assert np.abs(r["out"] - want).max() <= 1e-12


def test_both_mutants_are_caught_by_the_checks_of_the_gpu_tests():
    st, f, maps, solid, r, l = _case("cull", 96, 64)
    features_ref.check_render("float32 restatement", r["out32"], r, solid)
    features_ref.check_lift("float32 restatement", l["sums_q32"], l)
    bad = features_ref.render(st, f, mutant="ragged_last")
    assert np.array_equal(bad["out32"][:NCH - 1], r["out32"][:NCH - 1])
    with pytest.raises(AssertionError, match="render off"):
        features_ref.check_render("ragged_last", bad["out32"], r, solid)
    bad = features_ref.lift(st, maps, features_ref.amax_scale(maps), solid, mutant="unsigned_high")
    assert (bad["sums_q32"] != l["sums_q32"]).any()
    with pytest.raises(AssertionError, match="lift off"):
        features_ref.check_lift("unsigned_high", bad["sums_q32"], l)
    # positive maps never reach the mutant's branch: it is the sign that is tested
    pos = np.abs(maps)
    assert np.array_equal(features_ref.lift(st, pos, features_ref.amax_scale(pos), solid, mutant="unsigned_high")["sums_q32"],
                          features_ref.lift(st, pos, features_ref.amax_scale(pos), solid)["sums_q32"])


def test_argument_errors_of_the_entry_points_need_no_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    sc = _lib.B3gsScene()
    sc.P, sc.W, sc.H = 10, 32, 16
    buf = (C.c_uint8 * 64)()                      # host bytes: never read, the calls must fail before any HIP call
    p = C.addressof(buf)
    ones = (C.c_float * 256)(*([1.0] * 256))
    rv = (_lib.B3gsFeatureRenderView * 9)(*([_lib.B3gsFeatureRenderView(C.pointer(sc), p, p, p, p)] * 9))
    lv = (_lib.B3gsFeatureLiftView * 9)(*([_lib.B3gsFeatureLiftView(C.pointer(sc), p, p, p, p, None)] * 9))
    render, lift = L.b3gs_feature_render_batch, L.b3gs_feature_lift_batch
    for n in (0, 9, -1):
        assert render(n, rv, 3, p, None) == -1 and b"1..8 views" in L.b3gs_last_error()
        assert lift(n, lv, 3, ones, p, None, None) == -1 and b"1..8 views" in L.b3gs_last_error()
    for nch in (0, 257, -3):
        assert render(1, rv, nch, p, None) == -1 and b"1..256 channels" in L.b3gs_last_error()
        assert lift(1, lv, nch, ones, p, None, None) == -1 and b"1..256 channels" in L.b3gs_last_error()
    assert render(1, None, 3, p, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    assert render(1, rv, 3, None, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    assert lift(1, None, 3, ones, p, None, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    assert lift(1, lv, 3, None, p, None, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    assert lift(1, lv, 3, ones, None, None, None) == -1 and b"NULL view table" in L.b3gs_last_error()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        s = (C.c_float * 3)(1.0, 1.0, bad)
        assert lift(1, lv, 3, s, p, None, None) == -1 and b"scale" in L.b3gs_last_error()
    other = _lib.B3gsScene()
    other.P, other.W, other.H = 11, 32, 16
    two = (_lib.B3gsFeatureRenderView * 2)(rv[0], _lib.B3gsFeatureRenderView(C.pointer(other), p, p, p, p))
    assert render(2, two, 3, p, None) == -1 and b"share P" in L.b3gs_last_error()
    two = (_lib.B3gsFeatureLiftView * 2)(lv[0], _lib.B3gsFeatureLiftView(C.pointer(other), p, p, p, p, None))
    assert lift(2, two, 3, ones, p, None, None) == -1 and b"share P" in L.b3gs_last_error()
    v = (_lib.B3gsFeatureRenderView * 1)(_lib.B3gsFeatureRenderView(C.pointer(sc), p, p, p, None))
    assert render(1, v, 3, p, None) == -1 and b"NULL output planes" in L.b3gs_last_error()
    v = (_lib.B3gsFeatureLiftView * 1)(_lib.B3gsFeatureLiftView(C.pointer(sc), p, p, p, None, None))
    assert lift(1, v, 3, ones, p, None, None) == -1 and b"NULL feature maps" in L.b3gs_last_error()
    for k in ("geometry", "binning", "image"):
        v = (_lib.B3gsFeatureRenderView * 1)(_lib.B3gsFeatureRenderView(C.pointer(sc), p, p, p, p))
        setattr(v[0], k, None)
        assert render(1, v, 3, p, None) == -1 and b"NULL state buffer" in L.b3gs_last_error()


def test_the_compiled_module_refuses_host_tensors_and_python_side_shapes():
    import torch
    from binocular3dgs_amd import _C, _lib, features
    z = torch.zeros
    u8 = z(64, dtype=torch.uint8)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.feature_render([(u8, u8, u8, 16, 16, z(3, 16, 16))], z(4, 3))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.feature_lift([(u8, u8, u8, 16, 16, z(3, 16, 16), None)], torch.ones(3), z(4, 3, dtype=torch.int64), None)
    with pytest.raises(ValueError):
        _C.feature_render([], z(4, 3))
    s, w = torch.tensor([[2.0, -4.0], [1.0, 1.0], [3.0, 3.0]]), torch.tensor([2.0, 0.0, 0.5])
    assert torch.equal(features.mean_features(s, w), torch.tensor([[1.0, -2.0], [0.0, 0.0], [6.0, 6.0]]))
    assert torch.equal(features.mean_features(s, w, min_weight=1.0), torch.tensor([[1.0, -2.0], [0.0, 0.0], [0.0, 0.0]]))
    f = torch.tensor([[1.0, 0.0], [0.0, 2.0], [0.0, 0.0], [-1.0, 0.1]])
    assert features.similar(f, torch.tensor([3.0, 0.0]), 0.9).tolist() == [True, False, False, False]
    assert features.similar(f, torch.tensor([0.0, 0.0]), -1.0).tolist() == [False] * 4
