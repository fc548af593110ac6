"""b3gs_blend_pixel_maps_batch (csrc/pixelmaps.hip) against tests/pixelmaps_ref.py (float64), through the C ABI.

The forward runs with reference binning; the reference runs on the device's own records and tile lists (debug.state_views), so
projection and binning are out of the comparison (the Device / _View of tests/test_gpu_contrib.py).  Solid pixels are those
whose blend decisions are not fragile in the reference (helpers.FRAGILE_MARGIN), whose two largest weights are no near-tie
(contrib_ref.TIE_THRESHOLD) and which hold no entry with T within pixelmaps_ref.MEDIAN_THRESHOLD of one half.  There
median_depth is bit-equal to the reference's record depth, dominant and count are equal, and depth_m1 / depth_m2 are within
pixelmaps_ref.M1_BOUND / M2_BOUND (10 x the float32 noise of the reference, measured in tests/test_pixelmaps_ref_cpu.py, never
taken from the kernel), relative, with an absolute floor of one float32 ulp of the largest term.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_ref
import contrib_ref
import helpers
import pixelmaps_ref
from helpers import FRAGILE_MARGIN
from test_gpu_contrib import CASES, Device

pytestmark = pytest.mark.gpu
PLANES = pixelmaps_ref.PLANES
SENTINEL_F, SENTINEL_I = -12345.0, -7777
MEDIAN_SCENES = tuple(c for c in CASES if c[0] not in ("stack1", "stack63", "stack64", "stack65"))


def pixel_maps(dev, views, skip=(), outs=None):
    """One call for `views` -> per view a dict of host arrays [H, W] (float32 / int32) of the planes not in `skip` (those get
    a NULL pointer).  Every plane starts filled with a sentinel."""
    if outs is None:
        outs = [{p: torch.full((v.H, v.W), SENTINEL_F if p in PLANES[:3] else SENTINEL_I,
                               dtype=torch.float32 if p in PLANES[:3] else torch.int32, device="cuda") for p in PLANES if p not in skip}
                for v in views]
    arr = (dev.lib.B3gsPixelMapView * len(views))()
    for k, v in enumerate(views):
        arr[k].view = C.pointer(v.scene)
        arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        for p in PLANES:
            setattr(arr[k], p, outs[k][p].data_ptr() if p in outs[k] else None)
    dev.lib.check(dev.L.b3gs_blend_pixel_maps_batch(len(views), arr, dev.stream), "b3gs_blend_pixel_maps_batch")
    torch.cuda.synchronize()
    return [{p: t.cpu().numpy().copy() for p, t in o.items()} for o in outs]


_REF = {}


def _reference(key, got, W, H):
    """float64 blend_ref + pixelmaps_ref on the device's records and lists, once per scene -> (State, maps, solid mask)."""
    if key not in _REF:
        st = blend_ref.forward(got["records"], got["lists"], W, H, got["bg"])
        m = pixelmaps_ref.maps(st)
        _REF[key] = (st, m, pixelmaps_ref.solid_mask(st, m, FRAGILE_MARGIN))
    return _REF[key]


def check_against(name, got, st, m, solid):
    assert (~solid).mean() <= contrib_ref.MASKED_CAP, f"{name}: {(~solid).sum()} pixels left out"
    for p in PLANES:
        assert got[p].shape == (st.H, st.W)
    assert not (got["median_depth"] == np.float32(SENTINEL_F)).any() and not (got["depth_m1"] == np.float32(SENTINEL_F)).any()
    assert not (got["depth_m2"] == np.float32(SENTINEL_F)).any(), f"{name}: a pixel inside the image was not written"
    assert not (got["dominant"] == SENTINEL_I).any() and not (got["count"] == SENTINEL_I).any()
    ref_med = m["median_depth"].astype(np.float32)
    bad = solid & (got["median_depth"].view(np.uint32) != ref_med.view(np.uint32))
    assert not bad.any(), f"{name}: median depth differs at {np.argwhere(bad)[:5].tolist()}"
    for p in ("dominant", "count"):
        bad = solid & (got[p] != m[p])
        assert not bad.any(), f"{name}: {p} differs at {np.argwhere(bad)[:5].tolist()}"
    # floor: one float32 ulp of the largest term of the sum, w d <= d_max (w <= 1), w d d <= d_max^2
    dmax = float(np.abs(np.asarray(st.records)[:, 9]).max())
    ulp = float(np.finfo(np.float32).eps)
    e1 = np.abs(got["depth_m1"].astype(np.float64) - m["depth_m1"])
    e2 = np.abs(got["depth_m2"].astype(np.float64) - m["depth_m2"])
    h = solid & (m["count"] > 0)
    assert h.any()
    print(f"{name}: {int(h.sum())} solid pixels with entries of {solid.size}; largest relative error m1 "
          f"{(e1[h] / m['depth_m1'][h]).max():.2e} m2 {(e2[h] / m['depth_m2'][h]).max():.2e}; "
          f"{len(np.unique(got['median_depth'][h]))} distinct medians")
    assert (e1[solid] <= pixelmaps_ref.M1_BOUND * m["depth_m1"][solid] + ulp * dmax).all(), \
        f"{name}: depth_m1 off by {(e1[h] / m['depth_m1'][h]).max():.2e} (relative)"
    assert (e2[solid] <= pixelmaps_ref.M2_BOUND * m["depth_m2"][solid] + ulp * dmax * dmax).all(), \
        f"{name}: depth_m2 off by {(e2[h] / m['depth_m2'][h]).max():.2e} (relative)"
    empty = solid & (m["count"] == 0)
    assert not got["depth_m1"][empty].any() and not got["depth_m2"][empty].any() and not got["median_depth"][empty].any()
    assert (got["dominant"][empty] == -1).all()


def run_case(d, key, seg1_fraction=0.0):
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v], seg1_fraction=seg1_fraction)
    got = v.state()
    st, m, solid = _reference(key, got, v.W, v.H)
    assert np.array_equal(got["n_contrib"][solid], st.n_contrib[solid])
    return dev, v, got, st, m, solid


@pytest.mark.parametrize("name,W,H", CASES)
def test_pixel_maps_against_float64_reference(name, W, H):
    dev, v, got, st, m, solid = run_case(helpers.blend_scene(name, W, H), f"{name}_{W}x{H}")
    # what the scene is here for, from the device's own lists
    if name.startswith("stack"):
        L = int(name[5:])
        assert len(st.ids[0]) == L and (st.n_contrib[:16, :16] == L).all(), "every pixel of tile 0 blends the whole stack"
        assert (m["count"][:16, :16] == L).all()
    if (name, W, H) in (("cull", 75, 33), ("cull", 72, 41)):
        assert v.W % 16 and v.H % 16
    (r,) = pixel_maps(dev, [v])
    check_against(f"{name} {v.W}x{v.H}", r, st, m, solid)
    if (name, W, H) in MEDIAN_SCENES:
        assert len(np.unique(r["median_depth"][solid & (m["count"] > 0)])) >= 8
    # depth_m1 is the forward's own statement of its depth image
    e = np.abs(r["depth_m1"].astype(np.float64) - v.depth[0].cpu().numpy())
    assert (e <= pixelmaps_ref.M1_BOUND * m["depth_m1"] + np.finfo(np.float32).eps * 8.0)[solid].all()


def test_two_segments_are_both_walked():
    d = helpers.two_segment_scene()
    dev, v, got, st, m, solid = run_case(d, "two_segments", seg1_fraction=0.5)
    assert int(v.flag.item()) == 0
    len1 = got["len1"]
    len2 = np.array([len(a) for a in got["lists"]]) - len1
    helpers.two_segment_populations(len1, len2)
    (r,) = pixel_maps(dev, [v])
    check_against("two segments", r, st, m, solid)
    for t in (0, 3, 4, 5):          # len1 on a word boundary, inside a word, segment 2 only, a list crossing a chunk
        tile = np.s_[0:16, 16 * t:16 * t + 16]
        assert len2[t] > 0 and (st.blended[t][len1[t]:].sum(0) == len2[t]).any(), f"tile {t}: no pixel blends all of segment 2"
        # a pixel cannot count more than len1 entries without walking segment 2
        assert (r["count"][tile] > len1[t]).any(), f"tile {t}: segment 2 was not walked"


def test_three_sizes_in_one_call_equal_three_calls_bit_for_bit():
    ds = helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    assert len({(v.W, v.H) for v in views}) == 3
    singles = [pixel_maps(dev, [v])[0] for v in views]
    assert all((s["count"] > 0).any() for s in singles)
    for order in ((0, 1, 2), (2, 0, 1)):
        got = pixel_maps(dev, [views[i] for i in order])
        for i, g in zip(order, got):
            for p in PLANES:
                assert np.array_equal(g[p].view(np.uint32), singles[i][p].view(np.uint32)), (order, i, p)


def test_a_null_plane_is_skipped_and_its_neighbours_are_written():
    d = helpers.blend_scene("cull", 75, 33)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    (full,) = pixel_maps(dev, [v])
    for skip in (("depth_m1",), ("median_depth", "count"), ("depth_m2", "dominant")):
        # every plane allocated and sentinel-filled, the skipped ones not handed over
        outs = [{p: torch.full((v.H, v.W), SENTINEL_F if p in PLANES[:3] else SENTINEL_I,
                               dtype=torch.float32 if p in PLANES[:3] else torch.int32, device="cuda") for p in PLANES}]
        handed = [{p: t for p, t in outs[0].items() if p not in skip}]
        (r,) = pixel_maps(dev, [v], outs=handed)
        for p in PLANES:
            if p in skip:
                t = outs[0][p].cpu().numpy()
                assert (t == (np.float32(SENTINEL_F) if p in PLANES[:3] else SENTINEL_I)).all(), p
            else:
                assert np.array_equal(r[p].view(np.uint32), full[p].view(np.uint32)), p


def test_the_call_reads_the_forward_state_and_writes_only_its_planes():
    d = helpers.blend_scene("cull", 72, 41)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    state = (v.geom, v.binning, v.img, v.color, v.depth, v.alpha, v.scratch, v.radii)
    before = [t.clone() for t in state]
    (r,) = pixel_maps(dev, [v])
    assert (r["count"] > 0).any()
    for a, b in zip(before, state):
        assert torch.equal(a, b)


def test_two_layers_median_on_the_back_sheet_mean_between():
    d1, d2 = pixelmaps_ref.TWO_LAYER_D1, pixelmaps_ref.TWO_LAYER_D2
    dev, v, got, st, m, solid = run_case(pixelmaps_ref.two_layer_scene(0.3), "two_layer_0.3")
    (r,) = pixel_maps(dev, [v])
    check_against("two layers, front 0.3", r, st, m, solid)
    alpha = v.alpha[0].cpu().numpy()
    covered = (alpha > 0.95) & solid
    assert covered.mean() > 0.85
    med = r["median_depth"][covered]
    assert (med >= d2).all() and (med <= d2 + 0.31).all() and len(np.unique(med)) >= 8
    mean = r["depth_m1"][covered] / alpha[covered]
    assert (mean > d1 + 0.5).all() and (mean < med - 0.2).all()
    dev, v, got, st, m, solid = run_case(pixelmaps_ref.two_layer_scene(0.7), "two_layer_0.7")
    (r,) = pixel_maps(dev, [v])
    check_against("two layers, front 0.7", r, st, m, solid)
    covered = (v.alpha[0].cpu().numpy() > 0.9) & solid
    assert covered.mean() > 0.85 and (r["median_depth"][covered] == np.float32(d1)).all() and (r["dominant"][covered] == 0).all()
