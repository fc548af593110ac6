"""b3gs_feature_render_batch and b3gs_feature_lift_batch (csrc/features.hip) through the C ABI, and binocular3dgs_amd/features.py
end to end.

Exact statements carry no tolerance: the lift of an indicator plane and the weight_q of b3gs_blend_contribution_batch under that
mask are integer sums of the same rint(w 2^32) over the same (pixel, entry); three channels holding a view's record colours
render the bits of its colour planes over a zero background (the forward adds T * bg AFTER the accumulation: fma(T, 0, C) = C)
and a channel of record depths the bits of its depth plane; a channel of a C = 19 call holds the bits of the same channel alone;
a view gives the same bits alone and at any position of a batch.  Random features and maps are compared with
tests/features_ref.py (float64, on the device's own records and lists) on the pixels whose blend decisions are not fragile
(helpers.FRAGILE_MARGIN), within features_ref.RENDER_BOUND / LIFT_BOUND (10 x the float32 noise of the reference, measured in
tests/test_features_ref_cpu.py, never taken from the kernel).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import contrib_ref
import features_ref
import helpers
import segment_ref
from features_ref import LIFT_BOUND, RENDER_BOUND
from helpers import FRAGILE_MARGIN
from test_gpu_contrib import CASES, Device, _reference, check_against, run_case

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 4096          # floats in front of and behind every output buffer: they must keep the sentinel


def feat_render(dev, views, f):
    """One call for `views` -> per view a host float32 [C, H, W]; the planes start sentinel-filled, inside guard zones."""
    f = torch.tensor(np.ascontiguousarray(f, dtype=np.float32), device="cuda")
    assert f.shape[0] == dev.P and f.dim() == 2
    nch = f.shape[1]
    bufs = [torch.full((2 * GUARD + nch * v.H * v.W,), SENTINEL, dtype=torch.float32, device="cuda") for v in views]
    arr = (dev.lib.B3gsFeatureRenderView * len(views))()
    for k, v in enumerate(views):
        arr[k].view = C.pointer(v.scene)
        arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        arr[k].out = bufs[k].data_ptr() + 4 * GUARD
    dev.lib.check(dev.L.b3gs_feature_render_batch(len(views), arr, nch, f.data_ptr(), dev.stream), "b3gs_feature_render_batch")
    torch.cuda.synchronize()
    res = []
    for v, b in zip(views, bufs):
        h = b.cpu().numpy()
        assert (h[:GUARD] == np.float32(SENTINEL)).all() and (h[-GUARD:] == np.float32(SENTINEL)).all(), "a word outside the planes was written"
        res.append(h[GUARD:-GUARD].reshape(nch, v.H, v.W).copy())
    return res


def feat_lift(dev, views, maps, scale, masks=None, out=None, weight=True):
    """One call for `views` (maps: per view [C, H, W]; masks: per view None or [H, W]) -> (host int64 [P, C], host int64 [P] or
    None, the device tensors accumulated into)."""
    nch = np.asarray(maps[0]).shape[0]
    if out is None:
        out = (torch.zeros((dev.P, nch), dtype=torch.int64, device="cuda"), torch.zeros(dev.P, dtype=torch.int64, device="cuda") if weight else None)
    arr = (dev.lib.B3gsFeatureLiftView * len(views))()
    keep = []
    for k, v in enumerate(views):
        arr[k].view = C.pointer(v.scene)
        arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        m = torch.tensor(np.ascontiguousarray(maps[k], dtype=np.float32), device="cuda")
        assert m.shape == (nch, v.H, v.W)
        keep.append(m)
        arr[k].maps = m.data_ptr()
        if masks is not None and masks[k] is not None:
            pm = torch.tensor(np.ascontiguousarray(masks[k]).astype(np.uint8), device="cuda")
            assert pm.shape == (v.H, v.W)
            keep.append(pm)
            arr[k].pixel_mask = pm.data_ptr()
    sc = (C.c_float * nch)(*[float(s) for s in np.asarray(scale, np.float32).reshape(nch)])
    dev.lib.check(dev.L.b3gs_feature_lift_batch(len(views), arr, nch, sc, out[0].data_ptr(), out[1].data_ptr() if out[1] is not None else None,
                                                dev.stream), "b3gs_feature_lift_batch")
    torch.cuda.synchronize()
    del keep
    return out[0].cpu().numpy().copy(), (out[1].cpu().numpy().copy() if out[1] is not None else None), out


def _forward(d):
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    return dev, v


# ---- 1. the lift of an indicator plane is the contribution under that mask ----------------------------------------------------
@pytest.mark.parametrize("name,W,H", CASES)
def test_lift_of_indicator_planes_equals_the_contribution_kernel_bit_for_bit(name, W, H):
    dev, v = _forward(helpers.blend_scene(name, W, H))
    whole = dev.contrib([v])["weight_q"]
    assert whole.sum() > 0
    for kind in segment_ref.PLANES:
        plane, L = segment_ref.label_plane(kind, v.W, v.H)
        ind = np.stack([plane == l for l in range(L)]).astype(np.float32)            # L channels in one call
        sums, wq, _ = feat_lift(dev, [v], [ind], np.ones(L))
        assert np.array_equal(wq, whole), f"{name} / {kind}: weight_q32 is not the unmasked contribution"
        for l in range(L):
            want = dev.contrib([v], [plane == l])["weight_q"]
            assert np.array_equal(sums[:, l], want), f"{name} / {kind}: channel {l} differs at {np.nonzero(sums[:, l] != want)[0][:10]}"
        assert np.array_equal(feat_lift(dev, [v], [-ind], np.ones(L), weight=False)[0], -sums), f"{name} / {kind}: the negative"
        assert np.array_equal(feat_lift(dev, [v], [3.0 * ind], np.full(L, 3.0), weight=False)[0], sums), f"{name} / {kind}: F = 3, scale 3"
        assert np.array_equal(feat_lift(dev, [v], [0.25 * ind], np.full(L, 0.25), weight=False)[0], sums), f"{name} / {kind}: F = scale = 0.25"
    # a mask: the counted pixels are contrib's
    mask = segment_ref.label_plane("checker", v.W, v.H)[0]
    sums, wq, _ = feat_lift(dev, [v], [np.ones((1, v.H, v.W), np.float32)], [1.0], masks=[mask])
    want = dev.contrib([v], [mask])["weight_q"]
    assert np.array_equal(sums[:, 0], want) and np.array_equal(wq, want)


# ---- 2. colours and depths as features are the forward's planes ---------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", CASES)
def test_record_colours_and_depths_render_the_bits_of_the_forward_planes(name, W, H):
    d = dict(helpers.blend_scene(name, W, H))
    d["bg"] = torch.zeros(3)        # out_color = fma(T, bg, C): the accumulated C itself over a zero background
    dev, v = _forward(d)
    rec = v.state()["records"][:, :10].astype(np.float32)
    (planes,) = feat_render(dev, [v], rec[:, 6:10])
    colour, depth = v.color.cpu().numpy(), v.depth.cpu().numpy()
    assert np.abs(colour).sum() > 0 and np.abs(depth).sum() > 0
    assert np.array_equal(planes[:3].view(np.uint32), colour.view(np.uint32)), f"{name}: the colour planes differ"
    assert np.array_equal(planes[3].view(np.uint32), depth[0].view(np.uint32)), f"{name}: the depth plane differs"


# ---- 3. channel counts ------------------------------------------------------------------------------------------------------
_RENDER_REF, _LIFT_REF = {}, {}


def _render_ref(key, st, f):
    if key not in _RENDER_REF:
        _RENDER_REF[key] = features_ref.render(st, f)
    return _RENDER_REF[key]


@pytest.mark.parametrize("name,W,H", CASES)
def test_render_of_19_channels_against_float64_reference(name, W, H):
    dev, v, got, st, c, _solid = run_case(name, W, H)
    f = features_ref.random_features(dev.P, 19)
    (planes,) = feat_render(dev, [v], f)
    assert not (planes == np.float32(SENTINEL)).any(), "a pixel inside the image was not written"
    solid = st.margin >= FRAGILE_MARGIN
    features_ref.check_render(f"{name} {v.W}x{v.H}", planes, _render_ref((name, v.W, v.H, 19), st, f), solid)
    assert not planes[:, solid & (st.n_contrib == 0)].any(), "a pixel that blended nothing holds 0"


@pytest.mark.parametrize("nch", (1, 8, 9, 19))
def test_channel_counts_against_float64_reference(nch):
    dev, v, got, st, c, solid = run_case("cull", 96, 64)
    f = features_ref.random_features(dev.P, nch)
    (planes,) = feat_render(dev, [v], f)
    features_ref.check_render(f"render C = {nch}", planes, _render_ref(("cull", v.W, v.H, nch), st, f), st.margin >= FRAGILE_MARGIN)
    maps = features_ref.random_maps(nch, v.W, v.H)
    scale = features_ref.amax_scale(maps)
    sums, wq, _ = feat_lift(dev, [v], [maps], scale, masks=[solid])
    features_ref.check_lift(f"lift C = {nch}", sums, features_ref.lift(st, maps, scale, solid))
    assert np.array_equal(wq, dev.contrib([v], [solid])["weight_q"])
    # clamping: a scale below the largest |F| clips, as the reference does
    half = (0.5 * scale).astype(np.float32)
    features_ref.check_lift(f"lift C = {nch}, clamped", feat_lift(dev, [v], [maps], half, masks=[solid])[0], features_ref.lift(st, maps, half, solid))


def test_a_channel_of_a_19_channel_call_holds_the_bits_of_the_channel_alone():
    dev, v = _forward(helpers.blend_scene("cull", 75, 33))
    f = features_ref.random_features(dev.P, 19)
    maps = features_ref.random_maps(19, v.W, v.H)
    scale = features_ref.amax_scale(maps)
    (planes,) = feat_render(dev, [v], f)
    sums, _wq, _ = feat_lift(dev, [v], [maps], scale)
    assert np.abs(planes).sum() > 0 and np.abs(sums).sum() > 0
    for ch in range(19):
        (one,) = feat_render(dev, [v], f[:, ch:ch + 1])
        assert np.array_equal(one[0].view(np.uint32), planes[ch].view(np.uint32)), f"render channel {ch}"
        alone = feat_lift(dev, [v], [maps[ch:ch + 1]], scale[ch:ch + 1], weight=False)[0]
        assert np.array_equal(alone[:, 0], sums[:, ch]), f"lift channel {ch}"


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------
def test_three_resolutions_in_one_call_equal_three_calls_in_any_order():
    ds = helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    assert len({(v.W, v.H) for v in views}) == 3
    nch = 11
    f = features_ref.random_features(dev.P, nch)
    maps = [features_ref.random_maps(nch, v.W, v.H) for v in views]
    scale = np.max([features_ref.amax_scale(m) for m in maps], 0)
    singles_r = [feat_render(dev, [v], f)[0] for v in views]
    singles_l = [feat_lift(dev, [v], [m], scale) for v, m in zip(views, maps)]
    assert all(np.abs(s).sum() > 0 for s in singles_r) and all(np.abs(s[0]).sum() > 0 for s in singles_l)
    want_s, want_w = np.sum([s[0] for s in singles_l], 0), np.sum([s[1] for s in singles_l], 0)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 1, 2)):
        sums, wq, _ = feat_lift(dev, [views[i] for i in order], [maps[i] for i in order], scale)
        assert np.array_equal(sums, want_s) and np.array_equal(wq, want_w), order
        for i, planes in zip(order, feat_render(dev, [views[i] for i in order], f)):
            assert np.array_equal(planes.view(np.uint32), singles_r[i].view(np.uint32)), (order, i)
    # ... and accumulated into the same arrays call by call
    out = None
    for v, m in zip(views, maps):
        sums, wq, out = feat_lift(dev, [v], [m], scale, out=out)
    assert np.array_equal(sums, want_s) and np.array_equal(wq, want_w)


# ---- 5. both list segments -------------------------------------------------------------------------------------------------------
def test_two_segments_are_both_walked():
    d = helpers.two_segment_scene()
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v], seg1_fraction=0.5)
    assert int(v.flag.item()) == 0
    got = v.state()
    len1 = got["len1"]
    len2 = np.array([len(a) for a in got["lists"]]) - len1
    helpers.two_segment_populations(len1, len2)
    st, c, solid = _reference("two_segments", got, v.W, v.H)
    assert np.array_equal(got["n_contrib"][solid], st.n_contrib[solid])
    nch = 9
    maps = features_ref.random_maps(nch, v.W, v.H)
    scale = features_ref.amax_scale(maps)
    sums, wq, _ = feat_lift(dev, [v], [maps], scale, masks=[solid])
    features_ref.check_lift("two segments", sums, features_ref.lift(st, maps, scale, solid))
    f = features_ref.random_features(dev.P, nch)
    (planes,) = feat_render(dev, [v], f)
    features_ref.check_render("two segments", planes, features_ref.render(st, f), st.margin >= FRAGILE_MARGIN)
    for t in (0, 3, 4, 5):          # len1 on a word boundary, inside a word, segment 2 only, a list crossing a chunk
        seg2 = got["lists"][t][len1[t]:]
        assert len(seg2) > 0 and (wq[seg2] > 0).all() and (np.abs(sums[seg2]).sum(1) > 0).all(), f"tile {t}: segment 2 was not walked"


# ---- 6. the calls write only their outputs ---------------------------------------------------------------------------------------
def test_the_calls_read_the_forward_state_and_write_only_their_outputs():
    dev, v = _forward(helpers.blend_scene("cull", 75, 33))        # partial tiles on both edges
    state = (v.geom, v.binning, v.img, v.color, v.depth, v.alpha, v.scratch, v.radii)
    before = [t.clone() for t in state]
    f = features_ref.random_features(dev.P, 9)
    (planes,) = feat_render(dev, [v], f)                            # (checks the guard zones around the planes)
    maps = features_ref.random_maps(9, v.W, v.H)
    sums, wq, _ = feat_lift(dev, [v], [maps], features_ref.amax_scale(maps))
    assert np.abs(sums).sum() > 0 and wq.sum() > 0
    for a, b in zip(before, state):
        assert torch.equal(a, b)
    assert not (planes == np.float32(SENTINEL)).any(), "a pixel inside the image was not written"
    assert not planes[:, v.state()["n_contrib"] == 0].any(), "pixels that blended nothing hold 0"
    dev2, v2 = _forward(helpers.blend_scene("stack65"))              # tile 3 of a stack scene is empty
    (planes2,) = feat_render(dev2, [v2], features_ref.random_features(dev2.P, 9))
    empty = v2.state()["n_contrib"] == 0
    assert empty[:, 48:].all() and np.abs(planes2).sum() > 0 and not planes2[:, empty].any(), "pixels that blended nothing hold 0"
    # without the optional array nothing else is written either, and the sums are the same
    again = feat_lift(dev, [v], [maps], features_ref.amax_scale(maps), weight=False)[0]
    assert np.array_equal(again, sums)


# ---- 7. the pair is adjoint on the device ------------------------------------------------------------------------------------------
def test_render_and_lift_are_adjoint_on_the_device():
    for name, W, H, nch in (("cull", 96, 64, 19), ("stack257", None, None, 3)):
        dev, v = _forward(helpers.blend_scene(name, W, H))
        f = features_ref.random_features(dev.P, nch)
        maps = features_ref.random_maps(nch, v.W, v.H)
        scale = features_ref.amax_scale(maps)
        (planes,) = feat_render(dev, [v], f)
        (size,) = feat_render(dev, [v], np.abs(f))
        sums, _wq, _ = feat_lift(dev, [v], [maps], scale, weight=False)
        lifted = sums.astype(np.float64) / features_ref.Q32 * scale.astype(np.float64)[None, :]
        lhs = float((planes.astype(np.float64) * maps.astype(np.float64)).sum())
        rhs = float((f.astype(np.float64) * lifted).sum())
        bound = (RENDER_BOUND + LIFT_BOUND) * float((np.abs(maps).astype(np.float64) * size.astype(np.float64)).sum())
        print(f"{name}: <render(f), F> = {lhs:.9e}, <f, lift(F)> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
        assert bound > 0 and abs(lhs - rhs) <= bound


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    dev, v = _forward(helpers.blend_scene("stack1"))
    L, lib = dev.L, dev.lib
    f = torch.zeros((dev.P, 300), device="cuda")
    out = torch.zeros(300 * v.H * v.W, device="cuda")
    sums = torch.zeros((dev.P, 300), dtype=torch.int64, device="cuda")
    rv = (lib.B3gsFeatureRenderView * 2)()
    lv = (lib.B3gsFeatureLiftView * 2)()
    other = lib.B3gsScene()
    other.P, other.W, other.H = dev.P + 1, v.W, v.H
    for k, sc in enumerate((v.scene, other)):
        for a in (rv[k], lv[k]):
            a.view = C.pointer(sc)
            a.geometry, a.binning, a.image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        rv[k].out, lv[k].maps = out.data_ptr(), out.data_ptr()
    ones = (C.c_float * 300)(*([1.0] * 300))
    for nch in (0, 257):
        assert L.b3gs_feature_render_batch(1, rv, nch, f.data_ptr(), dev.stream) == -1 and b"channels" in L.b3gs_last_error()
        assert L.b3gs_feature_lift_batch(1, lv, nch, ones, sums.data_ptr(), None, dev.stream) == -1 and b"channels" in L.b3gs_last_error()
    assert L.b3gs_feature_render_batch(1, None, 3, f.data_ptr(), dev.stream) == -1
    assert L.b3gs_feature_render_batch(1, rv, 3, None, dev.stream) == -1
    assert L.b3gs_feature_lift_batch(1, None, 3, ones, sums.data_ptr(), None, dev.stream) == -1
    assert L.b3gs_feature_lift_batch(1, lv, 3, None, sums.data_ptr(), None, dev.stream) == -1
    assert L.b3gs_feature_lift_batch(1, lv, 3, ones, None, None, dev.stream) == -1
    assert L.b3gs_feature_render_batch(2, rv, 3, f.data_ptr(), dev.stream) == -1 and b"share P" in L.b3gs_last_error()
    assert L.b3gs_feature_lift_batch(2, lv, 3, ones, sums.data_ptr(), None, dev.stream) == -1 and b"share P" in L.b3gs_last_error()
    for bad in (0.0, -2.0):
        s = (C.c_float * 3)(1.0, bad, 1.0)
        assert L.b3gs_feature_lift_batch(1, lv, 3, s, sums.data_ptr(), None, dev.stream) == -1 and b"scale" in L.b3gs_last_error()
    torch.cuda.synchronize()
    assert not sums.any() and not out.any()
    with pytest.raises(lib.B3gsError, match="b3gs_feature_render_batch failed: B3GS_ERR_ARG"):
        lib.check(L.b3gs_feature_render_batch(1, rv, 0, f.data_ptr(), dev.stream), "b3gs_feature_render_batch")


# ---- 9. binocular3dgs_amd/features.py end to end ----------------------------------------------------------------------------------
E2E_SIZE = (96, 64)
LEFT, RIGHT = (1.0, 0.5, 0.0, -1.0), (-0.5, 1.0, 2.0, 0.25)


def _two_clusters():
    """The two-cluster scene of tests/test_gpu_segment.py, rebuilt: 96 x 64, 300 small flat splats (shortest axis z) on each side
    of an empty slab around x = 0 -- no footprint reaches the other side -- as a GaussianModel, three cameras on the z axis
    looking down +z (the plane x = 0 is the centre column of every one) and one behind the sheet looking down -z."""
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.camera import Camera
    from binocular3dgs_amd.gaussian_model import GaussianModel
    W, H = E2E_SIZE
    rng = np.random.RandomState(helpers.hash_name("two_clusters"))
    n = 300
    x = np.concatenate([rng.uniform(3, 38, n), rng.uniform(57, 92, n)])
    d = helpers.splat_scene(W, H, x=x, y=rng.uniform(3, H - 4, 2 * n), sig_a=rng.uniform(0.8, 2.1, 2 * n), sig_b=rng.uniform(0.8, 2.1, 2 * n),
                            theta=rng.uniform(0, np.pi, 2 * n), opacity=rng.uniform(0.2, 0.9, 2 * n), colour=rng.uniform(0.05, 0.95, (2 * n, 3)),
                            z=rng.uniform(3.0, 5.0, 2 * n))
    op = d["opacities"].double().reshape(-1, 1)
    model = GaussianModel.from_tensors(d["means3D"].float(), d["shs"][:, :1].float(), torch.zeros(2 * n, 3, 3),
                                       torch.log(d["scales"].double()).float(), d["rotations"].float(), torch.log(op / (1 - op)).float(),
                                       sh_degree=1, active_sh_degree=1, device="cuda", requires_grad=False)
    fovy = synth.fovy_from(helpers.BLEND_FOVX, W, H)
    cams = [Camera(np.eye(3), np.array([0.0, 0.0, -c]), helpers.BLEND_FOVX, fovy, W, H, device="cuda") for c in (0.0, -0.6, 0.5)]
    behind = Camera(np.diag([-1.0, 1.0, -1.0]), np.array([0.0, 0.0, 8.0]), helpers.BLEND_FOVX, fovy, W, H, device="cuda")
    side = (d["means3D"][:, 0] > 0).to(torch.uint8)
    assert int(side.sum()) == n
    return model, cams, behind, d["bg"].float().cuda(), side.cuda()


def _cluster_maps(n):
    W, H = E2E_SIZE
    right = (torch.arange(W) >= W // 2).expand(H, W)
    m = torch.where(right.unsqueeze(0), torch.tensor(RIGHT).view(4, 1, 1), torch.tensor(LEFT).view(4, 1, 1)).contiguous()
    return [m.cuda() if k % 2 == 0 else m.clone() for k in range(n)]          # (host maps are taken too)


def test_features_module_end_to_end_on_two_clusters():
    from binocular3dgs_amd import features, importance
    model, cams, behind, bg, side = _two_clusters()
    W, H = E2E_SIZE
    P = side.shape[0]
    maps = _cluster_maps(3)
    sums, weight = features.lift_features(model, cams, bg, maps)
    assert sums.shape == (P, 4) and weight.shape == (P,) and sums.dtype == weight.dtype == torch.float32 and sums.is_cuda
    con = importance.contributions(model, cams, bg)
    assert torch.equal(weight, con.weight.float())
    seen = weight > 0
    assert int(seen.sum()) > 0.9 * P
    mean = features.mean_features(sums, weight)
    want = torch.where(side.bool().unsqueeze(1), torch.tensor(RIGHT, device="cuda"), torch.tensor(LEFT, device="cuda"))
    scale = torch.tensor([1.0, 1.0, 2.0, 1.0], device="cuda").double()              # the default: the largest |F| per channel
    # per blended entry one float32 rounding of w * Fn (far inside LIFT_BOUND) and two quantisations of 2^-33 (sum and weight);
    # the float32 results round once more each
    hits = con.hits.double()
    tol = (LIFT_BOUND + 4 * 2.0 ** -24) * scale.unsqueeze(0) + (2.0 * hits * 2.0 ** -32 / con.weight.clamp(min=1e-30)).unsqueeze(1) * scale.unsqueeze(0)
    err = (mean.double() - want.double()).abs()
    print(f"two clusters: {int(seen.sum())} of {P} Gaussians seen, largest error of the mean feature {float(err[seen].max()):.2e}")
    assert bool((err[seen] <= tol[seen]).all()) and not bool(mean[~seen].any())
    assert torch.equal(features.similar(mean, torch.tensor(RIGHT), 0.99)[seen], side.bool()[seen])
    assert torch.equal(features.similar(mean, torch.tensor(LEFT), 0.99)[seen], ~side.bool()[seen])
    # the batch size and the order change nothing; a camera without a map is skipped; a mask counts only its pixels
    q = features.lift_features_q32(model, cams, bg, maps)
    for other in (features.lift_features_q32(model, cams, bg, maps, batch=1),
                  features.lift_features_q32(model, cams[::-1] + [cams[0]], bg, maps[::-1] + [None])):
        assert torch.equal(other[0], q[0]) and torch.equal(other[1], q[1])
    none = features.lift_features(model, cams, bg, maps, masks=[torch.zeros(H, W)] * 3)
    assert not bool(none[0].any()) and not bool(none[1].any())
    with pytest.raises(ValueError, match="not finite"):
        features.lift_features(model, cams, bg, [maps[0], maps[1], maps[2] * float("nan")])
    with pytest.raises(ValueError):
        features.lift_features(model, cams, bg, maps[:2])
    with pytest.raises(ValueError, match="scale"):
        features.lift_features(model, cams, bg, maps, scale=[1.0, 0.0, 1.0, 1.0])
    # render: the mean features paint their cluster's vector wherever the pixel is opaque enough to say so
    seen_cams = []
    for i, planes in features.render_features(model, cams, mean):
        seen_cams.append(i)
        assert planes.shape == (4, H, W) and planes.dtype == torch.float32
        left = planes[:, :, :W // 2]
        assert float(planes.abs().sum()) > 0 and bool((left[2] == 0).all()), "channel 2 of the left cluster's vector is 0"
    assert sorted(seen_cams) == [0, 1, 2]
    qv = features.feature_under(model, cams[0], mean, *_painted_pixel(features, model, cams[0], mean, right=True))
    assert abs(float((qv * qv).sum()) - 1.0) < 1e-5
    assert torch.equal(features.similar(mean, qv, 0.99)[seen], side.bool()[seen])


def _painted_pixel(features, model, cam, f, right):
    """(x, y) of the pixel of the wanted half with the largest rendered magnitude."""
    ((_i, planes),) = list(features.render_features(model, [cam], f))
    mag = (planes * planes).sum(0)
    W = mag.shape[1]
    mag[:, :W // 2] = mag[:, :W // 2] * (0.0 if right else 1.0)
    mag[:, W // 2:] = mag[:, W // 2:] * (1.0 if right else 0.0)
    k = int(mag.argmax())
    return k % W, k // W


def test_feature_render_autograd_is_the_lift():
    from binocular3dgs_amd import features
    model, cams, _behind, bg, _side = _two_clusters()
    P = model.get_xyz.shape[0]
    f = torch.tensor(features_ref.random_features(P, 5), device="cuda", requires_grad=True)
    gen = torch.Generator().manual_seed(5)
    F = (torch.rand((3, 5, E2E_SIZE[1], E2E_SIZE[0]), generator=gen) * 2 - 1).cuda()
    out = features.feature_field(model, cams)(f)
    assert out.shape == F.shape
    for i, planes in features.render_features(model, cams, f):
        assert torch.equal(out[i], planes)
    (grad,) = torch.autograd.grad((out * F).sum(), f)
    sums, _w = features.lift_features(model, cams, bg, [F[i] for i in range(3)])
    assert float(sums.abs().sum()) > 0 and torch.equal(grad, sums)
    # a few steps of gradient descent on frozen geometry lower a 2D loss
    target = torch.stack([m.cuda() for m in _cluster_maps(3)])
    feat = torch.zeros((P, 4), device="cuda", requires_grad=True)
    opt = torch.optim.Adam([feat], lr=0.05)
    field = features.feature_field(model, cams)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = ((field(feat) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]


def test_normals_of_a_fronto_parallel_sheet():
    from binocular3dgs_amd import features
    model, cams, behind, _bg, _side = _two_clusters()
    n = features.gaussian_normals(model)
    assert n.shape == (model.get_xyz.shape[0], 3) and bool(((n[:, 2].abs() - 1).abs() < 1e-6).all())
    res = list(features.render_normals(model, [cams[0], behind]))
    assert [r[0] for r in res] == [0, 1]
    for (i, normals, valid), z in zip(res, (-1.0, 1.0)):
        assert normals.shape == (3, E2E_SIZE[1], E2E_SIZE[0]) and valid.dtype == torch.bool
        assert int(valid.sum()) > valid.numel() // 10, f"camera {i} sees the sheet"
        want = torch.tensor([0.0, 0.0, z], device="cuda").view(3, 1)
        assert float((normals[:, valid] - want).abs().max()) <= 1e-5
        assert not bool(normals[:, ~valid].any())


def test_command_line(tmp_path, capsys):
    import json
    import os
    import shutil
    from binocular3dgs_amd import features, frames
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.init_points import load_ply
    from binocular3dgs_amd.scene import Scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = shutil.copytree(os.path.join(root, "tests", "golden", "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "model"
    np.random.seed(0)
    model = GaussianModel(1)
    scene = Scene.from_dataset(str(src), model, eval=True, n_views=3, dataset_name="LLFF", resolution=1, init_points="sparse",
                               model_path=str(out), shuffle=False)
    scene.save(7)
    P = model.get_xyz.shape[0]
    with open(out / "cfg_args", "w") as fp:
        fp.write(f"Namespace(source_path={str(src)!r}, images='images', eval=True, n_views=3, dataset_name='LLFF', resolution=1, "
                 "white_background=False, sh_degree=1, init_points='sparse')")
    cams = list(scene.getTrainCameras())
    n_test = len(list(scene.getTestCameras()))
    W, H = int(cams[0].image_width), int(cams[0].image_height)
    # 5-channel maps at a quarter of the size for two of the three training cameras: left half one vector, right half another
    maps_dir = tmp_path / "maps"
    os.makedirs(maps_dir)
    h, w = max(H // 4, 2), max(W // 4, 2)
    m = np.zeros((5, h, w), np.float32)
    m[:, :, :w // 2] = np.array([1, 0, 0, 0.5, -1], np.float32).reshape(5, 1, 1)
    m[:, :, w // 2:] = np.array([0, 1, 2, -0.5, 1], np.float32).reshape(5, 1, 1)
    for cam in cams[:2]:
        np.save(maps_dir / (str(cam.image_name) + ".npy"), m)
    feat = str(tmp_path / "features.npy")
    assert features.main(["-m", str(out), "lift", "--maps", str(maps_dir), "--out", feat]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["P"] == P and res["C"] == 5 and res["views"] == 2 and 0 < res["seen"] <= P
    f = np.load(feat)
    assert f.shape == (P, 5) and f.dtype == np.float32 and np.isfinite(f).all() and int((np.abs(f).sum(1) > 0).sum()) == res["seen"]
    pics = tmp_path / "pics"
    assert features.main(["-m", str(out), "render", "--features", feat, "--views", "test", "--out", str(pics), "--channels", "0", "1", "2"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["rendered"] == n_test > 0
    assert sorted(os.listdir(pics)) == sorted(["feature_%05d.npy" % i for i in range(n_test)] + ["feature_%05d.png" % i for i in range(n_test)])
    planes = np.load(pics / "feature_00000.npy")
    assert planes.shape[0] == 5 and planes.dtype == np.float32 and np.abs(planes).sum() > 0
    assert frames.read_png(str(pics / "feature_00000.png")).shape == planes.shape[1:] + (3,)
    nrm = tmp_path / "normals"
    assert features.main(["-m", str(out), "normals", "--views", "test", "--out", str(nrm)]) == 0
    capsys.readouterr()
    assert sorted(os.listdir(nrm)) == ["normal_%05d.png" % i for i in range(n_test)]
    assert frames.read_png(str(nrm / "normal_00000.png")).shape == planes.shape[1:] + (3,)
    # select: the pixel of the first training view with the largest rendered magnitude
    loaded = GaussianModel(1)
    loaded.load_ply(str(out / "point_cloud" / "iteration_7" / "point_cloud.ply"))
    x, y = _painted_pixel(features, loaded, cams[0], torch.from_numpy(f), right=True)
    new = tmp_path / "selected"
    assert features.main(["-m", str(out), "select", "--features", feat, "--view", str(cams[0].image_name), "--pixel", str(x), str(y),
                          "--threshold", "0.9", "--model_out", str(new)]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["P_before"] == P and 0 < res["P_after"] < P
    part = load_ply(str(new / "point_cloud" / "iteration_7" / "point_cloud.ply"), 1)
    assert part._xyz.shape[0] == res["P_after"] and os.path.exists(new / "cfg_args")
    with pytest.raises(SystemExit):
        features.main(["-m", str(out)])                                                     # no command
