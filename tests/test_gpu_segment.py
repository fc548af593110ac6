"""b3gs_label_votes_batch and b3gs_label_render_batch (csrc/segment.hip) through the C ABI, and binocular3dgs_amd/segment.py
end to end.

Votes: both they and the weight_q of b3gs_blend_contribution_batch under pixel_mask = (labels == l) are integer sums of the
same rint(w 2^32) over the same (pixel, entry) -- equal bit for bit, no tolerance -- on the thirteen scenes of
tests/test_gpu_contrib.py under five label planes (segment_ref.label_plane).  One float64 anchor ties the chain to
tests/segment_ref.py.  Label render: against segment_ref.label_render (float64, on the device's own records and lists) on the
pixels whose blend decisions are not fragile (helpers.FRAGILE_MARGIN) and whose two largest label sums are no near-tie
(contrib_ref.TIE_THRESHOLD): `label` equal exactly, `weight` within segment_ref.LABEL_WEIGHT_BOUND (10 x the float32 noise of the
reference, measured in tests/test_segment_ref_cpu.py, never taken from the kernel), relative, plus one float32 ulp of 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import contrib_ref
import helpers
import segment_ref
from helpers import BLEND_IMG_BOUND, FRAGILE_MARGIN
from test_gpu_contrib import CASES, Device, check_against, run_case

pytestmark = pytest.mark.gpu
SENTINEL_L, SENTINEL_W = 77, -12345.0


def label_votes(dev, views, planes, L, out=None):
    """One call for `views` (planes: per view a uint8 [H, W] array) -> (host int64 [P, L], the device tensor accumulated into)."""
    if out is None:
        out = torch.zeros((dev.P, L), dtype=torch.int64, device="cuda")
    arr = (dev.lib.B3gsLabelVoteView * len(views))()
    keep = []
    for k, v in enumerate(views):
        arr[k].view = C.pointer(v.scene)
        arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        m = torch.tensor(np.ascontiguousarray(planes[k], dtype=np.uint8), device="cuda")
        assert m.shape == (v.H, v.W)
        keep.append(m)
        arr[k].labels = m.data_ptr()
    dev.lib.check(dev.L.b3gs_label_votes_batch(len(views), arr, L, out.data_ptr(), dev.stream), "b3gs_label_votes_batch")
    torch.cuda.synchronize()
    del keep
    return out.cpu().numpy().copy(), out


def label_render(dev, views, gl, L):
    """One call for `views` -> per view (label uint8 [H, W], weight float32 [H, W]) host arrays; both start sentinel-filled."""
    g = torch.tensor(np.ascontiguousarray(gl, dtype=np.uint8), device="cuda")
    assert g.shape == (dev.P,)
    outs = [(torch.full((v.H, v.W), SENTINEL_L, dtype=torch.uint8, device="cuda"),
             torch.full((v.H, v.W), SENTINEL_W, dtype=torch.float32, device="cuda")) for v in views]
    arr = (dev.lib.B3gsLabelRenderView * len(views))()
    for k, v in enumerate(views):
        arr[k].view = C.pointer(v.scene)
        arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
        arr[k].label, arr[k].weight = outs[k][0].data_ptr(), outs[k][1].data_ptr()
    dev.lib.check(dev.L.b3gs_label_render_batch(len(views), arr, L, g.data_ptr(), dev.stream), "b3gs_label_render_batch")
    torch.cuda.synchronize()
    return [(a.cpu().numpy().copy(), b.cpu().numpy().copy()) for a, b in outs]


def _forward(d):
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    return dev, v


# ---- votes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", CASES)
def test_votes_equal_the_contribution_kernel_under_each_label_mask(name, W, H):
    dev, v = _forward(helpers.blend_scene(name, W, H))
    whole = dev.contrib([v])
    assert whole["hits"].sum() > 0
    for kind in segment_ref.PLANES:
        plane, L = segment_ref.label_plane(kind, v.W, v.H)
        votes, _ = label_votes(dev, [v], [plane], L)
        assert votes.shape == (dev.P, L) and votes.sum() > 0
        for l in range(L):
            want = dev.contrib([v], [plane == l])["weight_q"]
            assert np.array_equal(votes[:, l], want), f"{name} / {kind}: label {l} differs at {np.nonzero(votes[:, l] != want)[0][:10]}"
        labelled = whole["weight_q"] if (plane < L).all() else dev.contrib([v], [plane < L])["weight_q"]
        assert np.array_equal(votes.sum(1), labelled), f"{name} / {kind}: the votes do not add up to the contribution"
        if kind in ("checker", "stripes"):
            assert (votes > 0).any(0).all(), f"{name} / {kind}: a label without a vote"
    none, _ = label_votes(dev, [v], [np.full((v.H, v.W), 255, np.uint8)], 16)
    assert not none.any(), "no pixel carries a label: nothing is walked"


def test_votes_against_the_float64_reference():
    dev, v, got, st, c, solid = run_case("cull", 96, 64)
    plane, L = segment_ref.label_plane("draw5", v.W, v.H)
    plane = np.where(solid, plane, 255).astype(np.uint8)
    votes, _ = label_votes(dev, [v], [plane], L)
    ref_votes = segment_ref.votes(st, plane, L)
    for l in range(L):
        ref = contrib_ref.contributions(st, plane == l)
        assert np.array_equal(ref["weight_q"], ref_votes[:, l]) and ref["hits"].sum() > 0
        g = dev.contrib([v], [plane == l])       # hits, dominant, wmax of the same mask; the weight is the vote column
        g["weight_q"] = votes[:, l]
        check_against(f"cull 96x64, label {l}", g, ref)


def test_three_resolutions_in_one_call_equal_three_calls_in_any_order():
    ds = helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    assert len({(v.W, v.H) for v in views}) == 3
    planes = [segment_ref.label_plane("draw16", v.W, v.H)[0] for v in views]
    singles = [label_votes(dev, [v], [p], 16)[0] for v, p in zip(views, planes)]
    assert all(s.sum() > 0 for s in singles)
    want = np.sum(singles, 0)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 1, 2)):
        got, _ = label_votes(dev, [views[i] for i in order], [planes[i] for i in order], 16)
        assert np.array_equal(got, want), order
    # ... and accumulated into the same array call by call
    out = None
    for v, p in zip(views, planes):
        acc, out = label_votes(dev, [v], [p], 16, out=out)
    assert np.array_equal(acc, want)


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
    plane, L = segment_ref.label_plane("stripes", v.W, v.H)
    votes, _ = label_votes(dev, [v], [plane], L)
    for l in range(L):
        assert np.array_equal(votes[:, l], dev.contrib([v], [plane == l])["weight_q"])
    for t in (0, 3, 4, 5):          # len1 on a word boundary, inside a word, segment 2 only, a list crossing a chunk
        seg2 = got["lists"][t][len1[t]:]
        assert len(seg2) > 0 and (votes[seg2].sum(1) > 0).all(), f"tile {t}: a Gaussian of segment 2 received no vote"


def test_the_calls_read_the_forward_state_and_write_only_their_outputs():
    dev, v = _forward(helpers.blend_scene("cull", 72, 41))
    state = (v.geom, v.binning, v.img, v.color, v.depth, v.alpha, v.scratch, v.radii)
    before = [t.clone() for t in state]
    votes, _ = label_votes(dev, [v], [segment_ref.label_plane("draw16", v.W, v.H)[0]], 16)
    ((label, weight),) = label_render(dev, [v], *segment_ref.gaussian_labeling("mod16", dev.P))
    assert votes.sum() > 0 and (weight > 0).any()
    for a, b in zip(before, state):
        assert torch.equal(a, b)


# ---- label render ---------------------------------------------------------------------------------------------------------
_RENDER_REF = {}


def _render_ref(key, st, gl, L):
    if key not in _RENDER_REF:
        _RENDER_REF[key] = segment_ref.label_render(st, gl, L)
    return _RENDER_REF[key]


def check_render(name, label, weight, st, r):
    solid = segment_ref.solid_mask(st, r, FRAGILE_MARGIN)
    assert (~solid).mean() <= contrib_ref.MASKED_CAP, f"{name}: {(~solid).sum()} pixels left out"
    assert label.shape == weight.shape == (st.H, st.W)
    assert not (weight == np.float32(SENTINEL_W)).any(), f"{name}: a pixel inside the image was not written"
    bad = solid & (label.astype(np.int64) != r["label"])
    assert not bad.any(), f"{name}: label differs at {np.argwhere(bad)[:5].tolist()}"
    err = np.abs(weight.astype(np.float64) - r["weight"])
    h = solid & (r["weight"] > 0)
    assert h.any()
    print(f"{name}: {int(h.sum())} solid pixels with a label of {solid.size}, {len(np.unique(label[h]))} labels seen; largest "
          f"relative error of the winning sum {(err[h] / r['weight'][h]).max():.2e}")
    assert (err[solid] <= segment_ref.LABEL_WEIGHT_BOUND * r["weight"][solid] + segment_ref.LABEL_WEIGHT_FLOOR).all(), \
        f"{name}: weight off by {(err[h] / r['weight'][h]).max():.2e} (relative)"
    empty = solid & (r["weight"] == 0)
    assert (label[empty] == 255).all() and not weight[empty].any()


@pytest.mark.parametrize("name,W,H", CASES)
def test_label_render_against_float64_reference(name, W, H):
    dev, v, got, st, c, _solid = run_case(name, W, H)
    for labeling in segment_ref.labelings_for(name):
        gl, L = segment_ref.gaussian_labeling(labeling, dev.P)
        r = _render_ref((name, v.W, v.H, labeling), st, gl, L)
        ((label, weight),) = label_render(dev, [v], gl, L)
        check_render(f"{name} {v.W}x{v.H} / {labeling}", label, weight, st, r)
        if labeling == "mod16" and name == "cull":
            assert len(np.unique(label[label != 255])) >= 8


def test_no_labelled_gaussian_leaves_every_pixel_unlabelled():
    dev, v = _forward(helpers.blend_scene("cull", 75, 33))
    for L in (1, 3, 16):
        ((label, weight),) = label_render(dev, [v], np.full(dev.P, 255, np.uint8), L)
        assert (label == 255).all() and not weight.any()
    ((label, weight),) = label_render(dev, [v], np.full(dev.P, 7, np.uint8), 5)       # 7 >= L: no label either
    assert (label == 255).all() and not weight.any()


def test_a_single_label_is_the_count_plane_and_the_alpha_image():
    from test_gpu_pixelmaps import pixel_maps
    for name, W, H in (("cull", 75, 33), ("stack257", None, None)):
        dev, v = _forward(helpers.blend_scene(name, W, H))
        ((label, weight),) = label_render(dev, [v], np.zeros(dev.P, np.uint8), 1)
        (maps,) = pixel_maps(dev, [v])
        assert (maps["count"] > 0).any()
        assert np.array_equal(label == 0, maps["count"] > 0) and (label[maps["count"] == 0] == 255).all()
        alpha = v.alpha[0].cpu().numpy()
        assert (np.abs(weight.astype(np.float64) - alpha) <= BLEND_IMG_BOUND).all()


def _sixteen_splats():
    """48 x 32: sixteen overlapping splats of mixed size and opacity -- label = index makes every label sum ONE weight."""
    rng = np.random.RandomState(helpers.hash_name("sixteen_splats"))
    n = 16
    return helpers.splat_scene(48, 32, x=rng.uniform(4, 44, n), y=rng.uniform(4, 28, n), sig_a=rng.uniform(3, 9, n), sig_b=rng.uniform(2, 6, n),
                               theta=rng.uniform(0, np.pi, n), opacity=rng.uniform(0.15, 0.7, n), colour=rng.uniform(0.05, 0.95, (n, 3)),
                               z=2.0 + 0.1 * rng.permutation(n))


def test_label_equal_to_index_renders_the_dominant_plane():
    from test_gpu_contrib import _reference
    from test_gpu_pixelmaps import pixel_maps
    d = _sixteen_splats()
    dev, v = _forward(d)
    assert dev.P == 16
    got = v.state()
    st, c, solid = _reference("sixteen_splats", got, v.W, v.H)
    assert (~solid).mean() <= contrib_ref.MASKED_CAP
    ((label, weight),) = label_render(dev, [v], np.arange(16, dtype=np.uint8), 16)
    (maps,) = pixel_maps(dev, [v])
    dom = np.where(maps["dominant"] < 0, 255, maps["dominant"])
    assert len(np.unique(dom[solid])) >= 4 and (maps["count"][solid] >= 2).any()
    assert np.array_equal(label[solid].astype(np.int64), dom[solid].astype(np.int64))


def test_a_view_gives_the_same_bits_alone_and_at_each_position_of_a_batch():
    ds = helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    gl, L = segment_ref.gaussian_labeling("mod16", dev.P)
    singles = [label_render(dev, [v], gl, L)[0] for v in views]
    assert all((s[1] > 0).any() for s in singles)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got = label_render(dev, [views[i] for i in order], gl, L)
        for i, (label, weight) in zip(order, got):
            assert np.array_equal(label, singles[i][0]), (order, i)
            assert np.array_equal(weight.view(np.uint32), singles[i][1].view(np.uint32)), (order, i)


# ---- binocular3dgs_amd/segment.py end to end --------------------------------------------------------------------------
E2E_SIZE = (96, 64)


def _two_clusters():
    """96 x 64: 300 small splats on each side of an empty slab around x = 0 -- centres at least 9.5 pixels from the centre
    column, sigma at most 2.1 pixels, so that no footprint (alpha >= 1/255: within 3.4 sigma) reaches the other side -- as a
    GaussianModel, with three cameras on the z axis looking down +z: the plane x = 0 is the centre column of every one."""
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
    side = (d["means3D"][:, 0] > 0).to(torch.uint8)
    assert int(side.sum()) == n and float(d["means3D"][:, 0].abs().min()) > 0
    return model, cams, d["bg"].float().cuda(), side.cuda()


def test_segment_module_end_to_end_on_two_clusters():
    from binocular3dgs_amd import segment
    model, cams, bg, side = _two_clusters()
    W, H = E2E_SIZE
    plane = (torch.arange(W) >= W // 2).to(torch.uint8).expand(H, W).contiguous()      # column left or right of the plane x = 0
    planes = [plane.cuda(), plane.clone(), plane.cuda()]                                # (host planes are taken too)
    votes = segment.label_votes(model, cams, bg, planes, 2)
    P = side.shape[0]
    assert votes.shape == (P, 2) and votes.dtype == torch.int64 and votes.is_cuda
    voted = votes.sum(1) > 0
    assert int(voted.sum()) > 0.9 * P
    gl = segment.assign_labels(votes)
    assert gl.dtype == torch.uint8 and torch.equal(gl[voted], side[voted]), "every Gaussian that was seen takes its side's label"
    assert bool((gl[~voted] == 255).all())
    # the wrong side holds no vote at all: no footprint crosses the centre column
    assert not bool(votes.gather(1, (1 - side).long().unsqueeze(1)).any())
    part = segment.extract(model, gl, keep=[1])
    rows = gl == 1
    assert int(rows.sum()) > 0 and torch.equal(part._xyz.detach(), model._xyz.detach()[rows])
    assert torch.equal(part._opacity.detach(), model._opacity.detach()[rows])
    total = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
    seen = []
    for i, r in segment.render_labels(model, cams, bg, gl, 2):
        seen.append(i)
        assert r["label"].shape == (H, W) and r["label"].dtype == torch.uint8 and r["weight"].dtype == torch.float32
        assert r["rendered_alpha"].shape == (1, H, W)
        painted = r["weight"] > 0
        assert int(painted.sum()) > H * W // 10
        assert torch.equal(r["label"][painted], plane.cuda()[painted]), f"camera {i}: a pixel shows the other side's label"
        assert bool((r["label"][~painted] == 255).all())
        # scored on the pixels something was rendered into: there the re-rendered labels are the given ones
        given = torch.where(painted, plane.cuda(), torch.full_like(plane.cuda(), 255))
        total += segment.label_iou(r["label"], given, 2)
    assert sorted(seen) == [0, 1, 2]
    assert bool((total[:, 0] == total[:, 1]).all()) and bool((total[:, 0] > 0).all())
    # a camera without a plane changes nothing; the batch size changes nothing
    more = segment.label_votes(model, cams + [cams[1]], bg, planes + [None], 2)
    assert torch.equal(more, votes)
    assert torch.equal(segment.label_votes(model, cams, bg, planes, 2, batch=1), votes)
    assert not bool(segment.label_votes(model, cams, bg, [None, None, None], 2).any())
    # the votes are the contribution under each label's mask
    from binocular3dgs_amd import importance
    for l in (0, 1):
        w = importance.contributions(model, cams, bg, masks=[(p == l) for p in planes]).weight
        assert torch.equal(w, votes[:, l].double() / 2 ** 32)
    with pytest.raises(ValueError):
        segment.label_votes(model, cams, bg, planes[:2], 2)
    with pytest.raises(ValueError):
        segment.label_votes(model, cams, bg, planes, 17)


def test_command_line_writes_a_segmented_iteration(tmp_path, capsys):
    import json
    import os
    import shutil
    from binocular3dgs_amd import frames, segment
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
    # label planes for two of the three training cameras: left half 0, right half 2, a band of "no label" between; one as a
    # gray PNG (through frames.read_png), one as .npy; the third camera has no file and does not vote
    cams = list(scene.getTrainCameras())
    assert len(cams) == 3
    labels_dir = tmp_path / "labels"
    os.makedirs(labels_dir)
    W, H = int(cams[0].image_width), int(cams[0].image_height)
    plane = np.full((H, W), 255, np.uint8)
    plane[:, :W // 2 - 2], plane[:, W // 2 + 2:] = 0, 2
    np.save(labels_dir / (os.path.splitext(str(cams[0].image_name))[0] + ".npy"), plane)
    from test_segment_ref_cpu import _png
    (labels_dir / (os.path.splitext(str(cams[1].image_name))[0] + ".png")).write_bytes(_png(W, H, 0, plane))
    npz, pics = str(tmp_path / "stats.npz"), tmp_path / "pics"
    assert segment.main(["-m", str(out), "--labels", str(labels_dir), "--keep", "2", "--render", "test", "--out", str(pics),
                         "--stats", npz]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["n_labels"] == 3 and res["voting_views"] == 2 and res["P_before"] == P and res["kept"] == [2]
    assert len(res["gaussians_per_label"]) == 3 and res["gaussians_per_label"][1] == 0
    assert sum(res["gaussians_per_label"]) + res["unassigned"] == P and res["P_after"] == res["gaussians_per_label"][2] > 0
    assert res["iou"][1] is None and all(0.0 < res["iou"][l] <= 1.0 for l in (0, 2))
    seg_dir = out / "point_cloud" / "iteration_7_segmented"
    gl = np.load(seg_dir / "labels.npy")
    assert gl.dtype == np.uint8 and gl.shape == (P,) and int((gl == 2).sum()) == res["P_after"]
    part = load_ply(str(seg_dir / "point_cloud.ply"), 1)
    assert torch.equal(part._xyz.detach().cpu(), model._xyz.detach().cpu()[torch.from_numpy(gl == 2)])
    st = np.load(npz)
    assert st["votes_q32"].shape == (P, 3) and np.array_equal(st["labels"], gl)
    assert np.array_equal(segment.assign_labels(torch.from_numpy(st["votes_q32"])).numpy(), gl)
    n_test = len(list(scene.getTestCameras()))
    assert res["rendered"] == n_test > 0 and sorted(os.listdir(pics)) == ["label_%05d.png" % i for i in range(n_test)]
    pic = frames.read_png(str(pics / "label_00000.png"))
    colours = {tuple(c) for c in pic.reshape(-1, 3).tolist()}
    assert colours <= {segment.PALETTE[0], segment.PALETTE[2], (0, 0, 0)} and len(colours) >= 2
    with pytest.raises(SystemExit):
        segment.main(["-m", str(out), "--labels", str(labels_dir)])                      # neither --keep nor --remove
    with pytest.raises(SystemExit):
        segment.main(["-m", str(out), "--labels", str(labels_dir), "--dtu_masks", "--keep", "1"])
