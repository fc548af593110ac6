"""GPU: csrc/edit.hip and b3gs_nearest_query_index against tests/edit_ref.py, bit for bit; edit.register against the yardstick's
loop; the render of a transformed model from the transformed cameras against the render of the original; crop / merge round
trips."""
import math
import os

import numpy as np
import pytest
import torch

import edit_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else (a.view(np.uint64) if a.dtype == np.float64 else a)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _params(P, deg, seed):
    g = np.random.default_rng(seed)
    K = (deg + 1) ** 2 - 1
    p = [g.standard_normal(s).astype(np.float32) for s in ((P, 3), (P, 4), (P, 3), (P, K, 3))]
    if P > 2:
        for a in p:
            a[1] = 0.0                                        # a row of zeros
        p[0][2] = [-0.0, 0.0, -0.0]
    return p


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 257, 2000])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_transform_equals_the_yardstick(P, deg):
    from binocular3dgs_amd import _C, edit
    T = edit.Similarity(*edit_ref.random_similarity(11 * deg + P))
    words = T.device_words()
    host = _params(P, deg, P + deg)
    want = edit_ref.transform(*host, words, deg)
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    out = [torch.empty_like(t) for t in dev]
    _C.transform_gaussians(deg, *dev, words, *out)            # out of place
    for o, w, a in zip(out, want, dev):
        assert _same_bits(o, w)
    for t, a in zip(dev, host):
        assert _same_bits(t, a)                               # the inputs are untouched
    _C.transform_gaussians(deg, *dev, words, *dev)            # in place
    for t, w in zip(dev, want):
        assert _same_bits(t, w)
    pts = torch.from_numpy(host[0]).to(DEV)
    assert _same_bits(edit.transform_points(pts, T), want[0]) and _same_bits(want[0], edit_ref.transform_points(host[0], words))
    q = torch.from_numpy(host[0]).to(DEV)
    _C.transform_points(q, words, q)
    assert _same_bits(q, want[0])
    if P > 2:
        assert not np.any(want[3][1]) and not np.any(want[1][1])        # the row of zeros stays zero (t moves only xyz)


@pytest.mark.parametrize("deg", [0, 3])
def test_identity_similarity_keeps_the_bits(deg):
    """Identity: every finite value keeps its bits, except that -0.0 may come back as +0.0 (the header's rule); the yardstick
    says which."""
    from binocular3dgs_amd import _C, edit
    words = edit.Similarity().device_words()
    host = _params(300, deg, 5)
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    _C.transform_gaussians(deg, *dev, words, *dev)
    want = edit_ref.transform(*host, words, deg)
    for t, w, a in zip(dev, want, host):
        assert _same_bits(t, w)
        got = t.cpu().numpy()
        assert np.array_equal(got, a)                         # equal as numbers: -0.0 == +0.0
        nz = a != 0.0
        assert np.array_equal(got.view(np.uint32)[nz], a.view(np.uint32)[nz])


def test_transform_refuses_what_it_cannot_do():
    from binocular3dgs_amd import _C, _lib, edit
    words = edit.Similarity().device_words()
    z = lambda *s: torch.zeros(*s, device=DEV)               # noqa: E731
    with pytest.raises(ValueError):
        _C.transform_gaussians(4, z(2, 3), z(2, 4), z(2, 3), z(2, 15, 3), words, z(2, 3), z(2, 4), z(2, 3), z(2, 15, 3))
    with pytest.raises(ValueError):
        _C.transform_gaussians(3, z(2, 3), z(2, 4), z(2, 3), z(2, 8, 3), words, z(2, 3), z(2, 4), z(2, 3), z(2, 8, 3))
    with pytest.raises(_lib.B3gsError):
        _C.transform_points(torch.zeros(2, 3), words, torch.zeros(2, 3))
    bad = list(words)
    bad[12] = -1.0
    with pytest.raises(_lib.B3gsError, match="s > 0"):
        _C.transform_points(z(2, 3), bad, z(2, 3))


# ---- selection -----------------------------------------------------------------------------------------------------------------
def _select_case(V):
    """3000 Gaussians around the cameras of a ring, hand-placed points first; 32 x 24 masks"""
    from binocular3dgs_amd import edit
    from binocular3dgs_amd.camera import Camera, look_at_orbit
    g = np.random.default_rng(40 + V)
    W, H, P = 32, 24, 3000
    cams = [Camera(*look_at_orbit(360.0 * k / V + 3.0, pivot=(0.0, 0.0, 4.0)), 1.0, 0.8, W, H) for k in range(V)]
    cw = edit.camera_words(cams)
    xyz = (g.standard_normal((P, 3)) * 2.5 + np.array([0.0, 0.0, 4.0])).astype(np.float32)
    M = np.c_[np.eye(3), -np.array([0.5, 0.25, 4.0])]          # the box: centre (0.5, 0.25, 4), half (1, 2, 1.5): exact in float32
    half = np.array([1.0, 2.0, 1.5])
    k = 0
    for ax in range(3):                                        # on every face, and one float32 step outside it
        for sgn in (-1.0, 1.0):
            c = np.array([0.5, 0.25, 4.0], np.float32)
            c[ax] += np.float32(sgn * half[ax])
            xyz[k] = c
            c2 = c.copy()
            c2[ax] = np.nextafter(c[ax], np.float32(sgn * np.inf))
            xyz[k + 1] = c2
            k += 2
    centre, r = np.array([0.0, 0.0, 4.0]), 2.5                 # on the sphere's surface (1.5^2 + 2^2 = 2.5^2, exact), and one step outside
    xyz[k], xyz[k + 1] = [1.5, 2.0, 4.0], [np.nextafter(np.float32(1.5), np.float32(2)), 2.0, 4.0]
    k += 2
    xyz[k] = [np.nan, 0.0, 4.0]
    xyz[k + 1] = [0.0, np.inf, 4.0]
    xyz[k + 2] = [0.0, 0.0, -np.inf]
    k += 3
    # view 0 by hand, in words that are exact: the identity pose, fx = fy = 16, cx = 16, cy = 12, near = 0.25
    cw[0] = np.concatenate([np.c_[np.eye(3), np.zeros(3)].reshape(-1), [16.0, 16.0, 16.0, 12.0, W, H, 0.25]])
    xyz[k] = [0.3, 0.1, 0.25]                                  # z == near: out
    xyz[k + 1] = [-1.0, 0.0, 1.0]                              # u = 16 * -1 + 16 = 0: in
    xyz[k + 2] = [1.0, 0.0, 1.0]                               # u = 32 = W: out
    xyz[k + 3] = [0.0, -0.75, 1.0]                             # v = 0: in
    xyz[k + 4] = [0.0, 0.75, 1.0]                              # v = 24 = H: out
    xyz[k + 5] = [0.25, 0.25, 1.0]                             # texel (20, 16): zeroed in the mask below
    xyz[k + 6] = [0.3125, 0.25, 1.0]                           # texel (21, 16): set
    masks = (g.uniform(size=(V, H, W)) < 0.7).astype(np.uint8)
    ai = 0
    masks[ai] = 1
    masks[ai, 16, 20] = 0
    opacity = g.standard_normal((P, 1)).astype(np.float32)
    scaling = (g.standard_normal((P, 3)) * 0.5 - 3.0).astype(np.float32)
    logit = np.float32(math.log(0.3 / 0.7))
    opacity[0], opacity[1], opacity[2], opacity[3] = logit, np.nextafter(logit, np.float32(-10)), 5.0, 5.0
    lms = np.float32(math.log(0.08))
    scaling[0], scaling[1] = -9.0, -9.0
    scaling[2], scaling[3] = [lms, -9, -9], [-9, np.nextafter(lms, np.float32(0)), -9]
    return dict(xyz=xyz, opacity=opacity, scaling=scaling, box=(M, half), sphere=(centre, r * r), logit=float(logit), lms=float(lms),
                cams=cams, cw=cw, masks=masks, hand=k, axis=ai)


@pytest.mark.parametrize("V", [1, 8, 64])
def test_select_equals_the_yardstick_on_every_subset(V):
    from binocular3dgs_amd import _C
    c = _select_case(V)
    assert c["cw"].shape == (V, 19)
    xyz, op, sc = (torch.from_numpy(c[k]).to(DEV) for k in ("xyz", "opacity", "scaling"))
    cw, mk = torch.from_numpy(c["cw"]).to(DEV), torch.from_numpy(c["masks"]).to(DEV)
    box_words = [float(v) for v in c["box"][0].reshape(-1)] + [float(v) for v in c["box"][1]]
    sph_words = [float(v) for v in c["sphere"][0]] + [float(c["sphere"][1])]
    kept_any = False
    for subset in range(64):                                   # box, sphere, opacity, scale, views, masks
        on = [bool(subset >> b & 1) for b in range(6)]
        if on[5] and not on[4]:
            continue
        min_views = 1 + subset % 2
        keep, seen = _C.select_gaussians(xyz, op, sc, box_words if on[0] else None, sph_words if on[1] else None,
                                         c["logit"] if on[2] else None, c["lms"] if on[3] else None, cw if on[4] else None,
                                         mk if on[5] else None, min_views)
        wk, ws = edit_ref.select(c["xyz"], c["opacity"], c["scaling"], c["box"] if on[0] else None, c["sphere"] if on[1] else None,
                                 c["logit"] if on[2] else None, c["lms"] if on[3] else None, c["cw"] if on[4] else None,
                                 c["masks"] if on[5] else None, min_views)
        assert np.array_equal(keep.cpu().numpy().astype(bool), wk), on
        assert np.array_equal(seen.cpu().numpy(), ws), on
        kept_any |= bool(wk.any()) and not bool(wk.all())
    assert kept_any
    # the hand-placed points decide as written, in the yardstick (and therefore on the device)
    wk, _ = edit_ref.select(c["xyz"], None, None, box=c["box"])
    assert wk[:12].tolist() == [True, False] * 6
    wk, _ = edit_ref.select(c["xyz"], None, None, sphere=c["sphere"])
    assert wk[12:14].tolist() == [True, False] and not wk[14:17].any()
    k, ai = c["hand"], c["axis"]
    one = c["cw"][ai:ai + 1]
    _, s1 = edit_ref.select(c["xyz"], None, None, cameras=one)
    assert s1[k:k + 7].tolist() == [0, 1, 0, 1, 0, 1, 1] and not s1[14:17].any()
    _, s2 = edit_ref.select(c["xyz"], None, None, cameras=one, masks=c["masks"][ai:ai + 1])
    assert s2[k + 5:k + 7].tolist() == [0, 1]
    wk, _ = edit_ref.select(c["xyz"], c["opacity"], c["scaling"], logit_min=c["logit"], log_max_scale=c["lms"])
    assert wk[:4].tolist() == [True, False, True, False]


# ---- nearest point and the sums ------------------------------------------------------------------------------------------------
def _nearest_case():
    g = np.random.default_rng(8)
    b = (g.uniform(-1.0, 1.0, (3000, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.float32)
    b[100:110] = b[5]                                          # exact duplicates: the smallest index (5) wins
    b[2000] = b[1500]
    a = (g.uniform(-1.2, 1.2, (5000, 3)) * np.array([1.0, 0.6, 0.3])).astype(np.float32)
    a[:200] = b[g.integers(0, 3000, 200)]                      # on a point: d2 = 0 (several of them on the duplicates)
    a[200:210] = b[5]
    a[210] = b[1500]
    a[300:400] += np.float32(3.0)                              # beyond max_dist
    return a, b


def test_nearest_query_index_equals_the_brute_force():
    from binocular3dgs_amd.mesh_tools import NearestGrid
    import meshtools_ref
    a, b = _nearest_case()
    flat = b.copy()
    flat[:, 2] = 0.25
    for cloud, md in ((b, 0.2), (b[:1], 0.5), (flat, 0.2)):
        grid = NearestGrid(torch.from_numpy(cloud).to(DEV), md)
        q = torch.from_numpy(a).to(DEV)
        dist, index = grid.query_index(q)
        wd, wi = edit_ref.nearest_index(a, cloud, md)
        assert _same_bits(dist, wd)
        assert np.array_equal(index.cpu().numpy(), wi)
        assert _same_bits(grid.query(q), meshtools_ref.nearest_distances(a, cloud, md))     # nearest_query: as before
        assert _same_bits(grid.query(q), dist)
        if cloud is b:
            assert (wi[300:400] == -1).all() and (wi[200:210] == 5).all() and wi[210] == 1500 and (wi >= 0).sum() > 3000
    e, _ = NearestGrid(torch.from_numpy(b).to(DEV), 0.2).query_index(torch.zeros((0, 3), device=DEV))
    assert e.shape == (0,)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
def test_similarity_sums_equal_the_yardstick_fold(N):
    from binocular3dgs_amd import _C
    g = np.random.default_rng(N)
    a, b = g.standard_normal((N, 3)).astype(np.float32), g.standard_normal((700, 3)).astype(np.float32)
    index = g.integers(-1, 700, N).astype(np.int32)
    dist = g.uniform(0.0, 1.0, N).astype(np.float32)
    mask = g.uniform(size=N) < 0.8
    oa, ob = [0.1, -0.2, 0.3], [0.05, 0.0, -1.0]
    ta, tb, ti, td, tm = (torch.from_numpy(x).to(DEV) for x in (a, b, index, dist, mask))
    for gate, m, tmask in ((0.7, mask, tm), (2.0, None, None)):
        out = torch.zeros(2, 18, dtype=torch.float64, device=DEV)
        _C.similarity_sums(ta, tb, ti, td, gate, tmask, oa, ob, out[0])
        _C.similarity_sums(ta, tb, ti, td, gate, tmask, oa, ob, out[1])
        want = edit_ref.similarity_sums(a, b, index, dist, gate, m, oa, ob)
        assert _same_bits(out[0], want)
        assert _same_bits(out[1], out[0])                      # two calls: identical bits
        assert int(want[0]) == int(((index >= 0) & (dist <= np.float32(gate)) & (True if m is None else m)).sum())


def test_register_equals_the_yardstick_loop():
    from binocular3dgs_amd import edit
    src = edit_ref.surface_points(4000, seed=9)
    R = edit._rotation_about([0.2, 1.0, -0.4], 5.0)
    t, s = np.array([0.03, -0.02, 0.025]), 1.02
    dst = (s * (src.astype(np.float64) @ R.T) + t).astype(np.float32)
    for with_scale, iters in ((True, 30), (False, 8)):         # (a rigid fit of a scaled copy never settles: 8 iterations of it)
        T, hist = edit.register(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), max_dist=0.3, with_scale=with_scale,
                                iterations=iters)
        (Ry, ty, sy), hy = edit_ref.register(src, dst, 0.3, iterations=iters, with_scale=with_scale)
        assert _same_bits(np.concatenate([T.R.reshape(-1), T.t, [T.s]]), np.concatenate([Ry.reshape(-1), ty, [sy]]))     # 13 numbers
        assert hist == hy
    assert np.abs(T.R @ T.R.T - np.eye(3)).max() < 1e-12
    Ts, _ = edit.register(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV), max_dist=0.3, with_scale=True)
    assert np.abs(Ts.R - R).max() < 1e-5 and abs(Ts.s - s) < 1e-5 and np.abs(Ts.t - t).max() < 1e-5
    with pytest.raises(ValueError, match="fewer than 3"):
        edit.register(torch.from_numpy(src).to(DEV), torch.from_numpy(dst + np.float32(50.0)).to(DEV), max_dist=0.3)


# ---- renders -------------------------------------------------------------------------------------------------------------------
def _render(model, cam):
    from binocular3dgs_amd.render import PipelineParams, render
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), torch.zeros(3, device=DEV))
    return tuple(pkg[k].detach().cpu().numpy().astype(np.float64) for k in ("render", "rendered_depth", "rendered_alpha"))


def _to_dev(model):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    return GaussianModel.from_tensors(model._xyz, model._features_dc, model._features_rest, model._scaling, model._rotation, model._opacity,
                                      sh_degree=model.max_sh_degree, device=DEV, requires_grad=False)


def test_render_is_invariant_under_a_similarity():
    """The device render of edit.transform's model from transform_cameras' cameras against the device render of the original:
    at most d_ref (the float64 oracle's own difference between the two, tests/test_edit_ref_cpu.py) + 2 * 2e-5 (the project's
    colour tolerance against the oracle, README.md / DESIGN.md section 2, once for each render) per pixel, in colour, alpha and
    depth'/s relative to the depth."""
    from binocular3dgs_amd import edit
    d_ref = edit_ref.d_of(None)
    case = edit_ref.render_case()
    model = _to_dev(case["model"])
    moved = edit.transform(model, case["T"])
    want = edit_ref.transform(*(getattr(case["model"], n).numpy() for n in ("_xyz", "_rotation", "_scaling", "_features_rest")), case["words"], 3)
    for got, w in zip((moved._xyz, moved._rotation, moved._scaling, moved._features_rest), want):
        assert _same_bits(got, w)
    worst = 0.0
    for c0, c1 in zip(case["cameras"], edit.transform_cameras(case["cameras"], case["T"])):
        a, b = _render(model, c0.to(DEV)), _render(moved, c1.to(DEV))
        worst = max(worst, edit_ref.render_difference(a, b, case["T"].s))
    print(f"render invariance: device {worst:.3e}  d_ref {d_ref:.3e}  bound {d_ref + 4e-5:.3e}")
    assert worst <= d_ref + 2 * 2e-5


def test_crop_prune_save_load_round_trip(tmp_path):
    from binocular3dgs_amd import edit, importance
    from binocular3dgs_amd.gaussian_model import GaussianModel
    model = _to_dev(edit_ref.render_case()["model"])
    tests = dict(box=([-1.0, -1.0, 2.0], [1.5, 1.0, 7.0]), min_opacity=0.3)
    keep, seen = edit.select(model, **tests)
    wk, _ = edit_ref.select(model._xyz.cpu().numpy(), model._opacity.cpu().numpy(), None,
                            box=(np.c_[np.eye(3), -np.array([0.25, 0.0, 4.5])], np.array([1.25, 1.0, 2.5])), logit_min=math.log(0.3 / 0.7))
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), wk) and 0 < wk.sum() < len(wk) and not seen.any()
    cropped = edit.crop(model, **tests)
    pruned = importance.prune(model, keep)
    path = os.path.join(tmp_path, "point_cloud.ply")
    cropped.save_ply(path)
    back = GaussianModel(3)
    back.load_ply(path)
    for n in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(cropped, n), getattr(pruned, n)) and getattr(cropped, n).shape[0] == int(wk.sum())
        assert torch.equal(getattr(back, n).to(DEV).reshape(getattr(cropped, n).shape), getattr(cropped, n)), n


def test_merge_renders_as_the_oracle_renders_the_concatenation():
    from binocular3dgs_amd import edit, synth
    from binocular3dgs_amd.gaussian_model import GaussianModel
    a = synth.synth_model(700, seed=21, width=64, height=48, K=4, requires_grad=False, scale_mult=3.0)
    b = synth.synth_model(2000, seed=22, width=64, height=48, K=16, requires_grad=False, scale_mult=3.0)
    merged = edit.merge([_to_dev(a), _to_dev(b)])
    rest = torch.cat([torch.cat([a._features_rest, torch.zeros(700, 12, 3)], dim=1), b._features_rest])
    cat = GaussianModel.from_tensors(*(torch.cat([getattr(a, n), getattr(b, n)]) for n in ("_xyz", "_features_dc")), rest,
                                     *(torch.cat([getattr(a, n), getattr(b, n)]) for n in ("_scaling", "_rotation", "_opacity")),
                                     sh_degree=3, requires_grad=False)
    assert torch.equal(merged._features_rest.cpu(), rest) and merged._xyz.shape[0] == 2700 and merged.max_sh_degree == 3
    cam = synth.synth_cameras(64, 48, yaws=(4.0,))[0]
    want = edit_ref.oracle_render(cat, cam)
    got = _render(merged, cam.to(DEV))
    err = float(np.abs(got[0] - want[0]).max())
    print(f"merge: max|dC| against the oracle {err:.3e}")
    assert err <= 2e-5


# ---- the command lines -----------------------------------------------------------------------------------------------------------
def test_edit_command_line_composes_crops_merges_and_moves_the_dataset(tmp_path):
    """edit.main on a synthetic model folder: the options compose in the documented order, transform.json holds the matrix, the
    PLY holds crop(transform(model)) followed by the merged model (a lower SH degree, padded), --dataset_out writes the moved
    folder."""
    import json
    from binocular3dgs_amd import edit, synth, undistort as U
    from binocular3dgs_amd.gaussian_model import GaussianModel
    root = str(tmp_path / "model")
    os.makedirs(os.path.join(root, "point_cloud", "iteration_7"))
    src = str(tmp_path / "data")
    os.makedirs(os.path.join(src, "sparse/0"))
    q0, t0 = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1, 0.2, 0.3])
    U.write_cameras_bin(os.path.join(src, "sparse/0/cameras.bin"), {1: ("PINHOLE", 32, 24, (20.0, 20.0, 16.0, 12.0))})
    U.write_images_bin(os.path.join(src, "sparse/0/images.bin"), {1: (q0, t0, 1, "a.png")})
    with open(os.path.join(root, "cfg_args"), "w") as fp:
        fp.write(f"Namespace(sh_degree=3, source_path={src!r})")
    model = _to_dev(edit_ref.render_case()["model"])
    model.save_ply(os.path.join(root, "point_cloud", "iteration_7", "point_cloud.ply"))
    other = synth.synth_model(50, seed=4, K=4, device=DEV, requires_grad=False)             # degree 1
    other_path = str(tmp_path / "other.ply")
    other.save_ply(other_path)
    M0 = edit.Similarity(edit._rotation_about([0.0, 1.0, 0.0], 10.0), [0.5, 0.0, -1.0], 1.25).matrix()
    np.savetxt(str(tmp_path / "m.txt"), M0)
    out_data = str(tmp_path / "moved")
    assert edit.main(["-m", root, "--matrix", str(tmp_path / "m.txt"), "--rotate", "0", "0", "1", "30", "--translate", "0.5", "-0.25", "1",
                      "--scale", "2", "--box", "-4", "-4", "0", "4", "4", "14", "--min_opacity", "0.2", "--merge", other_path,
                      "--dataset_out", out_data]) == 0
    T = edit.Similarity(s=2.0).compose(edit.Similarity(t=[0.5, -0.25, 1.0])).compose(
        edit.Similarity(edit._rotation_about([0, 0, 1], 30.0))).compose(edit.Similarity.from_matrix(M0))
    out_dir = os.path.join(root, "point_cloud", "iteration_7_edited")
    tj = json.load(open(os.path.join(out_dir, "transform.json")))
    assert np.array_equal(np.array(tj["matrix"]), T.matrix()) and tj["s"] == T.s
    want = edit.merge([edit.crop(edit.transform(model, T), box=([-4, -4, 0], [4, 4, 14]), min_opacity=0.2), other])
    got = GaussianModel(3)
    got.load_ply(os.path.join(out_dir, "point_cloud.ply"))
    n = want._xyz.shape[0]
    assert 50 < n - 50 < model._xyz.shape[0] and got._xyz.shape[0] == n
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(got, name).to(DEV).reshape(getattr(want, name).shape), getattr(want, name)), name
    assert torch.count_nonzero(got._features_rest[-50:, 3:]) == 0 and torch.count_nonzero(got._features_rest[-50:, :3]) > 0
    q1, t1 = U.read_images_bin_full(os.path.join(out_data, "sparse/0/images.bin"))[1][:2]
    qw, tw = edit.transform_pose(q0, t0, T)
    assert np.array_equal(q1, qw) and np.array_equal(t1, tw)


def _trained_folder(tmp_path, folder, dataset_name, white):
    """a model folder (iteration 7, cfg_args) made from a copy of a golden scene folder, as train leaves one"""
    import shutil
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    src = str(shutil.copytree(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", folder), tmp_path / folder))
    out = str(tmp_path / "model")
    np.random.seed(0)
    scene = Scene.from_dataset(src, GaussianModel(1), eval=True, n_views=3, dataset_name=dataset_name, resolution=1,
                               white_background=white, init_points="sparse", model_path=out, shuffle=False)
    scene.save(7)
    with open(os.path.join(out, "cfg_args"), "w") as fp:
        fp.write(f"Namespace(source_path={src!r}, images='images', eval=True, n_views=3, dataset_name={dataset_name!r}, resolution=1, "
                 f"white_background={white!r}, sh_degree=1, init_points='sparse')")
    base = GaussianModel(1)
    base.load_ply(os.path.join(out, "point_cloud", "iteration_7", "point_cloud.ply"))
    return src, out, base, list(scene.getTrainCameras())


def _same_model(path, want, deg=1):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    got = GaussianModel(deg)
    got.load_ply(path)
    assert got._xyz.shape[0] == want._xyz.shape[0]
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(got, name).to(DEV).reshape(getattr(want, name).shape), getattr(want, name)), name


def test_edit_orients_by_the_scene_cameras_and_crops_by_their_masks(tmp_path):
    """edit.run --orient cameras --unit_radius --masked_views 2 on a Blender scene folder (RGBA images: every training view
    has an alpha mask with zero texels): the similarity is orient_from_cameras of the scene's training cameras, and the PLY is
    the transformed model cropped by the MOVED cameras with their masks."""
    from binocular3dgs_amd import edit, importance
    src, out, base, cams = _trained_folder(tmp_path, "scene_blender", "Blender", True)
    masks = [c.gt_alpha_mask for c in cams]
    assert all(m is not None for m in masks) and any(bool((m == 0).any()) for m in masks)
    res = edit.run(out, orient="cameras", unit_radius=True, masked_views=2)
    T = edit.orient_from_cameras(cams, True)
    assert np.array_equal(np.array(res["matrix"]), T.matrix()) and res["s"] == T.s
    moved = edit.transform_cameras(cams, T)
    centres = np.stack([edit._camera_pose(c)[1] for c in moved])
    assert abs(np.linalg.norm(centres, axis=1).mean() - 1.0) <= 1e-12                # the mean camera distance is 1 in the new frame
    tm = edit.transform(base, T)
    keep, seen = edit.select(tm, cameras=moved, masks=masks, min_views=2)
    unmasked, _ = edit.select(tm, cameras=moved, min_views=2)
    P = base._xyz.shape[0]
    assert 0 < int(keep.sum()) < int(unmasked.sum()) <= P and not bool((keep & ~unmasked).any())   # the masks took some away
    assert res["P_before"] == P and res["P_after"] == int(keep.sum())
    _same_model(res["ply"], importance.prune(tm, keep))


def test_edit_registers_to_a_cloud_and_the_moved_folders_serve_spiral(tmp_path):
    """edit.run --rotate ... --register_to CLOUD --dataset_out DST --model_out NEW on an LLFF scene folder.  The cloud is the
    model's own centres under a known similarity G, so the composed result Tr o T0 is G up to the float32 rounding of the two
    clouds: <= 2^-24 * 5.5 = 3.3e-7 per coordinate, which a least-squares fit over 300 exact pairs of spread 0.6 turns into at
    most 3.3e-7 / 0.6 = 5.5e-7 per rotation entry and 5.5e-7 * 4 + 3.3e-7 = 2.5e-6 per translation entry (the centroid lies 4
    from the origin): the bound is 1e-5.  DST holds the poses and poses_bounds.npy under the same matrix, and spiral runs
    on (NEW, DST)."""
    from binocular3dgs_amd import dataset_readers as dr, edit, spiral, undistort as U
    src, out, base, cams = _trained_folder(tmp_path, "scene_llff", "LLFF", False)
    T0 = edit.Similarity(edit._rotation_about([0.0, 0.0, 1.0], 2.0))
    G = edit.Similarity(edit._rotation_about([0.2, 1.0, 0.3], 0.5), [0.02, -0.01, 0.015]).compose(T0)
    xyz = base._xyz.detach().cpu().numpy().astype(np.float64)
    assert xyz.shape == (300, 3) and np.abs(xyz).max() < 5.5
    cloud = str(tmp_path / "cloud.ply")
    dr.write_point_ply(cloud, G.apply(xyz), np.zeros((300, 3)))
    dst, new = str(tmp_path / "llff_moved"), str(tmp_path / "model_moved")
    res = edit.run(out, rotate=[0.0, 0.0, 1.0, 2.0], register_to=cloud, max_dist=0.5, dataset_out=dst, model_out=new)
    assert res["register"]["pairs"] == 300 and res["register"]["iterations"] <= 30
    M = np.array(res["matrix"])
    err = float(np.abs(M - G.matrix()).max())
    print(f"edit --register_to: |Tr o T0 - G| {err:.3e}, rms {res['register']['rms']:.3e} after {res['register']['iterations']} iterations")
    assert err <= 1e-5 and res["s"] == 1.0
    # the same similarity object, not a decomposition of M: the device stages are reproducible bit for bit
    from binocular3dgs_amd.init_points import read_ply_vertices
    rows = read_ply_vertices(cloud)
    gt = torch.from_numpy(np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)).to(DEV)
    Tr, hist = edit.register(edit.transform_points(base._xyz.detach(), T0), gt, max_dist=0.5)
    T = Tr.compose(T0)
    assert np.array_equal(T.matrix(), M) and len(hist) == res["register"]["iterations"]
    _same_model(res["ply"], edit.transform(base, T))
    _same_model(os.path.join(new, "point_cloud", "iteration_7", "point_cloud.ply"), edit.transform(base, T))
    assert spiral.read_cfg_args(new) == spiral.read_cfg_args(out) and spiral.max_iteration(new) == 7
    before = U.read_images_bin_full(os.path.join(src, "sparse/0/images.bin"))
    after = U.read_images_bin_full(os.path.join(dst, "sparse/0/images.bin"))
    assert set(after) == set(before) and len(after) == 10
    for iid, rec in before.items():
        q, t = edit.transform_pose(rec[0], rec[1], T)
        assert np.array_equal(after[iid][0], q) and np.array_equal(after[iid][1], t) and after[iid][3] == rec[3]
    assert np.array_equal(np.load(os.path.join(dst, "poses_bounds.npy")),
                          edit.transform_poses_bounds(np.load(os.path.join(src, "poses_bounds.npy")), T))
    frames_dir = spiral.run(new, dst, n_frames=2)
    assert sorted(f for f in os.listdir(frames_dir) if f[0].isdigit()) == ["00000.png", "00001.png"]


def test_eval_mesh_align_registers_before_it_scores(tmp_path):
    from binocular3dgs_amd import edit, eval_mesh, mesh
    from binocular3dgs_amd import dataset_readers as dr
    nx, ny = 60, 42
    gx, gy = np.meshgrid(np.linspace(-1.0, 1.0, nx), np.linspace(-0.7, 0.7, ny), indexing="xy")
    x, y = gx.reshape(-1), gy.reshape(-1)
    z = 0.3 * np.sin(2.1 * x + 0.4) * np.cos(1.3 * y) + 0.15 * x * y + 0.1 * np.exp(-8.0 * ((x - 0.3) ** 2 + (y + 0.2) ** 2)) + 0.2 * x
    v = np.stack([x, y, z], axis=1)
    i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1)
    f = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)]).astype(np.int32)
    move = edit.Similarity(edit._rotation_about([0.3, 1.0, 0.2], 3.0), [0.02, -0.015, 0.02], 1.0)
    mesh_path, gt_path = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply")
    mesh.write_mesh_ply(mesh_path, move.inverse().apply(v).astype(np.float32), np.full((len(v), 3), 128, np.uint8), f)
    dr.write_point_ply(gt_path, v, np.zeros((len(v), 3)))
    ideal_path = str(tmp_path / "ideal" / "mesh.ply")
    os.makedirs(os.path.dirname(ideal_path))
    mesh.write_mesh_ply(ideal_path, v.astype(np.float32), np.full((len(v), 3), 128, np.uint8), f)
    ideal = eval_mesh.run(ideal_path, gt_path, 0.02, 0.2, 0.01)          # the mesh where it belongs: the floor its sampling leaves
    plain = eval_mesh.run(mesh_path, gt_path, 0.02, 0.2, 0.01)
    assert "align" not in plain and "before_align" not in plain
    res = eval_mesh.run(mesh_path, gt_path, 0.02, 0.2, 0.01, align=True)
    before, M = res["before_align"], np.array(res["align"]["matrix"])
    assert before["chamfer"] == plain["chamfer"] and before["n_recon"] == res["n_recon"]      # the same sampling density before and after
    assert res["spacing"] == 0.02 and res["align"]["s"] == 1.0
    # Where the registration leaves a vertex against where it belongs: the nearest-point distance is 1-Lipschitz in a point's
    # position, so no mean distance can exceed the ideal one by more than the largest such displacement.
    placed = edit.Similarity.from_matrix(M).apply(move.inverse().apply(v).astype(np.float32))
    delta = float(np.linalg.norm(placed - v, axis=1).max())
    start = float(np.linalg.norm(move.inverse().apply(v) - v, axis=1).max())
    print(f"eval_mesh --align: chamfer ideal {ideal['chamfer']:.4e} before {before['chamfer']:.4e} after {res['chamfer']:.4e}; "
          f"largest vertex displacement {start:.4e} -> {delta:.4e}")
    assert delta < start                                                   # nearer than it started
    assert res["accuracy"] <= ideal["accuracy"] + delta and res["completeness"] <= ideal["completeness"] + delta
    assert res["chamfer"] < before["chamfer"]
