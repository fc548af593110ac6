"""The mesh rasterizer on the device (csrc/meshraster.hip, binocular3dgs_amd/mesh_render.py) against the numpy restatement of
tests/meshraster_ref.py.  Coverage is integer work, depth and colour are single correctly rounded operations, the buffer is a
minimum: triangle ids, depth, alpha, both colour outputs, the per-face pixel counts and the rejected counts are compared bit
for bit.  Images are 16x12 .. 70x50 except where a path threshold needs a wider one (stated there)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402
import simplify_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12
CAM = rr.camera_row()[None]
BG = (0.25, 0.5, 0.75)
INT_MAX = 2 ** 31 - 1
PATHS = {"default": (-1, -1), "lane": (INT_MAX, INT_MAX), "wave": (0, INT_MAX), "group": (0, 0)}


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _device(v, c, f):
    return torch.from_numpy(np.ascontiguousarray(v, F)).to(DEV), torch.from_numpy(np.ascontiguousarray(c, np.uint8)).to(DEV), \
        torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(DEV)


def _check(v, c, f, cams, w, h, paths=("default",), cull=False, ref=None):
    """both shadings, the counts and face_pixels of one launch pair per path against the yardstick -> the yardstick's output"""
    from binocular3dgs_amd import mesh_render
    ref = rr.render(v, c, f, cams, w, h, BG, "both", cull) if ref is None else ref
    dv, dc, df = _device(v, c, f)
    bg = torch.tensor(BG, device=DEV)
    n = len(cams)
    for path in paths:
        small, wave = PATHS[path]
        fp = torch.zeros(len(f), dtype=torch.int32, device=DEV)
        tid, depth, alpha, colour, counts = mesh_render.raster_views(dv, dc, df, cams, w, h, bg, cull_backface=cull, face_pixels=fp,
                                                                     small_box=small, wave_box=wave)
        normal = mesh_render.raster_views(dv, None, df, cams, w, h, bg, shading="normal", cull_backface=cull, small_box=small, wave_box=wave)[3]
        assert np.array_equal(tid.cpu().numpy(), ref["triangle_id"]), path
        for name, got in (("depth", depth), ("alpha", alpha), ("colour", colour), ("normal", normal)):
            assert np.array_equal(_bits(got), _bits(ref[name])), f"{path}: {name}: {(_bits(got) != _bits(ref[name])).sum()} words differ"
        assert np.array_equal(fp.cpu().numpy(), ref["face_pixels"]), path
        assert counts.tolist() == ref["rejected"].tolist() + [0] * (8 - n) + [ref["bad"]], path
    return ref


def _tri(pix, z=1.0, w=W, h=H):
    v = rr.at_pixels(pix, z, w, h)
    return v, rr.grey(len(v), 1), np.arange(len(v), dtype=np.int32).reshape(-1, 3)


SINGLES = {
    "edges_through_centres": ([(2, 2), (10, 2), (2, 10)], 36),
    "other_winding": ([(2, 2), (2, 10), (10, 2)], 36),
    "sub_pixel_no_centre": ([(4.25, 4.25), (4.75, 4.25), (4.25, 4.75)], 0),
    "sub_pixel_one_centre": ([(4.75, 4.75), (5.5, 4.75), (4.75, 5.5)], 1),
    "zero_area": ([(2, 2), (6, 6), (10, 10)], 0),
    "outside": ([(-9, -7), (-2, -7), (-9, -1)], 0),
    "past_all_borders": ([(-40, -30), (90, -20), (5, 80)], W * H),
}


@pytest.mark.parametrize("name", list(SINGLES))
def test_a_single_triangle(name):
    pix, pixels = SINGLES[name]
    ref = _check(*_tri(pix, 2.5), CAM, W, H, paths=PATHS)
    assert ref["face_pixels"].tolist() == [pixels]


def test_cull_backface_drops_the_clockwise_winding():
    front, back = _tri([(2, 2), (2, 10), (10, 2)]), _tri([(2, 2), (10, 2), (2, 10)])
    assert _check(*front, CAM, W, H, cull=True)["face_pixels"].tolist() == [36]
    assert _check(*back, CAM, W, H, paths=PATHS, cull=True)["face_pixels"].tolist() == [0]


def test_a_fan_around_a_vertex_on_a_pixel_centre_gives_every_pixel_one_owner():
    rim = [(8 + 6.5 * math.cos(a), 6 + 5.25 * math.sin(a)) for a in np.arange(8) * math.pi / 4]
    rim = np.round(np.array(rim) * 4) / 4
    pix = [p for k in range(8) for p in ((8, 6), tuple(rim[k]), tuple(rim[(k + 1) % 8]))]
    v, c, f = _tri(pix)
    alone = sum(rr.render(v, c, f[k:k + 1], CAM, W, H)["alpha"][0, 0] for k in range(8))
    assert alone.max() == 1.0 and alone[6, 8] == 1.0
    ref = _check(v, c, f, CAM, W, H, paths=PATHS)
    assert ref["face_pixels"].sum() == alone.sum() and (ref["face_pixels"] > 0).all()


def test_interpenetrating_and_tied_triangles():
    a = rr.at_pixels([(1, 1), (14, 2), (3, 11)], [1.0, 4.0, 2.0], W, H)
    b = rr.at_pixels([(1, 2), (14, 1), (12, 11)], [4.0, 1.0, 2.0], W, H)
    ref = _check(np.concatenate([a, b]), rr.grey(6, 2), np.array([[0, 1, 2], [3, 4, 5]], np.int32), CAM, W, H, paths=PATHS)
    assert (ref["face_pixels"] > 5).all()                                      # each is in front somewhere
    # two identical triangles, ids swapped: the smaller index wins every pixel; coplanar overlapping triangles likewise
    v = rr.at_pixels([(2, 2), (2, 10), (13, 3), (6, 1), (1, 9), (14, 10)], 2.0, W, H)
    for faces in ([[0, 1, 2], [0, 1, 2]], [[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]):
        ref = _check(v, rr.grey(6, 3), np.array(faces, np.int32), CAM, W, H, paths=PATHS)
        one, two = (rr.render(v, rr.grey(6), np.array(fc, np.int32).reshape(1, 3), CAM, W, H) for fc in faces)
        overlap = (one["alpha"] == 1) & (two["alpha"] == 1)
        tied = overlap & (_bits(one["depth"]) == _bits(two["depth"]))       # (coplanar: equal up to the rounding of the weights)
        assert overlap.sum() > 10 and tied.sum() > 10 and (ref["triangle_id"][tied[:, 0]] == 0).all()
        nearer = overlap & (two["depth"] < one["depth"])
        assert (ref["triangle_id"][nearer[:, 0]] == 1).all()


def test_boxes_on_both_sides_of_the_path_thresholds():
    """clamped boxes of SMALL_BOX - 1, SMALL_BOX, SMALL_BOX + 1 pixels and of WAVE_BOX - 1, WAVE_BOX, WAVE_BOX + 1: the last
    needs 241 x 17, so this image is 250 x 70"""
    from binocular3dgs_amd import mesh_render
    assert (mesh_render.SMALL_BOX, mesh_render.WAVE_BOX) == (32, 4096)
    w, h = 250, 70
    pix, want = [], []
    for k, (bw, bh) in enumerate([(31, 1), (8, 4), (11, 3), (65, 63), (64, 64), (241, 17)]):
        x0, y0 = 3 + k, 2 + (k % 3)
        pix += [(x0, y0), (x0 + bw - 1, y0), (x0, y0 + bh - 1 + (0.5 if bh == 1 else 0))]
        want.append(bw * bh)
    v, c, f = _tri(pix, [1.0 + 0.25 * (k // 3) for k in range(18)], w, h)
    X, Y, _, _, _, _ = rr.project(v, CAM[0], w, h)
    boxes = [rr.box_pixels(rr.setup([int(q) for q in X[t]], [int(q) for q in Y[t]], w, h)) for t in f]
    assert boxes == [31, 32, 33, 4095, 4096, 4097] == want
    _check(v, c, f, CAM, w, h, paths=PATHS)


def test_one_triangle_over_the_whole_image_and_every_path_gives_the_same_bits():
    w, h = 70, 50
    big = rr.at_pixels([(-200, -150), (400, -100), (20, 500)], [1.0, 2.0, 4.0], w, h)
    v, c, f = rr.random_mesh(120, w, h, 11, span=9.0)
    v, c, f = np.concatenate([big, v]), np.concatenate([rr.grey(3, 4), c]), np.concatenate([[[0, 1, 2]], f + 3]).astype(np.int32)
    ref = _check(v, c, f, CAM, w, h, paths=PATHS)
    assert (ref["alpha"] == 1.0).all() and ref["face_pixels"][0] > 500 and (ref["face_pixels"][1:] > 0).sum() > 10


@pytest.mark.parametrize("nf", [63, 64, 65, 255, 256, 257])
def test_triangle_counts_around_a_wave_and_a_workgroup(nf):
    v, c, f = rr.random_mesh(nf, 40, 30, nf)
    _check(v, c, f, CAM, 40, 30, paths=("default", "wave"))


def test_more_large_triangles_than_one_chunk_of_the_ordered_scan():
    """The scan of the block sums takes 1024 blocks of 256 triangles per step: the seam is at 262144 triangles.  262144 + 300
    copies of one image-filling triangle all go to the wave list; the LAST one is nearer, so it must win every pixel -- its list
    position lies behind the seam."""
    from binocular3dgs_amd import mesh_render
    n = 1024 * 256 + 300
    v = np.concatenate([rr.at_pixels([(-40, -30), (90, -20), (5, 80)], 2.0, W, H), rr.at_pixels([(-40, -30), (90, -20), (5, 80)], 1.0, W, H)])
    f = np.tile(np.array([[0, 1, 2]], np.int32), (n, 1))
    f[-1] = [3, 4, 5]
    ref = rr.render(v, rr.grey(6), f[[0, -1]], CAM, W, H)
    dv, dc, df = _device(v, rr.grey(6), f)
    fp = torch.zeros(n, dtype=torch.int32, device=DEV)
    tid, depth, _, colour, counts = mesh_render.raster_views(dv, dc, df, CAM, W, H, face_pixels=fp)
    assert (tid == n - 1).all() and np.array_equal(_bits(depth), _bits(ref["depth"])) and np.array_equal(_bits(colour), _bits(ref["colour"]))
    assert int(fp[-1]) == W * H and int(fp.sum()) == W * H and counts.tolist() == [0] * 9


def test_rejected_triangles_are_counted_and_the_others_are_unaffected():
    good = rr.at_pixels([(2, 2), (2, 10), (10, 2)], 1.0, W, H)
    v = np.concatenate([good, rr.at_pixels([(3, 3), (9, 3), (3, 9)], [2, 2, 0.125], W, H),          # a vertex behind the near plane
                        rr.at_pixels([(3, 3), (9, 3), (3.0e4, 9)], 2.0, W, H),                       # beyond the guard band
                        np.array([[0.1, 0.1, 2.0], [0.2, np.nan, 2.0], [0.1, 0.3, 2.0]], F)])        # not finite
    f = np.array([[3, 4, 5], [0, 1, 2], [6, 7, 8], [9, 10, 11], [0, 1, 12], [-1, 1, 2]], np.int32)
    ref = _check(v, rr.grey(12, 5), f, CAM, W, H, paths=PATHS)
    assert ref["rejected"].tolist() == [5] and ref["bad"] == 2 and ref["face_pixels"].tolist() == [0, 36, 0, 0, 0, 0]


# ---- views -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    """the 24^3 sphere of simplify_ref.sphere_mesh() from nine cameras at 64 x 48, both shadings: computed once"""
    v, c, f = sr.sphere_mesh()
    cams = rr.orbit_cameras(9, (12.0, 12.0, 12.0), 30.0, 60.0, 58.0, height=-4.0)
    return v, c, f, cams, rr.render(v, c, f, cams, 64, 48, BG, "both")


def _slice(ref, a, b):
    out = {k: (v[a:b] if isinstance(v, np.ndarray) and k != "face_pixels" else v) for k, v in ref.items()}
    return out


def test_the_sphere_from_three_cameras_both_shadings(sphere):
    v, c, f, cams, ref = sphere
    sub = _slice(ref, 0, 3)
    sub["face_pixels"] = np.stack([np.bincount(ref["triangle_id"][k][ref["triangle_id"][k] >= 0], minlength=len(f)) for k in range(3)]).sum(0)
    _check(v, c, f, cams[:3], 64, 48, ref=sub)
    _check(v, c, f, cams[:3], 64, 48, ref=sub)                        # a second call: the same bits
    assert (ref["alpha"][:3].sum(axis=(1, 2, 3)) > 300).all()


@pytest.mark.parametrize("n", [1, 8, 9])
def test_render_mesh_splits_the_cameras_into_launches(sphere, n):
    from binocular3dgs_amd import mesh_render
    v, c, f, cams, ref = sphere
    dv, dc, df = _device(v, c, f)
    fp = torch.zeros(len(f), dtype=torch.int32, device=DEV)
    outs, rejected = mesh_render.render_mesh(dv, dc, df, cams[:n], torch.tensor(BG, device=DEV), size=(64, 48), face_pixels=fp)
    assert len(outs) == n and rejected.tolist() == [0] * (n + 1)
    for k, o in enumerate(outs):
        assert tuple(o["render"].shape) == (3, 48, 64) and tuple(o["rendered_depth"].shape) == (1, 48, 64) == tuple(o["rendered_alpha"].shape)
        assert np.array_equal(o["triangle_id"].cpu().numpy(), ref["triangle_id"][k])
        assert np.array_equal(_bits(o["render"]), _bits(ref["colour"][k])) and np.array_equal(_bits(o["rendered_depth"]), _bits(ref["depth"][k]))
    want = np.bincount(ref["triangle_id"][:n][ref["triangle_id"][:n] >= 0], minlength=len(f))
    assert np.array_equal(fp.cpu().numpy(), want)
    if n == 9:                                                        # accumulated over two calls = one call
        two = torch.zeros_like(fp)
        mesh_render.render_mesh(dv, dc, df, cams[:4], size=(64, 48), face_pixels=two)
        mesh_render.render_mesh(dv, dc, df, cams[4:9], size=(64, 48), face_pixels=two)
        assert torch.equal(two, fp) and torch.equal(mesh_render.face_pixels(dv, df, cams[:9], size=(64, 48)), fp)


def _cameras(sizes, fx=60.0):
    from binocular3dgs_amd.camera import Camera, focal2fov
    cams = []
    for k, (w, h) in enumerate(sizes):
        row = rr.orbit_cameras(len(sizes), (12.0, 12.0, 12.0), 30.0, fx)[k].astype(np.float64)
        R = row[:9].reshape(3, 3)
        cams.append(Camera(R.T, row[9:12], focal2fov(fx, w), focal2fov(fx, h), w, h, uid=k, device=DEV))
    return cams


def test_two_image_sizes_in_one_call(sphere):
    from binocular3dgs_amd import mesh, mesh_render
    v, c, f = sphere[:3]
    cams = _cameras([(64, 48), (64, 48), (40, 30)])
    table = mesh.camera_table(cams)
    outs, _ = mesh_render.render_mesh(*_device(v, c, f), cams, shading="normal")
    for k, (w, h) in enumerate([(64, 48), (64, 48), (40, 30)]):
        ref = rr.render(v, c, f, table[k:k + 1], w, h, shading="normal")
        assert tuple(outs[k]["render"].shape) == (3, h, w)
        assert np.array_equal(outs[k]["triangle_id"].cpu().numpy(), ref["triangle_id"][0]) and np.array_equal(_bits(outs[k]["render"]), _bits(ref["colour"][0]))


def test_raster_and_resolve_replay_from_a_graph_onto_a_changed_vertex_buffer():
    from binocular3dgs_amd import mesh_render
    meshes = [rr.random_mesh(90, 40, 30, s, span=9.0) for s in (21, 22)]
    f = meshes[0][2]
    dv, dc, df = _device(*meshes[0])
    fp = torch.zeros(len(f), dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mesh_render.raster_views(dv, dc, df, CAM, 40, 30, face_pixels=fp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tid, depth, alpha, colour, counts = mesh_render.raster_views(dv, dc, df, CAM, 40, 30, face_pixels=fp)
    for v, c, _ in (meshes[1], meshes[0]):
        dv.copy_(torch.from_numpy(v)), dc.copy_(torch.from_numpy(c)), fp.zero_()
        graph.replay()
        ref = rr.render(v, c, f, CAM, 40, 30)
        assert np.array_equal(tid.cpu().numpy(), ref["triangle_id"]) and np.array_equal(_bits(depth), _bits(ref["depth"]))
        assert np.array_equal(_bits(colour), _bits(ref["colour"])) and np.array_equal(fp.cpu().numpy(), ref["face_pixels"])
        assert counts.tolist() == [0] * 9


# ---- the callers -------------------------------------------------------------------------------------------------------
def test_cull_unseen_removes_a_sphere_hidden_inside_another():
    from binocular3dgs_amd import mesh_render
    vo, fo = rr.uv_sphere((0.0, 0.0, 0.0), 2.0, 14, 9)
    vi, fi = rr.uv_sphere((0.1, 0.0, 0.0), 0.7, 8, 5)
    v, f = np.concatenate([vo, vi]), np.concatenate([fo, fi + len(vo)]).astype(np.int32)
    c = rr.grey(len(v), 6)
    cams = rr.orbit_cameras(5, (0.0, 0.0, 0.0), 7.0, 40.0, height=-2.0)
    ref = rr.render(v, c, f, cams, 48, 40)
    dv, dc, df = _device(v, c, f)
    for min_pixels in (1, 3):
        keep = ref["face_pixels"] >= min_pixels
        assert not keep[len(fo):].any() and 10 < keep.sum() < len(fo)
        assert (ref["face_pixels"] == 2).any()                            # 1 and 3 keep different sets
        gv, gc, gf = mesh_render.cull_unseen(dv, dc, df, cams, min_pixels, size=(48, 40))
        used = np.unique(f[keep])
        remap = np.full(len(v), -1, np.int64)
        remap[used] = np.arange(len(used))
        assert np.array_equal(gf.cpu().numpy(), remap[f[keep]]) and np.array_equal(_bits(gv), _bits(v[used]))
        assert np.array_equal(gc.cpu().numpy(), c[used])
    bad = df.clone()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError, match="outside 0"):
        mesh_render.cull_unseen(dv, dc, bad, cams, size=(48, 40))


def _shell_model(tmp_path, P=400):
    """the 400-Gaussian shell of tests/test_gpu_mesh.py, built the same way"""
    from binocular3dgs_amd.camera import look_at_orbit
    from binocular3dgs_amd.extract_mesh import cameras_from_json
    from binocular3dgs_amd.gaussian_model import GaussianModel, inverse_sigmoid
    g = torch.Generator().manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1)
    xyz = d + torch.tensor([0.0, 0.0, 6.0])
    model = GaussianModel.from_tensors(xyz, torch.rand(P, 1, 3, generator=g), torch.zeros(P, 3, 3), torch.full((P, 3), math.log(0.12)),
                                       torch.randn(P, 4, generator=g), inverse_sigmoid(torch.full((P, 1), 0.95)), sh_degree=1,
                                       device=DEV, requires_grad=False)
    path = str(tmp_path / "model")
    model.save_ply(os.path.join(path, "point_cloud", "iteration_7", "point_cloud.ply"))
    entries = []
    for k in range(6):
        R, T = look_at_orbit(60.0 * k)
        entries.append({"id": k, "img_name": f"v{k}", "width": 64, "height": 48, "position": (-R @ T).tolist(),
                        "rotation": [row.tolist() for row in R], "fx": 110.0, "fy": 110.0})
    with open(os.path.join(path, "cameras.json"), "w") as fp:
        json.dump(entries, fp)
    with open(os.path.join(path, "cfg_args"), "w") as fp:
        fp.write("Namespace(sh_degree=1, white_background=False, source_path='')")
    loaded = GaussianModel(1)
    loaded.load_ply(os.path.join(path, "point_cloud", "iteration_7", "point_cloud.ply"))
    return path, loaded, cameras_from_json(os.path.join(path, "cameras.json"))


def test_end_to_end_depth_agreement_and_the_command_lines(tmp_path, capsys):
    """fuse_model on the shell, then the mesh against the model's depth in the same cameras.  The sums are checked against numpy
    on the returned images (means within n 2^-52 relative); the median |z_mesh - d| lies below the truncation of 4 voxels, inside
    which the zero crossing sits by construction: a sanity bound, not a quality claim."""
    from binocular3dgs_amd import eval_mesh, extract_mesh, frames, mesh, mesh_render, spiral
    from binocular3dgs_amd.evaluate import _batches
    path, model, cams = _shell_model(tmp_path)
    bg = torch.zeros(3, device=DEV)
    v, c, f, vol = mesh.fuse_model(model, cams, bg, resolution=24, return_volume=True)
    stats = mesh_render.depth_agreement(model, v, f, cams, bg)
    outs, _ = mesh_render.render_mesh(v, None, f, cams, shading="normal")
    d, nmodel, nmesh = [], 0, 0
    for idx, mo in _batches(model, cams, bg, 8, full=True):
        for i, o in zip(idx, mo):
            al, dep = o["rendered_alpha"].cpu().numpy().reshape(48, 64), o["rendered_depth"].cpu().numpy().reshape(48, 64).astype(np.float64)
            z, cover = outs[i]["rendered_depth"].cpu().numpy().reshape(48, 64).astype(np.float64), outs[i]["rendered_alpha"].cpu().numpy().reshape(48, 64) > 0
            both = (al >= 0.5) & cover
            d.append(np.abs(z[both] - dep[both] / al[both].astype(np.float64)))
            nmodel, nmesh = nmodel + int((al >= 0.5).sum()), nmesh + int(cover.sum())
    d = np.concatenate(d)
    n = len(d)
    with capsys.disabled():
        print(f"depth agreement: median {stats['median'] / vol.voxel_size:.4f} voxels, mean {stats['mean'] / vol.voxel_size:.4f} voxels, "
              f"{n} pixels, model_missed {stats['model_missed']:.4f}, mesh_uncovered {stats['mesh_uncovered']:.4f}")
    assert n > 1000 and (stats["pixels"], stats["model_pixels"], stats["mesh_pixels"]) == (n, nmodel, nmesh)
    assert abs(stats["mean"] - d.sum() / n) <= n * 2.0 ** -52 * (d.sum() / n)
    assert stats["median"] == np.sort(d)[(n - 1) // 2]
    assert stats["model_missed"] == (nmodel - n) / nmodel and stats["mesh_uncovered"] == (nmesh - n) / nmesh
    assert stats["median"] < 4.0 * vol.voxel_size
    # extract_mesh: without the new options the file is what the python call gives (the parent's bytes), with --cull_unseen the
    # arrays of mesh_render.cull_unseen
    out = os.path.join(path, "mesh", "iteration_7", "mesh.ply")
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24"]) == 0
    mesh.write_mesh_ply(str(tmp_path / "plain.ply"), v, c, f)
    assert open(out, "rb").read() == open(tmp_path / "plain.ply", "rb").read() and "culled" not in capsys.readouterr().out
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24", "--cull_unseen", "--min_pixels", "2"]) == 0
    cv, cc, cf = mesh_render.cull_unseen(v, c, f, cams, 2)
    assert f"culled: {f.shape[0] - cf.shape[0]} of {f.shape[0]} triangles seen by no camera, {v.shape[0] - cv.shape[0]} vertices" in capsys.readouterr().out
    pv, pc, pf = mesh.read_mesh_ply(out)
    assert np.array_equal(_bits(pv), _bits(cv)) and np.array_equal(pc, cc.cpu().numpy()) and np.array_equal(pf, cf.cpu().numpy())
    # eval_mesh -m
    gt = str(tmp_path / "gt.ply")
    mesh.write_mesh_ply(gt, v, c, f[:0])
    res = eval_mesh.run(str(tmp_path / "plain.ply"), gt, 0.05, 1.0, 0.1, model_path=path, views="all")
    assert res["depth_agreement"]["median"] == stats["median"] and res["depth_agreement"]["pixels"] == n
    assert json.load(open(tmp_path / "mesh_results.json"))["depth_agreement"]["mean"] == stats["mean"]
    # spiral --mesh
    src = os.path.join(ROOT, "tests", "golden", "scene_llff")
    assert spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "8", "--video", "--fps", "10", "--mesh", out, "--shading", "normal"]) == 0
    pngs = sorted(os.listdir(os.path.join(path, "render", "mesh_scene_llff")))
    assert len(pngs) == 24 and not os.path.exists(os.path.join(path, "render", "ours_7"))
    Wv, Hv, fps, got = frames.avi_frames(os.path.join(path, "out_mesh_scene_llff.avi"))
    assert fps == 10.0 and len(got) == 8 and all(g[:2] == b"\xff\xd8" and g[-2:] == b"\xff\xd9" for g in got)
    assert frames.read_png(os.path.join(path, "render", "mesh_scene_llff", pngs[0])).shape == (Hv, Wv, 3)
    assert sorted(n for n in os.listdir(path) if n.endswith(".avi")) == ["out_cdepth_mesh_scene_llff.avi", "out_depth_mesh_scene_llff.avi", "out_mesh_scene_llff.avi"]
