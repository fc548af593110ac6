"""The mesh texture calls on the device (csrc/texture.hip, binocular3dgs_amd/mesh_texture.py) against the numpy restatement of
tests/texture_ref.py: the accumulator, the texture, the coverage, the bad-face count and the textured render are compared bit
for bit.  Images are 16x12 .. 64x48 and atlases a few thousand texels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402
import simplify_ref as sr  # noqa: E402
import texture_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 12
CAM = rr.camera_row()[None]
BG = (0.25, 0.5, 0.75)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _check(v, c, f, cams, w, h, images, n, Wt, slack, two_sided=False, ref=None):
    """accumulate (8 views per call), finalize, bake_texture and the textured render of one scene against the yardstick
    -> (texture, coverage, bad, accum) of the yardstick"""
    from binocular3dgs_amd import _C, mesh_texture
    cams = np.asarray(cams, F).reshape(-1, 14)
    want_tex, want_cov, want_bad, want_acc = tr.bake(v, c, f, cams, w, h, images, n, Wt, slack, two_sided, ref=ref)
    dv, df = _dev(v, F), _dev(f, np.int32)
    dc = None if c is None else _dev(c, np.uint8)
    dimg = _dev(images, F)
    accum = torch.zeros(want_acc.shape, device=DEV)
    for s in range(0, len(cams), 8):
        bad = mesh_texture.accumulate_views(dv, df, cams[s:s + 8], w, h, dimg[s:s + 8], accum, cell=n, slack=slack, two_sided=two_sided)
    assert np.array_equal(_bits(accum), _bits(want_acc)), f"accum: {(_bits(accum) != _bits(want_acc)).sum()} words differ"
    assert bad.tolist() == [want_bad]
    tex, cov = _C.mesh_texture_finalize(len(v), dc, df, n, Wt, accum)
    assert np.array_equal(tex.cpu().numpy(), want_tex) and cov.tolist() == want_cov
    tex2, cov2 = mesh_texture.bake_texture(dv, dc, df, cams, list(dimg), cell=n, width=Wt, slack=slack, two_sided=two_sided, size=(w, h))
    assert torch.equal(tex2, tex) and torch.equal(cov2, cov)                 # the whole bake again: the same bits
    part = cams[:8]
    rref = rr.render(v, None, f, part, w, h, shading="normal") if ref is None else {k: ref[k][:8] for k in ("triangle_id", "depth", "alpha")}
    want_col = tr.resolve_textured(v, f, part, w, h, rref, want_tex, n, BG)
    outs, _ = mesh_texture.render_textured(dv, df, tex, n, part, torch.tensor(BG, device=DEV), size=(w, h))
    for k, o in enumerate(outs):
        assert np.array_equal(o["triangle_id"].cpu().numpy(), rref["triangle_id"][k]) and np.array_equal(_bits(o["rendered_depth"]), _bits(rref["depth"][k]))
        assert np.array_equal(_bits(o["rendered_alpha"]), _bits(rref["alpha"][k]))
        assert np.array_equal(_bits(o["render"]), _bits(want_col[k])), f"view {k}: {(_bits(o['render']) != _bits(want_col[k])).sum()} words differ"
    return want_tex, want_cov, want_bad, want_acc


# ---- the layout on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Wt", [(4, 33), (9, 54)])
@pytest.mark.parametrize("nf", [1, 2, 3, 63, 64, 65])
def test_triangle_counts_cells_a_ragged_margin_and_row_seams(nf, n, Wt):
    """6 (5) cells per row and 3 (4) spare columns: 63 .. 65 triangles fill 6 (7) rows of cells, the last one partly"""
    v, c, f = rr.random_mesh(nf, 40, 30, nf + n)
    _, cov, _, _ = _check(v, c, f, CAM, 40, 30, tr.pattern(1, 40, 30, nf), n, Wt, 0.25, two_sided=True)
    assert cov[1] == nf * n * (n + 1) // 2 and (nf < 60 or cov[0] > cov[1] // 4)


# ---- views ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ball():
    """a sphere of 64 triangles from nine cameras at 32 x 24: the rasterizer's yardstick, computed once"""
    v, f = rr.uv_sphere((0.0, 0.0, 0.0), 2.0, 8, 5)
    cams = rr.orbit_cameras(9, (0.0, 0.0, 0.0), 7.0, 28.0, height=-2.0)
    return v, rr.grey(len(v), 8), f, cams, rr.render(v, None, f, cams, 32, 24, shading="normal"), tr.pattern(9, 32, 24, 9)


@pytest.mark.parametrize("ncam", [1, 8, 9])
def test_the_accumulator_carries_over_the_calls(ball, ncam):
    v, c, f, cams, ref, img = ball
    sub = {k: ref[k][:ncam] for k in ("triangle_id", "depth", "alpha")}
    _, cov, _, _ = _check(v, c, f, cams[:ncam], 32, 24, img[:ncam], 5, 6 * 7 + 1, 0.05, ref=sub)
    assert cov[1] == 64 * 15 and 0 < cov[0] < cov[1]
    assert (ncam == 1) == (cov[0] < cov[1] // 2)                             # one camera sees less than half of a sphere, a ring of them most


def test_two_image_sizes_in_one_bake(ball):
    from binocular3dgs_amd import mesh, mesh_texture
    from binocular3dgs_amd.camera import Camera, focal2fov
    v, c, f = ball[:3]
    sizes = [(32, 24), (32, 24), (20, 16)]
    cams = []
    for k, (w, h) in enumerate(sizes):
        row = rr.orbit_cameras(3, (0.0, 0.0, 0.0), 7.0, 28.0)[k].astype(np.float64)
        cams.append(Camera(row[:9].reshape(3, 3).T, row[9:12], focal2fov(28.0, w), focal2fov(28.0, h), w, h, uid=k, device=DEV))
    table = mesh.camera_table(cams)
    images = [tr.pattern(1, w, h, k)[0] for k, (w, h) in enumerate(sizes)]
    n, Wt = 5, 43
    accum = np.zeros((tr.atlas_height(len(f), n, Wt), Wt, 4), F)
    for a, b, (w, h) in ((0, 2, sizes[0]), (2, 3, sizes[2])):
        r = rr.render(v, None, f, table[a:b], w, h, shading="normal")
        tr.accumulate(accum, v, f, table[a:b], w, h, n, r["triangle_id"], r["depth"], np.stack(images[a:b]), 0.05)
    want_tex, want_cov = tr.finalize(accum, c, len(v), f, n)
    tex, cov = mesh_texture.bake_texture(_dev(v, F), _dev(c, np.uint8), _dev(f, np.int32), cams, [_dev(im, F) for im in images], cell=n, width=Wt, slack=0.05)
    assert np.array_equal(tex.cpu().numpy(), want_tex) and cov.tolist() == want_cov


def test_the_sphere_of_the_rasterizer_tests_from_three_cameras():
    v, c, f = sr.sphere_mesh()
    cams = rr.orbit_cameras(9, (12.0, 12.0, 12.0), 30.0, 60.0, 58.0, height=-4.0)[:3]
    n, Wt = 4, 40 * 5 + 2
    _, cov, _, _ = _check(v, c, f, cams, 64, 48, tr.pattern(3, 64, 48, 4), n, Wt, 0.5)
    assert cov[1] == len(f) * 10 and cov[1] // 3 < cov[0] < cov[1]


# ---- the statements one by one -------------------------------------------------------------------------------------------
def test_texels_that_project_exactly_onto_the_first_and_the_last_column():
    """the quad over the pixels (0,2) .. (12,6) with legs of 4 texels: texel (i, j) of triangle 1 is the pixel (3 (i + j), 2 + i),
    so the gutter i + j = 5 sits at sx = 15 = W - 1 and corner 0 at sx = 0, exactly: both are inside"""
    v, f = tr.quad(0, 2, 12, 6, 2.0, W, H)
    _, cov, _, accum = _check(v, None, f, CAM, W, H, tr.pattern(1, W, H, 1), 6, 7, 0.0)
    assert cov == [42, 42] and (accum[..., 3] > 0).all()
    # half a pixel to the right: sx = 15.5 for the six gutter texels of triangle 1 and for texel (0, 5) of triangle 0 (3 j + 0.5)
    v, f = tr.quad(0.5, 2, 12.5, 6, 2.0, W, H)
    _, cov, _, _ = _check(v, None, f, CAM, W, H, tr.pattern(1, W, H, 1), 6, 7, 0.0)
    assert cov == [42 - 7, 42]


def test_a_view_behind_the_near_plane_adds_nothing():
    v, f = tr.quad(2, 2, 6, 6, 2.0, W, H)
    near = rr.camera_row(t=(0.0, 0.0, -1.875))                        # the quad at z = 0.125 of this camera
    img = tr.pattern(2, W, H, 2)
    one = _check(v, None, f, CAM, W, H, img[:1], 6, 7, 0.0)
    two = _check(v, None, f, np.stack([CAM[0], near]), W, H, img, 6, 7, 0.0)
    assert np.array_equal(one[3], two[3]) and one[1] == two[1] == [42, 42]


def test_a_back_facing_view_with_and_without_two_sided():
    v, f = tr.quad(6, 4, 10, 8, 2.0, W, H, facing=False)
    img = tr.pattern(1, W, H, 3)
    c = rr.grey(4, 3)
    assert _check(v, c, f, CAM, W, H, img, 4, 5, 0.0)[1] == [0, 20]
    assert _check(v, c, f, CAM, W, H, img, 4, 5, 0.0, two_sided=True)[1] == [20, 20]


@pytest.mark.parametrize("colours", [True, False])
def test_two_parallel_quads_a_slack_below_and_above_their_distance(colours):
    va, fa = tr.quad(1, 1, 10, 8, 1.0, W, H)
    vb, fb = tr.quad(4, 3, 8, 6, 2.0, W, H)
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + 4]).astype(np.int32)
    c = rr.grey(8, 5) if colours else None
    img = tr.pattern(1, W, H, 5)
    assert _check(v, c, f, CAM, W, H, img, 6, 14, 0.5)[1] == [42, 84]        # B is seen by no view: the vertex colours, or 0
    assert _check(v, c, f, CAM, W, H, img, 6, 14, 1.5)[1] == [84, 84]


def test_a_sub_pixel_triangle_that_wins_no_pixel_is_still_textured():
    vq, fq = tr.quad(1, 1, 10, 8, 2.0, W, H)
    vt = rr.at_pixels([(4.25, 4.25), (4.25, 4.75), (4.75, 4.25)], 1.0, W, H)
    v, f = np.concatenate([vq, vt]), np.concatenate([fq, [[4, 5, 6]]]).astype(np.int32)
    ref = rr.render(v, None, f, CAM, W, H, shading="normal")
    assert ref["face_pixels"].tolist()[2] == 0
    tex, cov, _, accum = _check(v, rr.grey(7, 6), f, CAM, W, H, tr.pattern(1, W, H, 6), 6, 14, 0.0, ref=ref)
    owner, _, _ = tr.owners(3, 6, 14)
    assert cov == [63, 63] and (accum[..., 3][owner == 2] > 0.9).all()


def test_a_bad_index_and_a_nan_vertex_are_counted_and_disturb_nothing():
    vq, fq = tr.quad(2, 2, 6, 6, 2.0, W, H)
    v = np.concatenate([vq, np.array([[0.1, 0.1, 2.0], [0.2, np.nan, 2.0], [0.1, 0.3, 2.0]], F)])
    f = np.concatenate([fq, [[0, 1, 7], [4, 5, 6], [-1, 1, 2]]]).astype(np.int32)
    c = rr.grey(7, 7)
    img = tr.pattern(1, W, H, 7)
    tex, cov, bad, accum = _check(v, c, f, CAM, W, H, img, 6, 14, 0.0)
    alone = tr.bake(vq, c[:4], fq, CAM, W, H, img, 6, 14, 0.0)
    owner, _, _ = tr.owners(5, 6, 14)
    assert bad == 2 and cov == [42, 5 * 21] and np.array_equal(tex[:6, :7], alone[0][:, :7]) and (accum[owner >= 2] == 0).all()
    assert (tex[(owner == 2) | (owner == 4)] == 0).all()               # a bad index: no fallback either


# ---- graphs --------------------------------------------------------------------------------------------------------------
def test_the_three_calls_replay_from_a_graph_onto_changed_images():
    from binocular3dgs_amd import _C, mesh_texture
    v, c, f = rr.random_mesh(40, 40, 30, 31, span=9.0)
    n, Wt = 5, 6 * 6
    dv, dc, df = _dev(v, F), _dev(c, np.uint8), _dev(f, np.int32)
    images = [tr.pattern(1, 40, 30, s) for s in (41, 42)]
    dimg = _dev(images[0], F)
    accum = torch.zeros(tr.atlas_height(40, n, Wt), Wt, 4, device=DEV)
    bg = torch.tensor(BG, device=DEV)

    def calls():
        accum.zero_()
        mesh_texture.accumulate_views(dv, df, CAM, 40, 30, dimg, accum, cell=n, slack=0.25, two_sided=True)
        tex, cov = _C.mesh_texture_finalize(len(v), dc, df, n, Wt, accum)
        return tex, cov, mesh_texture.raster_views_textured(dv, df, tex, n, CAM, 40, 30, bg)[3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tex, cov, colour = calls()
    rref = rr.render(v, None, f, CAM, 40, 30, shading="normal")
    for k in (1, 0):
        dimg.copy_(torch.from_numpy(images[k]))
        graph.replay()
        want_tex, want_cov, _, _ = tr.bake(v, c, f, CAM, 40, 30, images[k], n, Wt, 0.25, True, ref=rref)
        assert np.array_equal(tex.cpu().numpy(), want_tex) and cov.tolist() == want_cov
        assert np.array_equal(_bits(colour), _bits(tr.resolve_textured(v, f, CAM, 40, 30, rref, want_tex, n, BG)))


# ---- what it is for ------------------------------------------------------------------------------------------------------
def test_a_textured_plane_is_closer_to_the_picture_than_its_vertex_colours():
    """two triangles, one frontal camera, a checker of 6-pixel squares: the PSNR of the textured render against the picture
    exceeds that of the vertex-colour render (a condition, not a tolerance; fp64 on the returned tensors)"""
    from binocular3dgs_amd import mesh_render, mesh_texture
    w, h = 64, 48
    v, f = tr.quad(5.5, 4.5, 57.5, 42.5, 2.0, w, h)
    jj, ii = np.mgrid[0:h, 0:w]
    checker = ((ii // 6 + jj // 6) % 2).astype(F)
    img = np.stack([checker, 1 - checker, 0.5 * checker + 0.25]).astype(F)
    corner = np.array([img[:, int(y), int(x)] for x, y in ((5, 4), (57, 4), (57, 42), (5, 42))])
    dv, df, dc = _dev(v, F), _dev(f, np.int32), _dev(np.rint(corner * 255), np.uint8)
    n, Wt = mesh_texture.atlas_for(2, 128)
    tex, cov = mesh_texture.bake_texture(dv, dc, df, CAM, [_dev(img, F)], cell=n, width=Wt, slack=2.0 ** -10, size=(w, h))
    assert cov.tolist() == [n * (n + 1), n * (n + 1)]
    bg = torch.zeros(3, device=DEV)
    textured = mesh_texture.render_textured(dv, df, tex, n, CAM, bg, size=(w, h))[0][0]["render"]
    plain = mesh_render.render_mesh(dv, dc, df, CAM, bg, size=(w, h))[0][0]["render"]
    target = torch.from_numpy(img).to(DEV).double()

    def psnr(x):
        return float(-10.0 * torch.log10(((x.double() - target) ** 2).mean()))
    print(f"PSNR against the picture: textured {psnr(textured):.2f} dB, vertex colours {psnr(plain):.2f} dB")
    assert psnr(textured) > psnr(plain)


# ---- the command lines ---------------------------------------------------------------------------------------------------
def test_extract_mesh_texture_and_spiral_on_the_obj(tmp_path, capsys):
    from binocular3dgs_amd import extract_mesh, frames, mesh, mesh_texture, mesh_tools, spiral
    from test_gpu_meshraster import _shell_model
    path, model, cams = _shell_model(tmp_path)
    bg = torch.zeros(3, device=DEV)
    v, c, f, vol = mesh.fuse_model(model, cams, bg, resolution=24, return_volume=True)
    out_dir = os.path.join(path, "mesh", "iteration_7")
    # without --texture: the parent's bytes and lines, and no OBJ
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24"]) == 0
    mesh.write_mesh_ply(str(tmp_path / "plain.ply"), v, c, f)
    assert open(os.path.join(out_dir, "mesh.ply"), "rb").read() == open(tmp_path / "plain.ply", "rb").read()
    assert "texture (" not in capsys.readouterr().out and sorted(os.listdir(out_dir)) == ["mesh.ply"]
    # with it, after a simplification: the OBJ holds the simplified mesh and the atlas of bake_texture
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24", "--simplify", "2", "--texture", "--atlas_side", "256"]) == 0
    printed = capsys.readouterr().out
    sv, sc, sf = mesh_tools.simplify(v, c, f, 2.0 * vol.voxel_size)
    n, Wt = mesh_texture.atlas_for(sf.shape[0], 256)
    assert sorted(os.listdir(out_dir)) == ["mesh.mtl", "mesh.obj", "mesh.ply", "mesh.png"]
    ov, of, otex, on = mesh_texture.read_textured_obj(os.path.join(out_dir, "mesh.obj"))
    assert on == n and otex.shape[1] == Wt and np.array_equal(_bits(ov), _bits(sv)) and np.array_equal(of, sf.cpu().numpy())
    from binocular3dgs_amd.evaluate import render_views
    tex, cov = mesh_texture.bake_texture(sv, sc, sf, cams, render_views(model, cams, bg), cell=n, width=Wt, slack=2.0 * vol.voxel_size)
    assert np.array_equal(otex, tex.cpu().numpy())
    seen, owned = cov.tolist()
    assert f"cell {n}, atlas {Wt} x {otex.shape[0]}, {seen} of {owned} texels" in printed and seen > owned // 2
    with pytest.raises(SystemExit):
        extract_mesh.main(["-m", path, "--views", "all", "--two_sided"])
    capsys.readouterr()
    # spiral --mesh mesh.obj
    src = os.path.join(ROOT, "tests", "golden", "scene_llff")
    obj = os.path.join(out_dir, "mesh.obj")
    assert spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "4", "--mesh", obj]) == 0
    assert "(texture)" in capsys.readouterr().out
    pngs = sorted(os.listdir(os.path.join(path, "render", "mesh_scene_llff")))
    assert len(pngs) == 12 and frames.read_png(os.path.join(path, "render", "mesh_scene_llff", pngs[0])).ndim == 3
    with pytest.raises(ValueError, match="texture goes with"):
        spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "4", "--mesh", os.path.join(out_dir, "mesh.ply"), "--shading", "texture"])
    with pytest.raises(ValueError, match="texture goes with"):
        spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "4", "--mesh", obj, "--shading", "normal"])
