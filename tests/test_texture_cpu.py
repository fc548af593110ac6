"""CPU: the yardstick of the mesh texture calls (tests/texture_ref.py) and the host code of binocular3dgs_amd/mesh_texture.py
against truths written out by hand: the atlas layout, the bilinear-footprint property the layout exists for, two small bakes,
the OBJ files and every argument check that needs no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402
import texture_ref as tr  # noqa: E402

F = np.float32
W, H = 16, 12
CAM = rr.camera_row()[None]


# ---- the layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5])
def test_every_texel_of_a_cell_is_owned_once_and_the_halves_are_equal(n):
    from binocular3dgs_amd import mesh_texture
    f, i, j = tr.owners(2, n, n + 1)                                  # one cell, both triangles
    assert f.shape == (n, n + 1) == mesh_texture.atlas_size(2, n, n + 1)[::-1]
    for y in range(n):
        for x in range(n + 1):                                        # written out: the anti-diagonal x + y = n starts the odd half
            assert f[y, x] == (0 if x + y <= n - 1 else 1)
            assert (i[y, x], j[y, x]) == ((x, y) if x + y <= n - 1 else (n - x, n - 1 - y))
    assert (f == 0).sum() == (f == 1).sum() == n * (n + 1) // 2
    # both halves hold the same set of local indices: the odd half is the even half turned by 180 degrees
    assert sorted(zip(i[f == 0], j[f == 0])) == sorted(zip(i[f == 1], j[f == 1]))
    # with one triangle the odd half is unowned, and so is a ragged right margin
    f1, _, _ = tr.owners(1, n, n + 3)
    assert (f1[:, :n + 1] == np.where(f == 0, 0, -1)).all() and (f1[:, n + 1:] == -1).all()


def test_the_corners_of_the_first_cells_written_out():
    c = tr.corners(3, 4, 11)                                          # two cells of 5 x 4 per row, one spare column
    assert c[0].tolist() == [[0, 0], [2, 0], [0, 2]] and c[1].tolist() == [[4, 3], [2, 3], [4, 1]] and c[2].tolist() == [[5, 0], [7, 0], [5, 2]]
    from binocular3dgs_amd import mesh_texture
    assert np.array_equal(mesh_texture.face_corners(3, 4, 11), c)
    c = tr.corners(5, 6, 15)                                          # a second row of cells
    assert c[4].tolist() == [[0, 6], [4, 6], [0, 10]] and np.array_equal(mesh_texture.face_corners(5, 6, 15), c)


@pytest.mark.parametrize("n", [4, 5, 8])
def test_a_bilinear_fetch_inside_a_triangle_reads_its_own_texels_only(n):
    """every point of a lattice of step 1/8 inside (and on the border of) the UV triangle, for the four triangles of two cells:
    each texel of the footprint with a weight above 0 belongs to the triangle.  With legs of n - 1 the same check fails."""
    nf, Wt = 4, 2 * (n + 1) + 1
    Ht = tr.atlas_height(nf, n, Wt)
    owner, _, _ = tr.owners(nf, n, Wt)
    steps = 8

    def leaks(corner, leg):
        bad = 0
        for f in range(nf):
            o, a, b = (np.array(corner[f][k], dtype=np.float64) for k in range(3))
            ea, eb = (a - o) / (n - 2) * leg, (b - o) / (n - 2) * leg
            for p in range(steps + 1):
                for q in range(steps + 1 - p):
                    x, y = o + ea * p / steps + eb * q / steps
                    for tx, ty, w in tr.bilinear_footprint(x, y, Wt, Ht):
                        bad += w > 0 and owner[ty, tx] != f
        return bad
    corner = tr.corners(nf, n, Wt)
    assert leaks(corner, n - 2) == 0
    assert leaks(corner, n - 1) > 0


def test_atlas_size_around_a_full_row_of_cells():
    from binocular3dgs_amd import _C, _lib, mesh_texture
    n, Wt = 4, 23                                                     # 4 cells per row and 3 spare columns
    want = {1: 4, 2: 4, 3: 4, 7: 4, 8: 4, 9: 8}
    for nf, Ht in want.items():
        assert mesh_texture.atlas_size(nf, n, Wt) == (Wt, Ht) and tr.atlas_height(nf, n, Wt) == Ht
        assert _C.mesh_texture_atlas_height(nf, n, Wt) == Ht == _lib.lib().b3gs_mesh_texture_atlas_height(nf, n, Wt)
    assert mesh_texture.atlas_size(100000, 9, 4090) == (4090, 9 * 123)          # 409 cells per row, 50000 cells
    assert (mesh_texture.MIN_CELL, mesh_texture.MAX_CELL, mesh_texture.MAX_SIDE) == (_C.TEXTURE_MIN_CELL, _C.TEXTURE_MAX_CELL, _C.MAX_ATLAS_SIDE) \
        == (tr.MIN_CELL, tr.MAX_CELL, tr.MAX_SIDE)


def test_atlas_for_gives_the_largest_cell_that_fits_the_square():
    from binocular3dgs_amd import mesh_texture
    assert mesh_texture.atlas_for(2, 64) == (63, 64)                  # one cell of 64 x 63
    assert mesh_texture.atlas_for(8, 64) == (31, 64)                  # two cells per row, two rows: 64 x 62
    assert mesh_texture.atlas_for(2, 4096) == (256, 4096 // 257 * 257)
    n, Wt = mesh_texture.atlas_for(100000, 4096)
    assert mesh_texture.atlas_size(100000, n, Wt)[1] <= 4096 and not 0 < mesh_texture._height(100000, n + 1, 4096 // (n + 2) * (n + 2)) <= 4096
    assert n == 17                                                    # 227 cells per row, 221 rows of 17: 3757; 18 needs 232 rows: 4176
    with pytest.raises(ValueError, match="do not fit"):
        mesh_texture.atlas_for(100000, 256)


def test_the_atlas_limits_are_errors_that_name_the_largest_cell():
    from binocular3dgs_amd import _C, _lib, mesh_texture
    for nf, n, Wt in ((2, 3, 64), (2, 257, 4096), (2, 8, 8), (2, 8, 16385), (0, 8, 64)):
        with pytest.raises(ValueError, match="no atlas"):
            mesh_texture.atlas_size(nf, n, Wt)
        assert _C.mesh_texture_atlas_height(nf, n, Wt) == 0
    # 40000 triangles at width 100: cell 8 has 11 cells per row, 1819 rows, 14552 texels; cell 9 has 10 and 2000, 18000 > 16384
    assert mesh_texture.atlas_size(40000, 8, 100) == (100, 14552)
    with pytest.raises(ValueError, match="largest cell that fits this width is 8"):
        mesh_texture.atlas_size(40000, 9, 100)
    L = _lib.lib()
    assert L.b3gs_mesh_texture_accumulate_batch(1, None, W, H, 4, 40000, None, None, 9, 100, 18000, None, None, None, 0.0, 0, None, None, None) == -1
    assert b"largest cell that fits this width is 8" in L.b3gs_last_error()
    assert L.b3gs_mesh_texture_finalize(4, 2, None, None, 3, 64, 3, None, None, None, None) == -1
    assert L.b3gs_mesh_texture_finalize(4, 2, None, None, 4, 64, 5, None, None, None, None) == -1 and b"height" in L.b3gs_last_error()
    assert L.b3gs_mesh_resolve_textured_batch(1, None, W, H, 4, 2, None, None, None, None, None, 4, 64, 4, None, None, None, None, None, None) == -1


# ---- bakes with a known answer -------------------------------------------------------------------------------------------
def test_a_fronto_parallel_quad_on_the_pixel_lattice_takes_the_image_exactly():
    """cell 6, legs of 4 texels, over the pixels (2,2) .. (6,6): texel (i, j) of triangle 0 = (p0, p3, p2) is the pixel
    (2 + j, 2 + i + j), of triangle 1 = (p0, p2, p1) the pixel (2 + i + j, 2 + i); the gutter (i + j = 5) lies a pixel past the
    quad's edge, over empty pixels.  The image holds multiples of 1 / 255: the texture is the image, texel for pixel."""
    n = 6
    v, f = tr.quad(2, 2, 6, 6, 2.0, W, H)
    img = tr.pattern(1, W, H, 3)
    tex, cov, bad, _ = tr.bake(v, None, f, CAM, W, H, img, n, n + 1, 0.0)
    assert tex.shape == (6, 7, 3) and cov == [42, 42] and bad == 0
    want = np.rint(img[0] * 255).astype(np.uint8)
    for j in range(n):
        for i in range(n + 1):
            if i + j <= n - 1:
                assert tex[j, i].tolist() == want[:, 2 + i + j, 2 + j].tolist(), (i, j)
            else:
                ii, jj = n - i, n - 1 - j
                assert tex[j, i].tolist() == want[:, 2 + ii, 2 + ii + jj].tolist(), (i, j)
    # rendered through the atlas from the same camera, every covered pixel gets its own image value back
    ref = rr.render(v, None, f, CAM, W, H, shading="normal")
    out = tr.resolve_textured(v, f, CAM, W, H, ref, tex, n, bg=(0.5, 0.5, 0.5))
    m = ref["alpha"][0, 0] == 1.0
    assert m.sum() == 16 and np.array_equal(np.rint(out[0][:, m] * 255), np.rint(img[0][:, m] * 255)) and (out[0][:, ~m] == 0.5).all()


def test_a_hidden_quad_keeps_its_vertex_colours_and_coverage_says_so():
    """A over the pixels (1,1) .. (10,8) at z = 1, B over (4,3) .. (8,6) at z = 2.  The gutter of a patch reaches a quarter of
    a leg past the edge opposite corner 0: A's stays inside the image (over empty pixels, so it is seen), B's inside A's outline."""
    n = 6
    va, fa = tr.quad(1, 1, 10, 8, 1.0, W, H)
    vb, fb = tr.quad(4, 3, 8, 6, 2.0, W, H)
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + 4]).astype(np.int32)
    col = np.array([[200, 0, 0]] * 4 + [[10, 20, 30]] * 4, np.uint8)
    img = np.full((1, 3, H, W), 128.0 / 255.0, F)
    Wt = 2 * (n + 1)
    tex, cov, _, _ = tr.bake(v, col, f, CAM, W, H, img, n, Wt, 0.5)
    owner, _, _ = tr.owners(4, n, Wt)
    assert cov == [42, 84]
    assert (tex[owner < 2] == 128).all() and (tex[owner >= 2] == [10, 20, 30]).all()
    tex, cov, _, _ = tr.bake(v, col, f, CAM, W, H, img, n, Wt, 1.5)   # a slack beyond their distance: B is "seen" through A
    assert cov == [84, 84] and (tex == 128).all()
    tex, cov, _, _ = tr.bake(v, None, f, CAM, W, H, img, n, Wt, 0.5)  # no colours: the fallback is black
    assert cov == [42, 84] and (tex[owner >= 2] == 0).all()
    # interpolated vertex colours at the corners and in the clamped gutter
    col[4:] = [[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]]
    tex, _, _, _ = tr.bake(v, col, f, CAM, W, H, img, n, Wt, 0.5)
    c2 = tr.corners(4, n, Wt)[2].astype(int)                          # triangle 2 = vertices (4, 7, 6)
    assert [tex[y, x].tolist() for x, y in c2] == [[255, 0, 0], [255, 255, 255], [0, 0, 255]]
    x, y = c2[0] + [3, 2]                                             # (i, j) = (3, 2): b = (-1/4, 3/4, 1/2) -> (0, 3/5, 2/5)
    assert tex[y, x].tolist() == [153, 153, 255]


def test_weights_follow_the_squared_cosine_and_back_faces_are_skipped():
    n = 4
    v, f = tr.quad(6, 4, 10, 8, 2.0, W, H, facing=False)
    img = np.full((1, 3, H, W), 1.0, F)
    _, cov, _, accum = tr.bake(v, None, f, CAM, W, H, img, n, n + 1, 0.0)
    assert cov == [0, 20] and (accum == 0).all()
    _, cov, _, accum = tr.bake(v, None, f, CAM, W, H, img, n, n + 1, 0.0, two_sided=True)
    assert cov == [20, 20]
    q = rr.at_pixels([(6, 4)], 2.0, W, H)[0].astype(np.float64)       # corner 0 of triangle 0: texel (0, 0)
    cos2 = (q[2] / np.linalg.norm(q)) ** 2
    assert abs(accum[0, 0, 3] - cos2) < 1e-6 and abs(accum[0, 0, 0] - cos2) < 1e-6


# ---- the files -----------------------------------------------------------------------------------------------------------
def test_obj_round_trip_is_byte_identical_and_the_vt_are_the_atlas(tmp_path):
    from binocular3dgs_amd import mesh_texture
    rng = np.random.default_rng(7)
    v = rng.normal(size=(5, 3)).astype(F)
    f = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
    n, Wt = 4, 11
    tex = rng.integers(0, 256, size=(4, Wt, 3)).astype(np.uint8)
    path = str(tmp_path / "mesh.obj")
    assert mesh_texture.write_textured_obj(path, v, f, tex, n) == path
    assert sorted(os.listdir(tmp_path)) == ["mesh.mtl", "mesh.obj", "mesh.png"]
    lines = open(path).read().split("\n")
    assert lines[0] == "# b3gs_atlas cell 4 width 11" and lines[1] == "mtllib mesh.mtl" and "map_Kd mesh.png" in open(tmp_path / "mesh.mtl").read().split("\n")
    vt = [tuple(float(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("vt ")]
    # triangle 0: corners (0,0) (2,0) (0,2) of a 11 x 4 atlas; triangle 1, the odd half: (4,3) (2,3) (4,1); triangle 2: (5,0) (7,0) (5,2)
    want = [(0.5 / 11, 0.875), (2.5 / 11, 0.875), (0.5 / 11, 0.375), (4.5 / 11, 0.125), (2.5 / 11, 0.125), (4.5 / 11, 0.625),
            (5.5 / 11, 0.875), (7.5 / 11, 0.875), (5.5 / 11, 0.375)]
    assert len(vt) == 9 and np.array_equal(np.array(vt, F), np.array(want, F))
    assert [ln for ln in lines if ln.startswith("f ")] == ["f 1/1 2/2 3/3", "f 3/4 2/5 4/6", "f 5/7 1/8 4/9"]
    gv, gf, gt, gn = mesh_texture.read_textured_obj(path)
    assert gn == n and np.array_equal(gv.view(np.uint32), v.view(np.uint32)) and np.array_equal(gf, f) and np.array_equal(gt, tex)
    again = str(tmp_path / "again" / "mesh.obj")
    os.makedirs(tmp_path / "again")
    mesh_texture.write_textured_obj(again, gv, gf, gt, gn)
    for name in ("mesh.obj", "mesh.mtl", "mesh.png"):
        assert open(tmp_path / name, "rb").read() == open(tmp_path / "again" / name, "rb").read(), name
    # anything else raises
    text = open(path).read()
    for k, broken in enumerate((text.replace("# b3gs_atlas cell 4 width 11\n", ""), text.replace("usemtl atlas\n", ""),
                                text.replace("f 3/4 2/5 4/6", "f 3/4 2/5 4/7"), text.replace("f 5/7 1/8 4/9\n", ""),
                                text.replace("vt " + repr(float(F(0.5 / 11))), "vt 0.25", 1), text.replace("f 1/1", "f 9/1"),
                                text.replace("cell 4", "cell 5"), text + "o more\n")):
        other = str(tmp_path / "again" / "mesh.obj")
        with open(other, "w") as fp:
            fp.write(broken)
        with pytest.raises(ValueError):
            mesh_texture.read_textured_obj(other)
    with pytest.raises(ValueError, match=".obj"):
        mesh_texture.write_textured_obj(str(tmp_path / "mesh.ply"), v, f, tex, n)
    with pytest.raises(ValueError, match="outside"):
        mesh_texture.write_textured_obj(path, v, f + 3, tex, n)
    with pytest.raises(ValueError):
        mesh_texture.write_textured_obj(path, v, f, tex[:3], n)


# ---- the python entry points: checks that need no device ----------------------------------------------------------------
def test_argument_checks_before_any_launch():
    import torch
    from binocular3dgs_amd import _C, _lib, mesh_texture
    v, c, f = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32)
    table = np.tile(rr.camera_row(), (9, 1))
    img = [torch.zeros(3, H, W)]
    kw = dict(cell=4, width=5, slack=0.0, size=(W, H))
    bake = mesh_texture.bake_texture
    with pytest.raises(ValueError, match="float32"):
        bake(v.double(), c, f, table[:1], img, **kw)
    with pytest.raises(ValueError, match="int32"):
        bake(v, c, f.long(), table[:1], img, **kw)
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        bake(v[:, :2], c, f, table[:1], img, **kw)
    with pytest.raises(ValueError, match="one per vertex"):
        bake(v, c[:3], f, table[:1], img, **kw)
    with pytest.raises(ValueError, match="2 images for 1 cameras"):
        bake(v, c, f, table[:1], img * 2, **kw)
    with pytest.raises(ValueError, match="its camera 16 x 12"):
        bake(v, c, f, table[:1], [torch.zeros(3, H, W + 1)], **kw)
    with pytest.raises(ValueError, match=r"float32 \[3, H, W\]"):
        bake(v, c, f, table[:1], [torch.zeros(3, H, W, dtype=torch.float64)], **kw)
    with pytest.raises(ValueError, match=r"float32 \[3, H, W\]"):
        bake(v, c, f, table[:1], [torch.zeros(1, H, W)], **kw)
    for slack in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="slack"):
            bake(v, c, f, table[:1], img, **dict(kw, slack=slack))
    with pytest.raises(TypeError):
        bake(v, c, f, table[:1], img, cell=4, width=5, size=(W, H))              # slack is required
    with pytest.raises(ValueError, match="largest cell"):
        bake(v, c, f, table[:1], img, **dict(kw, cell=3))
    with pytest.raises(ValueError, match="largest cell"):
        bake(v, c, f, table[:1], img, **dict(kw, width=4))
    with pytest.raises(ValueError, match="size="):
        bake(v, c, f, table[:1], img, cell=4, width=5, slack=0.0)
    with pytest.raises(ValueError, match="per side"):
        bake(v, c, f, table[:1], img, **dict(kw, size=(W, 20000)))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):                 # no CPU path behind the module
        bake(v, c, f, table[:1], img, **kw)
    tex = torch.zeros(4, 5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"uint8 \[Ht, Wt, 3\]"):
        mesh_texture.render_textured(v, f, tex.float(), 4, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="not the atlas"):
        mesh_texture.render_textured(v, f, tex[:3], 4, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="largest cell"):
        mesh_texture.render_textured(v, f, tex, 5, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="int32"):
        next(mesh_texture.batches_textured(v, f.long(), tex, 4, table[:1], size=(W, H)))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mesh_texture.render_textured(v, f, tex, 4, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="1 .. 8 views"):
        _C.mesh_texture_accumulate(v, f, torch.from_numpy(table), W, H, 4, 5, torch.zeros(9, H, W, dtype=torch.int32), torch.zeros(9, 1, H, W),
                                   torch.zeros(9, 3, H, W), 0.0, False, torch.zeros(4, 5, 4))
