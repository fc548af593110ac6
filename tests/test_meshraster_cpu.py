"""CPU: the yardstick of the mesh rasterizer (tests/meshraster_ref.py) against truths written out by hand, and the argument
checks of binocular3dgs_amd/mesh_render.py that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402
import meshraster_ref as rr  # noqa: E402
import simplify_ref as sr  # noqa: E402

F = np.float32
W, H = 16, 12
CAM = rr.camera_row()[None]


def _one(pix, z=1.0, faces=((0, 1, 2),), **kw):
    v = rr.at_pixels(pix, z, W, H)
    return rr.render(v, rr.grey(len(v)), np.array(faces, np.int32), CAM, W, H, **kw)


def test_a_triangle_with_vertices_on_pixel_centres():
    """(2,2) (10,2) (2,10): the top edge (j = 2) and the left edge (i = 2) belong to it, the hypotenuse i + j = 12 does not"""
    for pix in ([(2, 2), (10, 2), (2, 10)], [(2, 2), (2, 10), (10, 2)]):          # both windings
        out = _one(pix)
        want = np.zeros((H, W), bool)
        for j in range(H):
            for i in range(W):
                want[j, i] = i >= 2 and j >= 2 and i + j <= 11
        assert want.sum() == 36
        assert np.array_equal(out["alpha"][0, 0] == 1.0, want) and np.array_equal(out["triangle_id"][0] == 0, want)
        assert out["face_pixels"].tolist() == [36] and out["rejected"].tolist() == [0]
        assert (out["depth"][0, 0][want] == 1.0).all() and (out["depth"][0, 0][~want] == 0.0).all()


@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("reverse", [False, True])
def test_a_quad_of_two_triangles_covers_its_interior_exactly_once(diagonal, reverse):
    """corners on the pixel centres (3,2) (12,2) (12,9) (3,9): the pixels 3 <= i < 12, 2 <= j < 9 once each, no other"""
    q = [(3, 2), (12, 2), (12, 9), (3, 9)]
    tris = [(0, 1, 2), (0, 2, 3)] if diagonal == 0 else [(0, 1, 3), (1, 2, 3)]
    if reverse:
        tris = [t[::-1] for t in tris]
    hits = np.zeros((H, W), np.int64)
    for t in tris:
        hits += (_one(q, faces=(t,))["alpha"][0, 0] == 1.0)
    want = np.zeros((H, W), np.int64)
    want[2:9, 3:12] = 1
    assert np.array_equal(hits, want)
    both = _one(q, faces=tris)
    assert both["face_pixels"].sum() == 63 and np.array_equal(both["alpha"][0, 0], want.astype(F))


def test_zero_area_and_sub_pixel_triangles():
    assert _one([(2, 2), (6, 6), (10, 10)])["face_pixels"].tolist() == [0]                     # zero area
    assert _one([(4.25, 4.25), (4.75, 4.25), (4.25, 4.75)])["face_pixels"].tolist() == [0]      # no centre inside
    out = _one([(4.75, 4.75), (5.5, 4.75), (4.75, 5.5)])                                       # the centre (5, 5) only
    assert out["face_pixels"].tolist() == [1] and out["triangle_id"][0, 5, 5] == 0


def test_a_closed_outward_sphere_shows_only_faces_that_face_the_camera():
    v, c, f = sr.sphere_mesh()
    cams = rr.orbit_cameras(3, (12.0, 12.0, 12.0), 30.0, 60.0)
    out = rr.render(v, c, f, cams, 64, 48)
    culled = rr.render(v, c, f, cams, 64, 48, cull_backface=True)
    for k in ("triangle_id", "depth", "colour"):
        assert np.array_equal(out[k], culled[k])
    for n in range(3):
        seen = np.unique(out["triangle_id"][n][out["triangle_id"][n] >= 0])
        assert len(seen) > 100
        p = rr.camera_space(v, cams[n]).astype(np.float64)[f[seen]]
        normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert ((normal * p[:, 0]).sum(axis=1) < 0).all()
    # the same sphere wound inward: with the cull, only its far side is left
    inward = rr.render(v, c, f[:, ::-1].copy(), cams, 64, 48, cull_backface=True)
    m = out["alpha"] == 1.0
    assert np.array_equal(inward["alpha"], out["alpha"]) and (inward["depth"][m] > out["depth"][m]).all()


def test_depth_is_the_z_of_the_plane_at_the_pixel_ray():
    """fronto-parallel: z itself; tilted: d / (n . ray).  The vertices sit exactly on sub-pixel positions, so the bound is
    the rounding of the statements alone: three divisions, three products, two sums and the reciprocal, 2^-24 each, and the
    three b that need not sum to one exactly -- 16 * 2^-24 covers them."""
    tol = 16.0 * 2.0 ** -24
    flat = _one([(1.5, 0.75), (14.25, 2.5), (5.0, 10.5)], z=2.5)
    m = flat["alpha"][0, 0] == 1.0
    assert m.sum() > 30 and (np.abs(flat["depth"][0, 0][m].astype(np.float64) / 2.5 - 1.0) <= tol).all()
    pix, z = [(1.5, 0.75), (14.25, 2.5), (5.0, 10.5)], [1.0, 4.0, 2.0]
    tilted = _one(pix, z=z)
    p = rr.at_pixels(pix, z, W, H).astype(np.float64)
    n = np.cross(p[1] - p[0], p[2] - p[0])
    jj, ii = np.nonzero(tilted["alpha"][0, 0] == 1.0)
    ray = np.stack([(ii - (0.5 * W - 0.5)) / 16.0, (jj - (0.5 * H - 0.5)) / 16.0, np.ones(len(ii))], axis=1)
    want = (n @ p[0]) / (ray @ n)
    assert len(ii) > 30 and (np.abs(tilted["depth"][0, 0, jj, ii] / want - 1.0) <= tol).all()
    # colours: a vertex colour comes back at the vertex's own pixel, up to the same roundings
    v = rr.at_pixels([(2, 2), (12, 2), (2, 10)], [1.0, 2.0, 4.0], W, H)
    col = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
    out = rr.render(v, col, np.array([[0, 1, 2]], np.int32), CAM, W, H)
    assert np.allclose(out["colour"][0, :, 2, 2], [1.0, 0.0, 0.0], atol=1e-6)


def test_the_rasterizer_and_the_fusion_agree_on_where_a_pixel_is():
    """rint(X / 256) is the pixel the fusion assigns to a point, wherever the point is more than 1/256 px from a pixel boundary:
    for 1000 random points against the fusion's statement, and for the 1000 voxel centres of a volume through mesh_ref.integrate
    itself (an image whose colours are the pixel coordinates comes back in the volume)."""
    rng = np.random.default_rng(5)
    Wi, Hi = 40, 30
    cam = rr.orbit_cameras(1, (0.3, -0.2, 0.1), 4.0, 31.0, 29.0, height=-0.7)[0]
    pts = rng.uniform(-1.5, 1.5, size=(1000, 3)).astype(F)
    X, Y, pz, good, sx, sy = rr.project(pts, cam, Wi, Hi)
    assert good.all()
    clear = (np.abs(sx - np.floor(sx) - 0.5) > 1 / 256) & (np.abs(sy - np.floor(sy) - 0.5) > 1 / 256)
    assert clear.sum() > 950
    assert np.array_equal(np.rint(X / 256)[clear], np.rint(sx)[clear]) and np.array_equal(np.rint(Y / 256)[clear], np.rint(sy)[clear])
    vol = mr.new_volume((10, 10, 10), (-1.4, -1.3, -1.5), 0.29)
    jj, ii = np.mgrid[0:Hi, 0:Wi]
    image = np.stack([ii, jj, np.zeros_like(ii)]).astype(F)
    mr.integrate(vol, cam[None], [np.full((Hi, Wi), 1e6, F)], [np.ones((Hi, Wi), F)], [image], 1.0)
    px, py, pz_ = mr.centres(vol)
    grid = np.stack(np.broadcast_arrays(px[None, None, :], py[None, :, None], pz_[:, None, None]), axis=-1).reshape(-1, 3)
    X, Y, _, good, sx, sy = rr.project(grid, cam, Wi, Hi)
    seen = vol["weight"].reshape(-1) == 1.0
    clear = seen & (np.abs(sx - np.floor(sx) - 0.5) > 1 / 256) & (np.abs(sy - np.floor(sy) - 0.5) > 1 / 256)
    assert clear.sum() > 500
    rgb = vol["rgb"].reshape(-1, 3)
    assert np.array_equal(np.rint(X / 256)[clear], rgb[clear, 0]) and np.array_equal(np.rint(Y / 256)[clear], rgb[clear, 1])


def test_rejected_triangles_are_counted_not_drawn():
    v = rr.at_pixels([(2, 2), (10, 2), (2, 10), (3, 3), (9, 3), (3, 9)], [1, 1, 1, 2, 2, 0.125], W, H)
    out = rr.render(v, rr.grey(6), np.array([[0, 1, 2], [3, 4, 5], [0, 1, 6]], np.int32), CAM, W, H)
    assert out["rejected"].tolist() == [2] and out["bad"] == 1 and out["face_pixels"].tolist() == [36, 0, 0]


# ---- the python entry points: checks that need no device ----------------------------------------------------------------
def test_constants_mirror_the_header():
    from binocular3dgs_amd import _C, mesh_render
    assert (mesh_render.SMALL_BOX, mesh_render.WAVE_BOX) == (_C.MESH_SMALL_BOX, _C.MESH_WAVE_BOX) == (rr.SMALL_BOX, rr.WAVE_BOX)
    assert mesh_render.SHADINGS == {"colour": _C.MESH_SHADE_COLOUR, "normal": _C.MESH_SHADE_NORMAL}
    assert _C.mesh_raster_workspace_bytes(8, 1000, 2000, 64, 48) % 256 == 0
    assert _C.mesh_raster_workspace_bytes(9, 10, 10, 64, 48) == 0 and _C.mesh_raster_workspace_bytes(1, 10, 10, 16385, 48) == 0


def test_argument_checks_before_any_launch():
    import torch
    from binocular3dgs_amd import _C, _lib, mesh_render
    v, c, f = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32)
    table = np.tile(rr.camera_row(), (9, 1))
    with pytest.raises(ValueError, match="float32"):
        mesh_render.render_mesh(v.double(), c, f, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="int32"):
        mesh_render.render_mesh(v, c, f.long(), table[:1], size=(W, H))
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        mesh_render.render_mesh(v[:, :2], c, f, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="one per vertex"):
        mesh_render.render_mesh(v, c[:3], f, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="shading"):
        mesh_render.render_mesh(v, c, f, table[:1], size=(W, H), shading="phong")
    with pytest.raises(ValueError, match="needs the vertex colours"):
        mesh_render.render_mesh(v, None, f, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="size="):
        mesh_render.render_mesh(v, c, f, table[:1])
    with pytest.raises(ValueError, match="per side"):
        mesh_render.render_mesh(v, c, f, table[:1], size=(W, 20000))
    with pytest.raises(ValueError, match="min_pixels"):
        mesh_render.cull_unseen(v, c, f, table[:1], 0, size=(W, H))
    with pytest.raises(ValueError, match="views per launch"):
        mesh_render.raster_views(v, c, f, table, W, H)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):                 # no CPU path behind the module
        mesh_render.render_mesh(v, c, f, table[:1], size=(W, H))
    with pytest.raises(ValueError, match="1 .. 8 views"):
        _C.mesh_raster(v, f, torch.from_numpy(table), W, H)
    L = _lib.lib()
    assert L.b3gs_mesh_raster_batch(0, None, W, H, 4, 2, None, None, 0, -1, -1, None, None, None) == -1
    assert L.b3gs_mesh_raster_batch(1, None, W, H, 4, 2, None, None, 0, -1, -1, None, None, None) == -1
    assert L.b3gs_mesh_resolve_batch(1, None, W, 0, 4, 2, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
