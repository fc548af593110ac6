"""CPU: the mesh smoothing stage without a device -- the yardstick (tests/meshsmooth_ref.py) on hand-checked meshes and its
properties, the C ABI's argument checks, the python surface's errors, the command lines' parser errors and the PLY normals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshsmooth_ref as sm  # noqa: E402

F = np.float32
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("b3gs_mesh_adjacency_workspace_bytes", "b3gs_mesh_adjacency_layout", "b3gs_mesh_adjacency_build", "b3gs_mesh_smooth",
       "b3gs_mesh_vertex_normals", "b3gs_mesh_resolve_shaded_batch")


# ---- hand-checked topology -----------------------------------------------------------------------------------------------
def test_one_triangle():
    t = sm.topology(*sm.TRIANGLE)
    assert (t["edges"], t["boundary_edges"], t["non_manifold_edges"], t["pinned_vertices"], t["isolated_vertices"]) == (3, 3, 0, 3, 0)
    assert t["euler"] == 1 and not t["closed"] and t["pinned"].tolist() == [1, 1, 1]
    assert [sm.neighbours(t, i) for i in range(3)] == [[1, 2], [0, 2], [0, 1]]
    assert [sm.incident(t, i) for i in range(3)] == [[0], [0], [0]]


def test_tetrahedron():
    t = sm.topology(*sm.TETRAHEDRON)
    assert t["edges"] == 6 and t["closed"] and t["euler"] == 2 and t["pinned_vertices"] == 0
    assert [sm.neighbours(t, i) for i in range(4)] == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]
    assert t["offsets"].tolist() == [0, 3, 6, 9, 12]
    assert [sm.incident(t, i) for i in range(4)] == [[0, 1, 3], [0, 1, 2], [0, 2, 3], [1, 2, 3]]


@pytest.mark.parametrize("mesh", [sm.TWO_TRIANGLES, sm.TWO_TRIANGLES_FLIPPED])
def test_two_triangles_on_one_edge(mesh):
    t = sm.topology(*mesh)
    assert t["edges"] == 5 and t["boundary_edges"] == 4 and t["non_manifold_edges"] == 0
    assert t["pinned_vertices"] == 4 and sm.neighbours(t, 0) == [1, 2, 3] and sm.neighbours(t, 1) == [0, 2]
    assert t["euler"] == 1


def test_three_triangles_on_one_edge():
    t = sm.topology(*sm.THREE_ON_AN_EDGE)
    assert t["non_manifold_edges"] == 1 and t["edges"] == 7 and t["boundary_edges"] == 6 and not t["closed"]
    assert sm.neighbours(t, 0) == [1, 2, 3, 4]


def test_a_face_listed_twice_reads_as_closed():
    t = sm.topology(*sm.TWICE)
    assert t["edges"] == 3 and t["edge_faces"].tolist() == [2, 2, 2] and t["closed"] and t["bad_faces"] == 0 and t["pinned_vertices"] == 0
    assert sm.incident(t, 0) == [0, 1]


def test_a_degenerate_face():
    t = sm.topology(*sm.DEGENERATE)
    assert t["edges"] == 1 and sm.incident(t, 0) == [0] and sm.incident(t, 1) == [0] and sm.neighbours(t, 0) == [1]
    assert t["isolated_vertices"] == 1 and sm.neighbours(t, 2) == []


def test_an_isolated_vertex_and_a_bad_face():
    t = sm.topology(*sm.with_isolated(sm.TETRAHEDRON))
    assert t["isolated_vertices"] == 1 and t["euler"] == 2 and t["offsets"].tolist() == [0, 3, 6, 9, 12, 12]
    good = sm.topology(*sm.TETRAHEDRON)
    t = sm.topology(*sm.with_bad_face(sm.TETRAHEDRON))
    assert t["bad_faces"] == 2 and t["good_faces"] == 4
    for key in ("offsets", "indices", "pinned", "inc_faces"):
        assert np.array_equal(t[key], good[key]), key
    assert sm.topology(np.zeros((0, 3), F), np.zeros((0, 3), np.int32))["totals"] == [0] * 8


# ---- properties of the yardstick -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noisy_sphere():
    v, f = sm.icosphere(3, noise=0.02, seed=4)
    assert v.shape == (642, 3) and f.shape == (1280, 3)
    return v, f, sm.topology(v, f)


def test_smoothing_lowers_the_radial_noise_and_taubin_keeps_the_radius(noisy_sphere):
    v, f, topo = noisy_sphere
    assert topo["closed"] and topo["euler"] == 2
    rms0, mean0 = sm.radial_rms(v)
    taubin = sm.smooth(v, f, 10, 0.5, -0.53, topo=topo)
    laplace = sm.smooth(v, f, 10, 0.5, 0.0, topo=topo)
    rms1, mean1 = sm.radial_rms(taubin)
    _, mean2 = sm.radial_rms(laplace)
    assert rms1 < rms0
    assert abs(mean1 - mean0) < abs(mean2 - mean0)


def test_pinned_vertices_stay_and_no_iteration_is_the_identity(noisy_sphere):
    v, f = sm.grid(12, 9, noise=0.3, seed=2)
    topo = sm.topology(v, f)
    assert topo["pinned_vertices"] == 2 * 12 + 2 * 9 - 4 and topo["boundary_edges"] == 2 * 11 + 2 * 8
    out = sm.smooth(v, f, 4, topo=topo)
    keep = topo["pinned"] == 1
    assert np.array_equal(out[keep].view(np.uint32), v[keep].view(np.uint32)) and (out[~keep] != v[~keep]).any()
    free = sm.smooth(v, f, 4, pin_boundary=False, topo=topo)
    assert (free[keep] != v[keep]).any()
    sv, sf, stopo = noisy_sphere
    assert np.array_equal(sm.smooth(sv, sf, 0, topo=stopo).view(np.uint32), sv.view(np.uint32))


def test_octahedron_normals_are_the_vertex_positions():
    v, f = sm.OCTAHEDRON
    n = sm.vertex_normals(v, f)
    assert np.array_equal(n.view(np.uint32), v.view(np.uint32))
    # vertex 0 = (1, 0, 0) by hand, the statements of g over its faces 0, 3, 4, 7 in that order
    topo = sm.topology(v, f)
    assert sm.incident(topo, 0) == [0, 3, 4, 7]
    N = [D(0.0), D(0.0), D(0.0)]
    for t in (0, 3, 4, 7):
        p0, p1, p2 = (v[k].astype(D) for k in f[t])
        u, w = p1 - p0, p2 - p0
        nx = u[1] * w[2] - u[2] * w[1]
        ny = u[2] * w[0] - u[0] * w[2]
        nz = u[0] * w[1] - u[1] * w[0]
        N = [N[0] + nx, N[1] + ny, N[2] + nz]
    l = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2])
    assert (N[0], N[1], N[2], l) == (4.0, 0.0, 0.0, 4.0)
    assert [F(N[a] / l) for a in range(3)] == n[0].tolist() == [1.0, 0.0, 0.0]
    # a vertex without faces, and a face of no area
    assert sm.vertex_normals(*sm.with_isolated(sm.OCTAHEDRON))[-1].tolist() == [0.0, 0.0, 0.0]
    assert not sm.vertex_normals(*sm.DEGENERATE).any()


# ---- the C ABI without a device ------------------------------------------------------------------------------------------
def test_abi_is_still_18_and_the_new_names_are_declared():
    from binocular3dgs_amd import _C, _lib
    header = open(os.path.join(ROOT, "include", "b3gs_raster.h")).read()
    assert _lib.ABI_VERSION == 18 and _lib.lib().b3gs_abi_version() == 18 and "#define B3GS_ABI_VERSION 18" in header
    for name in NEW:
        assert name in _lib.EXPORTS and name + "(" in header, name
    assert (_C.MESH_SHADE_SMOOTH, _C.MESH_SHADE_LIT) == (2, 3)
    assert "#define B3GS_MESH_SHADE_SMOOTH 2" in header and "#define B3GS_MESH_SHADE_LIT 3" in header


def test_entry_points_check_their_arguments_before_the_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    wb = L.b3gs_mesh_adjacency_workspace_bytes
    big = (2 ** 31 - 1) // 6
    assert wb(-1, 0) == 0 and wb(0, -1) == 0 and wb(2 ** 31, 0) == 0 and wb(10, big + 1) == 0 and wb(10, big) > 0
    prev = 0
    for V, nf in ((0, 0), (1, 0), (1, 1), (100, 200), (100, 201), (101, 201), (10 ** 6, 2 * 10 ** 6)):
        b = wb(V, nf)
        assert b % 256 == 0 and b >= prev and b > 0
        prev = b
    off = (C.c_size_t * 5)()
    assert L.b3gs_mesh_adjacency_layout(100, 200, off) == 0 and all(o % 256 == 0 and 0 < o < wb(100, 200) for o in off)
    assert L.b3gs_mesh_adjacency_layout(100, 200, None) == -1 and L.b3gs_mesh_adjacency_layout(-1, 0, off) == -1
    ws = 256 * 4                                                      # an aligned address that is never read: the checks come first
    assert L.b3gs_mesh_adjacency_build(3, 1, None, None, ws, None) == -1 and b"NULL" in L.b3gs_last_error()
    assert L.b3gs_mesh_adjacency_build(3, 1, None, None, None, None) == -1 and b"aligned" in L.b3gs_last_error()
    assert L.b3gs_mesh_adjacency_build(-1, 0, None, None, ws, None) == -1
    assert L.b3gs_mesh_adjacency_build(3, big + 1, None, None, ws, None) == -1 and b"6 F" in L.b3gs_last_error()
    assert L.b3gs_mesh_smooth(3, 1, None, ws, 1, 0.5, -0.53, 1, None, None) == -1 and b"NULL" in L.b3gs_last_error()
    assert L.b3gs_mesh_smooth(3, 1, None, ws + 8, 1, 0.5, -0.53, 1, None, None) == -1 and b"aligned" in L.b3gs_last_error()
    assert L.b3gs_mesh_smooth(3, 1, None, ws, -1, 0.5, -0.53, 1, None, None) == -1 and b"iterations" in L.b3gs_last_error()
    for lam, mu in ((0.0, -0.53), (1.5, -2.0), (float("nan"), -0.53), (0.5, 0.1), (0.5, -0.5), (0.5, -0.4), (0.5, float("nan")), (0.5, -float("inf"))):
        assert L.b3gs_mesh_smooth(3, 1, None, ws, 1, lam, mu, 1, None, None) == -1, (lam, mu)
    assert L.b3gs_mesh_vertex_normals(3, 1, None, None, ws, None, None) == -1 and b"NULL" in L.b3gs_last_error()
    assert L.b3gs_mesh_vertex_normals(3, -1, None, None, ws, None, None) == -1
    cams = (C.c_float * 14)()
    rs = L.b3gs_mesh_resolve_shaded_batch
    assert rs(1, None, 8, 8, 3, 1, None, None, ws, None, 2, None, None, None, None, None, None) == -1 and b"NULL" in L.b3gs_last_error()
    assert rs(0, cams, 8, 8, 0, 0, None, None, ws, None, 2, None, None, None, None, None, None) == -1 and b"views" in L.b3gs_last_error()
    assert rs(1, cams, 8, 8, 0, 0, None, None, ws, None, 1, None, None, None, None, None, None) == -1 and b"mode" in L.b3gs_last_error()
    assert rs(1, cams, 8, 8, 0, 0, None, None, None, None, 2, None, None, None, None, None, None) == -1 and b"aligned" in L.b3gs_last_error()
    assert rs(1, cams, 8, 0, 0, 0, None, None, ws, None, 3, None, None, None, None, None, None) == -1


# ---- the python surface --------------------------------------------------------------------------------------------------
def test_python_errors_without_a_device():
    import torch
    from binocular3dgs_amd import _lib, mesh_render, mesh_tools
    v, f = torch.from_numpy(sm.TETRAHEDRON[0]), torch.from_numpy(sm.TETRAHEDRON[1])
    for kw in ({"iterations": -1}, {"lam": 0.0}, {"lam": 1.5}, {"mu": 0.1}, {"mu": -0.5}, {"mu": -0.2}, {"lam": 0.6, "mu": -0.53}):
        with pytest.raises(ValueError, match="smooth:"):
            mesh_tools.smooth(v, f, **kw)
    with pytest.raises(ValueError, match="int32"):
        mesh_tools.smooth(v, f.long())
    with pytest.raises(ValueError, match="float32"):
        mesh_tools.vertex_normals(v.double(), f)
    for call in (lambda: mesh_tools.adjacency(v, f), lambda: mesh_tools.smooth(v, f), lambda: mesh_tools.smooth(v, f, mu=0.0),
                 lambda: mesh_tools.vertex_normals(v, f), lambda: mesh_tools.topology(v, f)):
        with pytest.raises(_lib.B3gsError, match="HIP device only"):
            call()
    assert mesh_render.SHADINGS == {"colour": 0, "normal": 1} and mesh_render.SHADED == {"smooth": 2, "lit": 3}
    cam = np.zeros((1, 14), F)
    with pytest.raises(ValueError, match="mode is one of"):
        mesh_render.render_mesh_shaded(v, v, f, cam, mode="normal", size=(8, 8))
    with pytest.raises(ValueError, match="normals are float32"):
        mesh_render.render_mesh_shaded(v, v[:3], f, cam, size=(8, 8))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mesh_render.render_mesh_shaded(v, v, f, cam, mode="lit", size=(8, 8))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        next(mesh_render.batches_shaded(v, v, f, cam, size=(8, 8)))
    line = mesh_tools.topology_line({"vertices": 4, "triangles": 4, "euler": 2, "closed": True, **dict(zip(mesh_tools.TOTALS, sm.topology(*sm.TETRAHEDRON)["totals"]))})
    assert line == "topology: 4 vertices (0 isolated), 6 edges (0 boundary, 0 non-manifold), 4 triangles, euler 2, closed"
    assert mesh_tools.TOTALS == sm.TOTALS


def test_parser_errors(capsys):
    from binocular3dgs_amd import extract_mesh, spiral
    for extra in (["--smooth_lambda", "0.4"], ["--smooth_mu", "-0.6"], ["--free_boundary"], ["--smooth", "0"], ["--smooth", "2", "--smooth_lambda", "0"],
                  ["--smooth", "2", "--smooth_mu", "-0.3"], ["--smooth", "2", "--smooth_mu", "0.2"]):
        with pytest.raises(SystemExit):
            extract_mesh.main(["-m", "nowhere"] + extra)
    assert "need --smooth" in capsys.readouterr().err
    a = extract_mesh.parser().parse_args(["-m", "x", "--smooth", "3", "--smooth_mu", "0", "--free_boundary", "--normals"])
    assert (a.smooth, a.smooth_lambda, a.smooth_mu, a.free_boundary, a.normals) == (3, None, 0.0, True, True)
    with pytest.raises(SystemExit):
        spiral.main(["-m", "nowhere", "--mesh", "m.ply", "--shading", "clay"])
    with pytest.raises(ValueError, match="texture goes with"):
        spiral.main(["-m", "nowhere", "--mesh", "m.obj", "--shading", "lit"])


# ---- PLY -----------------------------------------------------------------------------------------------------------------
def _parent_write_mesh_ply(path, v, c, f):
    """the bytes the four-argument write_mesh_ply has always written, assembled independently"""
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as fp:
        fp.write(header.encode("ascii"))
        for p, q in zip(v, c):
            fp.write(np.asarray(p, "<f4").tobytes() + np.asarray(q, "u1").tobytes())
        for t in f:
            fp.write(b"\x03" + np.asarray(t, "<i4").tobytes())


def test_ply_with_and_without_normals(tmp_path):
    from binocular3dgs_amd import mesh
    v, f = sm.icosphere(1, noise=0.05, seed=1)
    c = np.random.default_rng(0).integers(0, 256, size=v.shape).astype(np.uint8)
    n = sm.vertex_normals(v, f)
    plain, parent, normal = (str(tmp_path / name) for name in ("plain.ply", "parent.ply", "normal.ply"))
    mesh.write_mesh_ply(plain, v, c, f)
    _parent_write_mesh_ply(parent, v, c, f)
    assert open(plain, "rb").read() == open(parent, "rb").read()
    mesh.write_mesh_ply(plain, v, c, f, normals=None)
    assert open(plain, "rb").read() == open(parent, "rb").read()
    mesh.write_mesh_ply(normal, v, c, f, n)
    head = open(normal, "rb").read().split(b"end_header\n")[0].decode("ascii")
    assert "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar red" in head
    assert os.path.getsize(normal) == os.path.getsize(plain) + 12 * len(v) + len("property float nx\n") * 3
    rv, rc, rf, rn = mesh.read_mesh_ply(normal, return_normals=True)
    assert all(np.array_equal(a, b) for a, b in ((rv.view(np.uint32), v.view(np.uint32)), (rc, c), (rf, f), (rn.view(np.uint32), n.view(np.uint32))))
    three = mesh.read_mesh_ply(normal)
    assert len(three) == 3 and np.array_equal(three[0], v) and np.array_equal(three[1], c) and np.array_equal(three[2], f)
    four = mesh.read_mesh_ply(plain, return_normals=True)
    assert len(four) == 4 and four[3] is None and np.array_equal(four[0], v)
    assert len(mesh.read_mesh_ply(plain)) == 3
    with pytest.raises(ValueError, match="one normal per vertex"):
        mesh.write_mesh_ply(normal, v, c, f, n[:-1])
