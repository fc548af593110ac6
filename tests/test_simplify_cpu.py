"""CPU: the vertex-clustering rule of include/b3gs_raster.h in its numpy restatement (tests/simplify_ref.py), the host
logic of simplify_to, the command line, and the argument checks of the two entry points, which need no device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as sr  # noqa: E402

F = np.float32
ERR_ARG = -1
CENTRE, RADIUS, CELL = 12.0, 8.0, 2.5


def test_library_and_binding_list_the_entry_points():
    from binocular3dgs_amd import _C, _lib
    assert _lib.lib().b3gs_abi_version() == _lib.ABI_VERSION == _C.ABI_VERSION
    for name in ("b3gs_mesh_simplify_workspace_bytes", "b3gs_mesh_simplify_count", "b3gs_mesh_simplify_emit"):
        assert name in _lib.EXPORTS
    assert callable(_C.mesh_simplify_count) and callable(_C.mesh_simplify_emit)
    assert (_C.SIMPLIFY_QUADRIC, _C.SIMPLIFY_MEAN) == (0, 1)


def test_entry_points_refuse_bad_arguments_without_touching_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    nan = float("nan")
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 255) & ~255                                   # a host address: never dereferenced by a refused call
    count, emit = L.b3gs_mesh_simplify_count, L.b3gs_mesh_simplify_emit
    assert count(4, 2, None, p, 1.0, p, None) == ERR_ARG                  # NULL vertices
    assert count(4, 2, p, None, 1.0, p, None) == ERR_ARG                  # NULL faces
    assert count(4, 2, p, p, 1.0, None, None) == ERR_ARG                  # NULL workspace
    assert count(4, 2, p, p, 1.0, p + 8, None) == ERR_ARG                 # ... or one that is not 256-byte aligned
    assert count(4, 2, p, p, 0.0, p, None) == ERR_ARG and b"cell" in L.b3gs_last_error()
    assert count(4, 2, p, p, -1.0, p, None) == ERR_ARG
    assert count(4, 2, p, p, nan, p, None) == ERR_ARG
    assert count(4, 2, p, p, float("inf"), p, None) == ERR_ARG
    assert count(-1, 2, p, p, 1.0, p, None) == ERR_ARG
    assert count(4, -1, p, p, 1.0, p, None) == ERR_ARG
    assert count(4, 2 ** 31 // 3 + 1, p, p, 1.0, p, None) == ERR_ARG      # 3 F does not fit int32
    ok = (4, 2, p, p, p, 1.0, 0, p, 4, 2, p, p, p, None)

    def with_(**kw):
        names = ("V", "F", "vertices", "colours", "faces", "cell", "placement", "workspace", "nverts", "ntris", "out_vertices",
                 "out_colours", "out_faces", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for name in ("vertices", "colours", "faces", "workspace", "out_vertices", "out_colours", "out_faces"):
        assert emit(*with_(**{name: None})) == ERR_ARG, name
    for kw in ({"cell": 0.0}, {"cell": -2.0}, {"cell": nan}, {"V": -1}, {"F": -1}, {"placement": 2}, {"placement": -1},
               {"nverts": 5}, {"ntris": 3}, {"nverts": -1}, {"nverts": 2 ** 31}, {"ntris": 2 ** 31}):
        assert emit(*with_(**kw)) == ERR_ARG, kw
    assert emit(*with_(placement=7)) == ERR_ARG and b"placement" in L.b3gs_last_error()
    size = L.b3gs_mesh_simplify_workspace_bytes
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size(2 ** 31, 0) == 0 and size(0, 2 ** 31 // 3 + 1) == 0
    assert size(0, 0) % 256 == 0 and 0 < size(0, 0) < size(1000, 2000) < size(1000, 4000) and size(1000, 2000) % 256 == 0


def test_python_wrappers_refuse_bad_arguments_before_any_launch():
    import torch
    from binocular3dgs_amd import _lib, mesh_tools
    v, c, f = torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.uint8), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="placement"):
        mesh_tools.simplify(v, c, f, 1.0, placement="median")
    with pytest.raises(ValueError, match="cell"):
        mesh_tools.simplify(v, c, f, 0.0)
    with pytest.raises(ValueError, match="cell"):
        mesh_tools.simplify(v, c, f, float("nan"))
    with pytest.raises(ValueError, match="target_triangles"):
        mesh_tools.simplify_to(v, c, f, 0)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mesh_tools.simplify(v, c, f, 1.0)


# ---- the restatement on the sphere -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    v, c, f = sr.sphere_mesh()
    assert len(v) > 3000 and len(f) > 7000
    out = {p: sr.simplify(v, c, f, CELL, p) for p in ("quadric", "mean")}
    return {"v": v, "c": c, "f": f, "out": out}


@pytest.mark.parametrize("placement", ["quadric", "mean"])
def test_restatement_leaves_a_clean_mesh_within_the_cell_bounds(sphere, placement):
    v, f = sphere["v"], sphere["f"]
    ov, oc, of, info = sphere["out"][placement]
    assert 0 < len(of) < len(f) / 10 and ov.dtype == F and oc.dtype == np.uint8 and of.dtype == np.int32
    # no degenerate and no duplicate face survives
    assert (of[:, 0] != of[:, 1]).all() and (of[:, 1] != of[:, 2]).all() and (of[:, 0] != of[:, 2]).all()
    assert len(np.unique(np.sort(of, axis=1), axis=0)) == len(of)
    # every surviving vertex is named by a face, and ids are dense
    assert np.array_equal(np.unique(of), np.arange(len(ov)))
    assert info["triangles_degenerate"] + info["triangles_duplicate"] + len(of) == len(f)
    assert info["vertices_dropped"] == len(v) - len(ov) and info["clusters"] >= len(ov)
    # the mean lies in its cell's box (closed: the fp64 mean of float32 members of the float32 cell)
    m, cc, o = info["mean"], info["cluster_cell"], info["origin"].astype(np.float64)
    lo = o[None, :] + cc * CELL
    slack = 1e-5                                                           # cell membership is decided in float32
    assert (m >= lo - slack).all() and (m <= lo + CELL + slack).all()
    # the representative stays within one cell of the mean along every axis
    assert np.abs(ov.astype(np.float64) - m).max() <= CELL + 1e-6
    if placement == "mean":
        assert np.array_equal(ov, m.astype(F))
    # every point of a surviving triangle is within 2 sqrt(3) cell of the same point of its input triangle: corners suffice
    # (the difference is linear in the barycentric weights), checked at the corners and at random weights
    src = v[f[info["kept_faces"]].astype(np.int64)].astype(np.float64)
    dst = ov[of.astype(np.int64)].astype(np.float64)
    bound = 2.0 * math.sqrt(3.0) * CELL
    assert np.linalg.norm(src - dst, axis=2).max() <= bound
    w = np.random.default_rng(3).dirichlet((1.0, 1.0, 1.0), size=len(of))
    assert np.linalg.norm(np.einsum("fk,fkx->fx", w, src - dst), axis=1).max() <= bound
    # the corners map to their own clusters, with the input's corner order
    assert np.array_equal(of, info["cluster_of_vertex"][f[info["kept_faces"]].astype(np.int64)])


def test_both_placements_share_topology_and_colours(sphere):
    q, m = sphere["out"]["quadric"], sphere["out"]["mean"]
    assert np.array_equal(q[2], m[2]) and np.array_equal(q[1], m[1]) and sr.stats(q[3]) == sr.stats(m[3])
    assert not np.array_equal(q[0], m[0])


def test_colour_is_the_rounded_integer_mean():
    v = np.array([[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [5, 0, 0], [0, 5, 0]], F)
    c = np.array([[0, 1, 255], [1, 2, 255], [1, 2, 254], [9, 9, 9], [7, 7, 7]], np.uint8)
    f = np.array([[0, 3, 4], [1, 3, 4], [2, 4, 3]], np.int32)
    ov, oc, of, info = sr.simplify(v, c, f, 1.0)
    assert oc.tolist() == [[1, 2, 255], [9, 9, 9], [7, 7, 7]]           # 2/3 -> 1, 5/3 -> 2, 764/3 -> 255
    assert of.tolist() == [[0, 1, 2]] and info["triangles_duplicate"] == 2 and info["triangles_degenerate"] == 0


def test_quadric_is_nearer_to_the_analytic_sphere_than_the_mean(sphere):
    def err(p):
        r = np.linalg.norm(sphere["out"][p][0].astype(np.float64) - CENTRE, axis=1)
        return float(np.abs(r - RADIUS).mean())
    assert err("quadric") < err("mean")


def test_quadric_finds_the_ridge_of_a_roof_and_the_mean_does_not():
    """Two planes z = s x and z = s (12 - x) meet in the ridge x = 6, the middle of the cells 4 <= x < 8 (cell 4).  Slope s = 1,
    chosen with the restatement: the quadric representatives of the ridge clusters lie within 2.8e-3 of both planes (the
    bound is 1e-2 cell = 4e-2; the regulariser lambda keeps them off the ridge by that much), the means 1.06 away."""
    slope, cell = 1.0, 4.0
    v, c, f, ridge = sr.roof_mesh(slope, cell=cell)
    dist = {}
    for placement in ("quadric", "mean"):
        ov, _, _, info = sr.simplify(v, c, f, cell, placement)
        ids = np.unique(info["cluster_of_vertex"][v[:, 0] == F(ridge)])
        ids = ids[ids >= 0]
        assert len(ids) >= 4
        p = ov[ids].astype(np.float64)
        norm = math.sqrt(1.0 + slope * slope)
        d = np.maximum(np.abs(slope * p[:, 0] - p[:, 2]), np.abs(slope * (2 * ridge - p[:, 0]) - p[:, 2])) / norm
        dist[placement] = (float(d.min()), float(d.max()))
    # measured: quadric (0.00238, 0.00275), mean (1.0607, 1.0607)
    assert dist["quadric"][1] <= 1e-2 * cell
    assert dist["mean"][0] >= 10.0 * dist["quadric"][1] and dist["mean"][0] >= 10.0 * 1e-2 * cell


def test_errors_of_the_restatement_match_the_rule():
    v, c, f = sr.grid_mesh(3, 3)
    with pytest.raises(ValueError, match="1024"):
        sr.simplify(v, c, f, 2.0 / 1024.5)
    nan = v.copy()
    nan[4, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sr.simplify(nan, c, f, 1.0)
    bad = f.copy()
    bad[3, 2] = len(v)
    with pytest.raises(ValueError, match="index"):
        sr.simplify(v, c, bad, 1.0)
    ov, oc, of, info = sr.simplify(v, c, f, 100.0)                       # everything in one cell: the empty mesh, no error
    assert ov.shape == (0, 3) and oc.shape == (0, 3) and of.shape == (0, 3) and info["clusters"] == 1


# ---- simplify_to ---------------------------------------------------------------------------------------------------------
def test_smallest_cell_is_the_first_float32_that_fits_1024_cells():
    from binocular3dgs_amd import mesh_tools
    for extent in (1.0, 23.0, 0.3, 1000.0, 3.1415927):
        c = F(mesh_tools.smallest_cell(extent))
        assert float(c) == mesh_tools.smallest_cell(extent)
        assert np.floor(F(extent) / c) <= 1023
        assert np.floor(F(extent) / np.nextafter(c, F(0))) >= 1024


def test_bisection_returns_the_smallest_tried_cell_that_meets_the_target(sphere):
    from binocular3dgs_amd import mesh_tools
    v, f = sphere["v"], sphere["f"]
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    tried = []

    def count(cell):
        tried.append((cell, sr.count_triangles(v, f, F(cell))))
        return tried[-1][1]

    for target in (len(f) // 4, 100, 1, len(f)):
        tried.clear()
        cell, n = mesh_tools.bisect_cell(count, extent, target)
        assert 1 <= len(tried) <= mesh_tools.MAX_TRIALS == 12
        assert n <= target and (cell, n) in tried
        assert cell == min(c for c, k in tried if k <= target)
        assert all(extent / 1024 * 0.999 <= c <= extent for c, _ in tried)
    assert cell == tried[0][0] and len(tried) == 1                         # the whole mesh fits the last target: the lower end
    with pytest.raises(ValueError, match="whole extent"):
        mesh_tools.bisect_cell(lambda c: 5, extent, 4)


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_cli_takes_one_of_the_two_simplify_options():
    from binocular3dgs_amd.extract_mesh import parser
    p = parser()
    a = p.parse_args(["-m", "x"])
    assert a.simplify is None and a.target_triangles is None and a.placement == "quadric"
    a = p.parse_args(["-m", "x", "--simplify", "2.5", "--placement", "mean"])
    assert a.simplify == 2.5 and a.placement == "mean"
    assert p.parse_args(["-m", "x", "--target_triangles", "1000"]).target_triangles == 1000
    for bad in (["--simplify", "2", "--target_triangles", "10"], ["--simplify", "0"], ["--simplify", "-1"], ["--simplify", "nan"],
                ["--target_triangles", "0"], ["--placement", "median"]):
        with pytest.raises(SystemExit):
            p.parse_args(["-m", "x"] + bad)
