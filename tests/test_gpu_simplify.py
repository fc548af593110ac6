"""Vertex clustering on the device (csrc/simplify.hip, mesh_tools.simplify / simplify_to) against the numpy restatement of
tests/simplify_ref.py.  Clusters, surviving faces, colours, counts and statistics are integer work; the positions are fp64
statements in one fixed order, rounded once to float32: everything is compared bit for bit, for both placements."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
PLACEMENTS = ("quadric", "mean")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _check(v, c, f, cell, placements=PLACEMENTS):
    """simplify on the device == the restatement, bit for bit, statistics included -> the device outputs per placement"""
    from binocular3dgs_amd import mesh_tools
    dv, dc, df = _dev(v), _dev(c), _dev(f)
    out = {}
    for placement in placements:
        want = sr.simplify(v, c, f, cell, placement)
        got = mesh_tools.simplify(dv, dc, df, cell, placement, return_stats=True)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32 and got[0].is_cuda
        assert got[3] == sr.stats(want[3]), placement
        for name, g, w in zip(("vertices", "colours", "faces"), got[:3], want[:3]):
            assert tuple(g.shape) == w.shape, (placement, name)
            assert np.array_equal(_bits(g), _bits(w)), (placement, name)
        out[placement] = got
    return out


@pytest.fixture(scope="module")
def sphere():
    v, c, f = sr.sphere_mesh()
    return v, c, f


@pytest.mark.parametrize("cell", [1.5, 2.5, 6.0])
def test_sphere_matches_the_restatement(sphere, cell):
    out = _check(*sphere, cell)
    assert 0 < out["quadric"][2].shape[0] < sphere[2].shape[0]


def test_two_calls_give_identical_bits(sphere):
    from binocular3dgs_amd import mesh_tools
    d = [_dev(a) for a in sphere]
    for placement in PLACEMENTS:
        a = mesh_tools.simplify(*d, 2.5, placement)
        b = mesh_tools.simplify(*d, 2.5, placement)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def _soup(V, nf, seed):
    """V random vertices in a 6 x 6 x 6 box and nf random faces over them"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 6, size=(V, 3)).astype(F)
    c = rng.integers(0, 256, size=(V, 3), dtype=np.uint8)
    f = rng.integers(0, V, size=(nf, 3)).astype(np.int32)
    return v, c, f


@pytest.mark.parametrize("V", [63, 64, 65])
@pytest.mark.parametrize("nf", [255, 256, 257])
def test_wave_and_block_edges(V, nf):
    _check(*_soup(V, nf, 100 * V + nf), 1.0)


@pytest.mark.parametrize("n,what", [(401, "faces"), (520, "vertices")])
def test_scan_seams_at_2_to_the_18(n, what):
    v, c, f = sr.grid_mesh(n, n)
    assert (len(f), len(v))[what == "vertices"] == {401: 320000, 520: 270400}[n] > 2 ** 18
    _check(v, c, f, 3.5)


def test_vertices_exactly_on_cell_faces():
    rng = np.random.default_rng(7)
    v = (rng.integers(0, 41, size=(500, 3)) * 0.25).astype(F)
    v[0] = 0.0                                                             # the origin is 0
    c = rng.integers(0, 256, size=(500, 3), dtype=np.uint8)
    f = rng.integers(0, 500, size=(1500, 3)).astype(np.int32)
    for cell in (0.25, 0.75, 1.25):
        _check(v, c, f, cell)


def test_identical_positions_and_unreferenced_vertices():
    rng = np.random.default_rng(8)
    base = rng.uniform(0, 8, size=(40, 3)).astype(F)
    v = np.concatenate([base, base, base[:10], np.array([[20.5, 20.5, 20.5], [20.6, 20.5, 20.5]], F)])   # a cluster nobody names
    c = rng.integers(0, 256, size=(len(v), 3), dtype=np.uint8)
    f = rng.integers(0, 90, size=(300, 3)).astype(np.int32)                # never 90, 91; some of 0 .. 89 stay unnamed too
    out = _check(v, c, f, 2.0)
    want = sr.simplify(v, c, f, 2.0)
    assert want[3]["clusters"] > len(want[0])                              # a cluster without a surviving face was dropped
    assert out["quadric"][3]["vertices_dropped"] == len(v) - len(want[0])


def test_a_face_with_two_corners_in_one_cluster_counts_once_in_the_quadric():
    # vertices 0 and 1 share a cell; face 0 names both (degenerate, dropped, but part of the cluster's quadric ONCE)
    v = np.array([[0.1, 0.1, 0.1], [0.6, 0.3, 0.2], [3.2, 0.4, 0.3], [0.3, 3.3, 0.9], [3.5, 3.1, 2.7], [0.2, 0.4, 3.6]], F)
    c = np.arange(18, dtype=np.uint8).reshape(6, 3)
    f = np.array([[0, 1, 2], [0, 2, 3], [1, 3, 4], [0, 0, 5], [1, 5, 3], [2, 4, 3]], np.int32)
    out = _check(v, c, f, 1.5)
    assert out["quadric"][3]["triangles_degenerate"] == 2
    # counting face 0 twice would move the representative: the restatement with the face doubled differs
    doubled = sr.simplify(v, c, np.concatenate([f[:1], f]), 1.5)
    assert not np.array_equal(_bits(doubled[0]), _bits(out["quadric"][0]))


def test_opposite_winding_duplicates_keep_the_first_listed():
    v, c, f = sr.grid_mesh(9, 9)
    back = f[:, [0, 2, 1]]
    for faces in (np.concatenate([f, back]), np.concatenate([back, f])):
        out = _check(v, c, faces, 2.0)
        kept = sr.simplify(v, c, faces, 2.0)[3]["kept_faces"]
        assert (kept < len(f)).all() and out["mean"][3]["triangles_duplicate"] > 0


def test_two_parallel_sheets_closer_than_a_cell():
    v0, c0, f0 = sr.grid_mesh(12, 12, z=0.0)
    v1, c1, f1 = sr.grid_mesh(12, 12, z=0.4)
    v, c, f = np.concatenate([v0, v1]), np.concatenate([c0, c1]), np.concatenate([f0, f1 + len(v0)])
    out = _check(v, c, f, 2.5)
    assert out["mean"][3]["triangles_duplicate"] > 0                        # the sheets merge


def test_everything_inside_one_cell_is_the_empty_mesh():
    from binocular3dgs_amd import mesh_tools
    v, c, f = sr.grid_mesh(5, 5)
    out = _check(v, c, f, 50.0)
    for p in PLACEMENTS:
        assert out[p][0].shape == (0, 3) and out[p][1].shape == (0, 3) and out[p][2].shape == (0, 3)
        assert out[p][3] == {"clusters": 1, "vertices_dropped": 25, "triangles_degenerate": 32, "triangles_duplicate": 0}
    e = mesh_tools.simplify(_dev(v), _dev(c), torch.zeros((0, 3), dtype=torch.int32, device=DEV), 1.0)     # no faces at all
    assert e[0].shape == (0, 3) and e[2].shape == (0, 3)


def test_errors_are_value_errors_and_the_device_stays_usable():
    from binocular3dgs_amd import mesh_tools
    v, c, f = sr.grid_mesh(6, 6)                                           # extent 5
    d = (_dev(v), _dev(c), _dev(f))
    with pytest.raises(ValueError, match="smallest admissible cell") as e:
        mesh_tools.simplify(*d, 5.0 / 1024.5)                              # 1025 cells along x and y
    named = float(str(e.value).rsplit(" ", 1)[1])
    assert named == mesh_tools.smallest_cell(5.0)
    ok = mesh_tools.simplify(*d, named)                                    # the named cell is admissible
    assert ok[2].shape[0] == len(f)
    with pytest.raises(ValueError, match="smallest admissible cell"):
        mesh_tools.simplify(*d, float(np.nextafter(F(named), F(0))))       # ... and the float32 below it is not
    nan = v.copy()
    nan[7, 2] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        mesh_tools.simplify(_dev(nan), d[1], d[2], 1.0)
    bad = f.copy()
    bad[11, 1] = len(v)
    with pytest.raises(ValueError, match="outside 0"):
        mesh_tools.simplify(d[0], d[1], _dev(bad), 1.0)
    torch.cuda.synchronize()
    _check(v, c, f, 2.0)


def test_simplify_to_meets_the_target_and_equals_simplify_at_its_cell(sphere):
    from binocular3dgs_amd import mesh_tools
    d = [_dev(a) for a in sphere]
    target = len(sphere[2]) // 4
    for placement in PLACEMENTS:
        ov, oc, of, cell = mesh_tools.simplify_to(*d, target, placement)
        assert 0 < of.shape[0] <= target
        same = mesh_tools.simplify(*d, cell, placement)
        assert torch.equal(ov, same[0]) and torch.equal(oc, same[1]) and torch.equal(of, same[2])
        extent = float((sphere[0].max(axis=0) - sphere[0].min(axis=0)).max())
        want_cell, want_n = mesh_tools.bisect_cell(lambda x: sr.count_triangles(sphere[0], sphere[2], F(x)), extent, target)
        assert cell == want_cell and of.shape[0] == want_n


def test_simplified_sphere_scores_within_the_cell_bound(sphere):
    from binocular3dgs_amd import mesh_tools
    d = [_dev(a) for a in sphere]
    cell = 2.5
    gt = mesh_tools.sample_surface(d[0], d[2], 0.5)
    for placement in PLACEMENTS:
        ov, _, of = mesh_tools.simplify(*d, cell, placement)
        score = mesh_tools.score_mesh(ov, of, gt, 0.5, 100.0, 1.0)
        assert score["accuracy"] <= 2.0 * math.sqrt(3.0) * cell
