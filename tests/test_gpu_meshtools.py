"""Cleaning and scoring an extracted mesh on the device (csrc/meshtools.hip, binocular3dgs_amd/mesh_tools.py) against the numpy
restatement of tests/meshtools_ref.py.  Components, compaction and the lattice membership are integer work, a nearest
distance is a minimum over a set, and every float statement is one correctly rounded float32 operation on both sides:
everything is compared bit for bit.  Only the fp64 means are sums; their bound is that of any summation order."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402
import meshtools_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- components and clean ----------------------------------------------------------------------------------------------
def _torus(n, m):
    """A closed n x m quad grid cut into 2 n m triangles over n m vertices."""
    idx = lambda i, j: (i % n) * m + j % m                                          # noqa: E731
    return [t for i in range(n) for j in range(m)
            for t in ((idx(i, j), idx(i + 1, j), idx(i, j + 1)), (idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)))]


def _debris_mesh():
    """Before the permutation: a strip of 2 500 triangles; two closed blobs of 2 000 triangles each (the tie); two strips of
    100 triangles that share one vertex (one component of 200); one triangle with a repeated index; 399 single triangles;
    37 vertices no triangle names.  -> (vertices, colours, faces), vertex ids randomly permuted."""
    faces, base = [], 0
    faces += [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(2500)]
    base += 2502
    for _ in range(2):
        faces += [tuple(base + q for q in t) for t in _torus(40, 25)]
        base += 1000
    faces += [(base + k, base + k + 1, base + k + 2) for k in range(100)]
    joint = base + 101                                                               # the last vertex of the first strip ...
    base += 102
    second = [joint] + [base + k for k in range(101)]                                # ... is the first of the second
    faces += [(second[k], second[k + 1], second[k + 2]) for k in range(100)]
    base += 101
    faces.append((base, base, base + 1))
    base += 2
    faces += [(base + 3 * k, base + 3 * k + 1, base + 3 * k + 2) for k in range(399)]
    base += 3 * 399
    V = base + 37
    rng = np.random.default_rng(11)
    perm = rng.permutation(V)
    faces = perm[np.array(faces, dtype=np.int64)].astype(np.int32)
    faces = faces[rng.permutation(len(faces))]
    vertices = rng.normal(size=(V, 3)).astype(F)
    colours = rng.integers(0, 256, size=(V, 3), dtype=np.uint8)
    return vertices, colours, faces


@pytest.fixture(scope="module")
def debris():
    v, c, f = _debris_mesh()
    assert len(v) % 64 and len(f) % 64 and 5900 < len(v) < 6100
    labels, count = tr.components(len(v), f)
    sizes = sorted(count[count > 0].tolist(), reverse=True)
    assert sizes[:4] == [2500, 2000, 2000, 200] and sizes[4] == 1 and len(sizes) == 4 + 1 + 399
    assert (count[labels] == 0).sum() == 37
    return {"v": v, "c": c, "f": f, "labels": labels, "count": count, "dev": (_dev(v), _dev(c), _dev(f))}


def test_components_match_the_yardstick(debris):
    from binocular3dgs_amd import mesh_tools
    dv, _, df = debris["dev"]
    labels, count = mesh_tools.components(dv, df)
    assert labels.dtype == torch.int32 and count.dtype == torch.int32 and labels.is_cuda
    assert np.array_equal(labels.cpu().numpy(), debris["labels"])
    assert np.array_equal(count.cpu().numpy(), debris["count"])
    again = mesh_tools.components(len(debris["v"]), df)                               # V itself; the same bits twice
    assert torch.equal(again[0], labels) and torch.equal(again[1], count)
    # another order of the triangles: the same labels and counts
    order = np.random.default_rng(12).permutation(len(debris["f"]))
    other = mesh_tools.components(dv, _dev(debris["f"][order]))
    assert torch.equal(other[0], labels) and torch.equal(other[1], count)


def test_components_of_nothing():
    from binocular3dgs_amd import mesh_tools
    labels, count = mesh_tools.components(5, torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert labels.tolist() == [0, 1, 2, 3, 4] and count.tolist() == [0] * 5
    labels, count = mesh_tools.components(0, torch.zeros((0, 3), dtype=torch.int32, device=DEV))
    assert labels.shape == (0,) and count.shape == (0,)


@pytest.mark.parametrize("keep_largest,min_triangles,triangles", [(0, 0, 7100), (1, 0, 2500), (2, 0, 6500), (0, 100, 6700)])
def test_clean_matches_the_yardstick(debris, keep_largest, min_triangles, triangles):
    from binocular3dgs_amd import mesh_tools
    want = tr.clean(debris["v"], debris["c"], debris["f"], keep_largest, min_triangles)
    assert len(want[2]) == triangles
    got = mesh_tools.clean(*debris["dev"], keep_largest, min_triangles)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape and np.array_equal(_bits(g), _bits(w))
    # order and winding: the kept triangles name the same positions, corner by corner, in the input's order
    kept = debris["count"][debris["labels"][debris["f"][:, 0]]] >= tr.threshold(debris["count"], keep_largest, min_triangles)
    assert np.array_equal(_bits(got[0].cpu().numpy()[got[2].cpu().numpy()]), _bits(debris["v"][debris["f"][kept]]))
    again = mesh_tools.clean(*debris["dev"], keep_largest, min_triangles)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    if (keep_largest, min_triangles) == (0, 0):
        assert got[0].shape[0] == len(debris["v"]) - 37


def test_clean_that_keeps_nothing_returns_empty_tensors(debris):
    from binocular3dgs_amd import mesh_tools
    v, c, f = mesh_tools.clean(*debris["dev"], 0, 10 ** 6)
    assert tuple(v.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32 and v.is_cuda
    v, c, f, st = mesh_tools.clean(*debris["dev"], 2, 0, return_stats=True)
    assert st == {"components": 404, "kept": 3, "vertices_dropped": len(debris["v"]) - 4502, "triangles_dropped": 600}


def _graph_replay(fn, outputs):
    """Captures fn() (which promises no host read) after a warm-up on a side stream, clears `outputs(result)`, replays once."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = fn()
    for t in outputs(result):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    return result


def test_components_and_threshold_replay_from_a_graph(debris):
    from binocular3dgs_amd import mesh_tools
    dv, _, df = debris["dev"]

    def fn():
        labels, count = mesh_tools.components(dv, df)
        return labels, count, mesh_tools.component_threshold(count, 2, 0)

    labels, count, thr = _graph_replay(fn, lambda r: r)
    assert np.array_equal(labels.cpu().numpy(), debris["labels"]) and np.array_equal(count.cpu().numpy(), debris["count"])
    assert thr.tolist() == [2000]


# ---- points on the surface ---------------------------------------------------------------------------------------------
SPACING = 0.125


def _mixed_triangles():
    rng = np.random.default_rng(21)
    v = rng.uniform(-1.0, 1.0, size=(120, 3)).astype(F)
    f = rng.integers(0, 120, size=(290, 3)).astype(np.int32)                         # edges from 0 (a repeated index) to ~3
    extra_v = np.array([[0, 0, 0], [0.05, 0, 0], [0, 0.04, 0.03],                    # shorter than the spacing: vertices only
                        [2, 2, 2], [2.5, 2.5, 2.5], [3, 3, 3],                       # zero area
                        [1, 0, 0], [1 + 4 * SPACING, 0, 0], [1, 0.3, 0],             # |e1| = 4 spacings exactly
                        [5, 5, 5], [5, 5, 5], [5, 5, 5]], dtype=F)                   # three equal points
    extra_f = np.arange(120, 132, dtype=np.int32).reshape(4, 3)
    tiny = np.stack([v[:6] + F(0.01), v[:6] + F(0.02), v[:6] + F(0.03)], axis=1).reshape(18, 3)
    tiny_f = np.arange(132, 150, dtype=np.int32).reshape(6, 3)
    return np.concatenate([v, extra_v, tiny]), np.concatenate([f, extra_f, tiny_f])


def test_sample_surface_matches_the_yardstick():
    from binocular3dgs_amd import mesh_tools
    v, f = _mixed_triangles()
    assert len(f) == 300
    want = tr.sample_surface(v, f, SPACING)
    per = [len(tr.lattice(v[t[0]], v[t[1]], v[t[2]], SPACING)) for t in f]
    assert per[291] > 0 and per[290] == 0 and per[293] == 0 and min(per[294:]) == 0 and max(per) > 100
    assert per[292] == len([1 for i in range(5) for j in range(3) if (i or j) and 3 * i + 5 * j < 15])     # n1 = 4, n2 = 2
    got = mesh_tools.sample_surface(_dev(v), _dev(f), SPACING)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(_bits(got), _bits(want))
    assert torch.equal(got, mesh_tools.sample_surface(_dev(v), _dev(f), SPACING))
    # no triangles: the vertices
    none = mesh_tools.sample_surface(_dev(v), torch.zeros((0, 3), dtype=torch.int32, device=DEV), SPACING)
    assert np.array_equal(_bits(none), _bits(v))


def test_sample_surface_errors():
    from binocular3dgs_amd import mesh_tools
    v = _dev(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F))
    f = _dev(np.array([[0, 1, 2]] * 8, np.int32))
    with pytest.raises(ValueError, match="spacing"):
        mesh_tools.sample_surface(v, f, 0.0)
    with pytest.raises(ValueError, match="spacing"):
        mesh_tools.sample_surface(v, f, -1.0)
    with pytest.raises(ValueError, match="32768 spacings"):                          # n = 100 000: seen by the count kernel
        mesh_tools.sample_surface(v, f, 1e-5)
    with pytest.raises(ValueError, match="do not fit int32"):                        # 8 x ~4.5e8 points: counted, never emitted
        mesh_tools.sample_surface(v, f, 1.0 / 30000.0)
    with pytest.raises(ValueError, match="outside 0"):
        mesh_tools.sample_surface(v, _dev(np.array([[0, 1, 3]], np.int32)), 0.5)


# ---- nearest distances -------------------------------------------------------------------------------------------------
MAX_DIST = 0.25


def _clouds(cell=None):
    """b: 7 001 points in [-1, 1]^3 with the two corners of the box among them, 50 exact duplicates and -- once the cell edge
    is known -- 200 points snapped onto multiples of it.  a: 5 003 queries: uniform ones, 300 outside b's box, 100 farther
    than max_dist from everything, 100 equal to a point of b and 100 snapped onto multiples of the cell edge."""
    rng = np.random.default_rng(31)
    b = rng.uniform(-1.0, 1.0, size=(7001, 3)).astype(F)
    b[0], b[1] = -1.0, 1.0
    b[100:150] = b[200:250]
    a = rng.uniform(-1.0, 1.0, size=(5003, 3)).astype(F)
    a[:300] = (rng.uniform(1.0, 1.3, size=(300, 3)) * rng.choice([-1.0, 1.0], size=(300, 3))).astype(F)
    a[300:400] = rng.uniform(3.0, 50.0, size=(100, 3)).astype(F)
    a[400:500] = b[1000:1100]
    if cell is not None:
        b[2000:2200] = (np.round(b[2000:2200] / F(cell)) * F(cell)).astype(F)
        a[500:600] = (np.round(a[500:600] / F(cell)) * F(cell)).astype(F)
    return a, b


def test_nearest_distances_match_the_brute_force():
    from binocular3dgs_amd import mesh_tools
    _, b0 = _clouds()
    p0 = mesh_tools.NearestGrid(_dev(b0), MAX_DIST).params()
    a, b = _clouds(p0["cell"])
    grid = mesh_tools.NearestGrid(_dev(b), MAX_DIST)
    p = grid.params()
    assert p["cell"] == p0["cell"] and p["origin"] == p0["origin"] and p["dims"] == p0["dims"]     # the box did not move
    assert min(p["dims"]) > 8 and p["dims"][0] * p["dims"][1] * p["dims"][2] <= 8 * 7001 and 2 <= p["shells"] <= 17
    want = tr.nearest_distances(a, b, MAX_DIST)
    assert (want[300:400] == F(MAX_DIST)).all() and (want[400:500] == 0).all()
    assert 0 < (want[:300] < F(MAX_DIST)).sum() < 300 and (want < F(MAX_DIST)).sum() > 4000
    got = grid.query(_dev(a))
    assert got.dtype == torch.float32 and tuple(got.shape) == (5003,)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{diff.sum()} of 5003 differ, first at {np.flatnonzero(diff)[:5]}"
    assert torch.equal(mesh_tools.nearest_distances(_dev(a), _dev(b), MAX_DIST), got)
    # the other way round, and a cap so large that every shell is needed
    assert np.array_equal(_bits(mesh_tools.nearest_distances(_dev(b), _dev(a), MAX_DIST)), _bits(tr.nearest_distances(b, a, MAX_DIST)))
    assert np.array_equal(_bits(mesh_tools.nearest_distances(_dev(a[:700]), _dev(b), 100.0)), _bits(tr.nearest_distances(a[:700], b, 100.0)))


def test_nearest_distances_when_the_cloud_is_one_cell_or_one_point():
    from binocular3dgs_amd import mesh_tools
    rng = np.random.default_rng(32)
    b = rng.uniform(0.52, 0.53, size=(500, 3)).astype(F)
    a = rng.uniform(-0.6, 1.6, size=(1003, 3)).astype(F)
    a[:50] = b[:50]
    grid = mesh_tools.NearestGrid(_dev(b), 1.0)
    assert grid.params()["dims"] == [1, 1, 1]
    want = tr.nearest_distances(a, b, 1.0)
    assert (want[:50] == 0).all() and (want == F(1.0)).any() and (want < F(1.0)).sum() > 300
    assert np.array_equal(_bits(grid.query(_dev(a))), _bits(want))
    one = b[:1]
    assert np.array_equal(_bits(mesh_tools.nearest_distances(_dev(a), _dev(one), 0.7)), _bits(tr.nearest_distances(a, one, 0.7)))
    assert mesh_tools.nearest_distances(torch.zeros((0, 3), device=DEV), _dev(b), 1.0).shape == (0,)
    with pytest.raises(ValueError, match="empty"):
        mesh_tools.nearest_distances(_dev(a), torch.zeros((0, 3), device=DEV), 1.0)
    with pytest.raises(ValueError, match="max_dist"):
        mesh_tools.nearest_distances(_dev(a), _dev(b), 0.0)


# ---- the score ---------------------------------------------------------------------------------------------------------
def _sphere_mesh():
    from binocular3dgs_amd.mesh import TsdfVolume
    ref = mr.sphere_volume()
    nz, ny, nx = ref["tsdf"].shape
    vol = TsdfVolume(ref["origin"], [o + d * ref["voxel"] for o, d in zip(ref["origin"], (nx, ny, nz))], ref["voxel"], 4.0, device=DEV)
    vol.tsdf.copy_(torch.from_numpy(ref["tsdf"]))
    vol.weight.copy_(torch.from_numpy(ref["weight"]))
    vol.rgb.copy_(torch.from_numpy(ref["rgb"]))
    return vol.extract()


def _assert_score(got, want, n_recon, n_gt):
    for key in ("n_recon", "n_gt", "n_recon_below_tau", "n_gt_below_tau", "precision", "recall", "fscore"):
        assert got[key] == want[key], key
    for key, n in (("accuracy", n_recon), ("completeness", n_gt)):
        assert abs(got[key] - want[key]) <= n * 2.0 ** -52 * want[key], key            # any order of n non-negative terms
    assert abs(got["chamfer"] - want["chamfer"]) <= (n_recon + n_gt) * 2.0 ** -52 * want["chamfer"]


def test_score_of_a_sphere_mesh():
    from binocular3dgs_amd import mesh_tools
    vertices, _, faces = _sphere_mesh()
    rng = np.random.default_rng(41)
    d = rng.normal(size=(4001, 3))
    gt = (np.array([10.0, 9.0, 8.0]) + 6.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    gt[:40] += F(3.0)                                                                # reference points the mesh does not reach
    spacing, max_dist, tau = 0.4, 2.0, 0.15
    recon = tr.sample_surface(vertices.cpu().numpy(), faces.cpu().numpy(), spacing)
    d_recon, d_gt = tr.nearest_distances(recon, gt, max_dist), tr.nearest_distances(gt, recon, max_dist)
    got = mesh_tools.score_mesh(vertices, faces, _dev(gt), spacing, max_dist, tau, return_distances=True)
    assert np.array_equal(_bits(got["d_recon"]), _bits(d_recon)) and np.array_equal(_bits(got["d_gt"]), _bits(d_gt))
    want = tr.score(d_recon, d_gt, tau)
    assert 0 < want["precision"] < 1 and 0 < want["recall"] < 1 and want["n_recon"] == len(recon) > len(vertices)
    _assert_score(got, want, len(recon), len(gt))
    # masks drop points from the means, not from the clouds searched
    mask_recon, mask_gt = rng.uniform(size=len(recon)) < 0.7, np.arange(len(gt)) >= 40
    got = mesh_tools.score_clouds(_dev(recon), _dev(gt), max_dist, tau, _dev(mask_recon), _dev(mask_gt), return_distances=True)
    assert np.array_equal(_bits(got["d_recon"]), _bits(d_recon)) and np.array_equal(_bits(got["d_gt"]), _bits(d_gt))
    want = tr.score(d_recon, d_gt, tau, mask_recon, mask_gt)
    assert want["n_recon"] == int(mask_recon.sum()) and want["n_gt"] == len(gt) - 40
    _assert_score(got, want, want["n_recon"], want["n_gt"])
    again = mesh_tools.score_clouds(_dev(recon), _dev(gt), max_dist, tau, _dev(mask_recon), _dev(mask_gt))
    assert all(again[k] == got[k] for k in again)
    with pytest.raises(ValueError, match="leaves no point"):
        mesh_tools.score_clouds(_dev(recon), _dev(gt), max_dist, tau, None, _dev(np.zeros(len(gt), bool)))


def test_distances_and_sums_replay_from_a_graph():
    from binocular3dgs_amd import _C, mesh_tools
    a, b = _clouds()
    da, db = _dev(a[:1501]), _dev(b)
    sums = torch.empty(3, dtype=torch.float64, device=DEV)

    def fn():
        d = mesh_tools.nearest_distances(da, db, MAX_DIST)
        _C.cloud_score(d, None, 0.05, sums)
        return d

    d = _graph_replay(fn, lambda r: (r, sums))
    want = tr.nearest_distances(a[:1501], b, MAX_DIST)
    assert np.array_equal(_bits(d), _bits(want))
    total, n, below = sums.tolist()
    assert n == 1501 and below == int((want < F(0.05)).sum())
    assert abs(total - want.astype(np.float64).sum()) <= 1501 * 2.0 ** -52 * want.astype(np.float64).sum()


# ---- command line ------------------------------------------------------------------------------------------------------
def _shell_model(tmp_path, P=400):
    """Gaussians on a sphere shell of radius 1 around (0, 0, 6), saved as a trained model folder with 6 cameras around it
    (cameras.json); -> (model path, model, cameras), both read back from the folder."""
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


def test_the_command_lines(tmp_path, capsys):
    from binocular3dgs_amd import eval_mesh, extract_mesh, mesh, mesh_tools
    from binocular3dgs_amd.matcher_cloud import write_cloud_ply
    path, model, cams = _shell_model(tmp_path)
    out = os.path.join(path, "mesh", "iteration_7", "mesh.ply")
    v, c, f = mesh.fuse_model(model, cams, torch.zeros(3, device=DEV), resolution=24)
    plain = str(tmp_path / "plain.ply")
    mesh.write_mesh_ply(plain, v, c, f)
    # without the new flags (and with both at 0) the file is what the extraction alone writes, byte for byte
    for extra in ([], ["--keep_largest", "0", "--min_triangles", "0"]):
        assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24"] + extra) == 0
        assert "components" not in capsys.readouterr().out
        assert open(out, "rb").read() == open(plain, "rb").read()
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24", "--keep_largest", "1"]) == 0
    text = capsys.readouterr().out
    want = mesh_tools.clean(v, c, f, 1, 0, return_stats=True)
    st = want[3]
    assert f"{st['components']} components, {st['kept']} kept: dropped {st['vertices_dropped']} vertices, {st['triangles_dropped']} triangles" in text
    pv, pc, pf = mesh.read_mesh_ply(out)
    assert np.array_equal(_bits(pv), _bits(want[0])) and np.array_equal(pc, want[1].cpu().numpy()) and np.array_equal(pf, want[2].cpu().numpy())
    labels, count = tr.components(len(pv), pf)
    assert (count > 0).sum() == 1 and (labels == 0).all()
    # the score of that file against points on the shell
    d = np.random.default_rng(5).normal(size=(3000, 3))
    gt = (np.array([0.0, 0.0, 6.0]) + d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    cloud = str(tmp_path / "gt.ply")
    write_cloud_ply(cloud, gt, np.zeros((3000, 3), np.uint8))
    assert eval_mesh.main(["--mesh", out, "--gt", cloud, "--spacing", "0.05", "--max_dist", "0.5", "--tau", "0.1"]) == 0
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    stored = json.load(open(os.path.join(path, "mesh", "iteration_7", "mesh_results.json")))
    assert printed == stored and stored["triangles"] == len(pf)
    recon = tr.sample_surface(pv, pf, 0.05)
    want = tr.score(tr.nearest_distances(recon, gt, 0.5), tr.nearest_distances(gt, recon, 0.5), 0.1)
    _assert_score(stored, want, len(recon), len(gt))
    assert stored["n_recon"] == len(recon)
