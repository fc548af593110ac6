"""The mesh smoothing stage on the device (csrc/meshsmooth.hip, binocular3dgs_amd/mesh_tools.py, mesh_render.py) against the numpy
restatement of tests/meshsmooth_ref.py: the neighbour lists, the incidence lists, the totals, the pinned mask, the filtered
positions, the vertex normals and the shaded render are compared bit for bit.  Meshes have a few to a few thousand vertices; the
three that cross the block span of the ordered scan have up to 131072 triangles and are checked once each."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402
import meshsmooth_ref as sm  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binocular3dgs_amd", "csrc")


def _constant(path, name):
    return int(re.search(name + r"\s*=?\s*(\d+)\s*;?", open(os.path.join(CSRC, path)).read()).group(1))


TPB = _constant("mesh_tri.h", r"constexpr int MESH_TPB")                    # the workgroup size of every kernel of meshsmooth.hip
SPAN = _constant("b3gs_internal.h", r"#define B3GS_SCAN_TPB") * TPB         # positions whose block sums one step of the ordered scan takes


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), f"{what}: {(_bits(a) != _bits(b)).sum()} words differ"


def _check_adjacency(adj, topo, V):
    from binocular3dgs_amd import mesh_tools
    assert adj.totals.tolist() == topo["totals"]
    lists = {k: t.cpu().numpy() for k, t in adj.lists().items()}
    _same(lists["neighbour_offsets"], topo["offsets"], "neighbour offsets")
    _same(lists["neighbour_indices"][:len(topo["indices"])], topo["indices"], "neighbour indices")
    _same(lists["pinned"], topo["pinned"], "pinned mask")
    rng, cnt = lists["incidence_ranges"].astype(np.int64), topo["inc_hi"] - topo["inc_lo"]
    assert np.array_equal(rng[:, 1] - rng[:, 0], cnt) and np.array_equal(rng[cnt > 0, 0], topo["inc_lo"][cnt > 0])
    _same(lists["incident_faces"][:len(topo["inc_faces"])], topo["inc_faces"], "incident faces")
    assert mesh_tools.TOTALS == sm.TOTALS


def _check_mesh(v, f, iterations=(0, 1, 2, 5), full=True):
    """everything of one valid mesh against the yardstick -> the holder"""
    from binocular3dgs_amd import mesh_tools
    topo = sm.topology(v, f)
    dv, df = _dev(v, F).reshape(-1, 3), _dev(f, np.int32).reshape(-1, 3)
    adj = mesh_tools.adjacency(dv, df)
    _check_adjacency(adj, topo, len(v))
    info = mesh_tools.topology(dv, df, adjacency=adj)
    assert [info[k] for k in sm.TOTALS] == topo["totals"] and info["euler"] == topo["euler"] and info["closed"] == topo["closed"]
    for n in iterations:
        for pin, mu in ((True, -0.53), (False, -0.53), (True, 0.0)) if full else ((True, -0.53),):
            want = sm.smooth(v, f, n, 0.5, mu, pin, topo=topo)
            _same(mesh_tools.smooth(dv, df, n, 0.5, mu, pin, adjacency=adj), want, f"smooth n={n} pin={pin} mu={mu}")
    _same(mesh_tools.smooth(dv, df, 2), sm.smooth(v, f, 2, topo=topo), "smooth with a fresh adjacency")
    _same(mesh_tools.smooth(dv, df, 1, 1.0, -1.5, adjacency=adj), sm.smooth(v, f, 1, 1.0, -1.5, topo=topo), "smooth with other factors")
    want = sm.vertex_normals(v, f, topo=topo)
    _same(mesh_tools.vertex_normals(dv, df, adjacency=adj), want, "vertex normals (reused adjacency)")
    _same(mesh_tools.vertex_normals(dv, df), want, "vertex normals (fresh adjacency)")
    _check_adjacency(adj, topo, len(v))                               # the calls left the lists alone
    return adj


# ---- the hand-built meshes -----------------------------------------------------------------------------------------------
HAND = {"triangle": sm.TRIANGLE, "tetrahedron": sm.TETRAHEDRON, "two_triangles": sm.TWO_TRIANGLES, "two_flipped": sm.TWO_TRIANGLES_FLIPPED,
        "three_on_an_edge": sm.THREE_ON_AN_EDGE, "twice": sm.TWICE, "degenerate": sm.DEGENERATE, "octahedron": sm.OCTAHEDRON,
        "isolated": sm.with_isolated(sm.TETRAHEDRON, 2), "no_vertex": (np.zeros((0, 3), F), np.zeros((0, 3), np.int32)),
        "no_face": (np.arange(15, dtype=F).reshape(5, 3), np.zeros((0, 3), np.int32))}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_meshes(name):
    _check_mesh(*HAND[name])


def test_noisy_open_grid():
    v, f = sm.grid(40, 40, noise=0.3, seed=7)
    adj = _check_mesh(v, f)
    assert adj.totals.tolist()[3] == 4 * 39 and adj.totals.tolist()[5] == 4 * 39


def test_icosphere():
    v, f = sm.icosphere(3, noise=0.02, seed=4)
    adj = _check_mesh(v, f)
    t = adj.totals.tolist()
    assert (t[2], t[3], t[4], t[7]) == (1920, 0, 0, 1280)


def test_hub_fan_of_degree_200():
    v, f = sm.hub_fan(200)
    adj = _check_mesh(v, f)
    off = adj.lists()["neighbour_offsets"].cpu().numpy()
    assert off[1] - off[0] == 201


# V and 6 F one below, at and one above a multiple of the workgroup size (6 F is a multiple of 6: the nearest values on either
# side stand in where the multiple itself cannot be hit) and of the scan's block span
_AT = 3 * TPB // 6                       # 6 F = 3 TPB, a multiple of both
SMALL = [(V, nf) for V in (TPB - 1, TPB, TPB + 1) for nf in (_AT - 1, _AT, _AT + 1)]
LARGE = [(87 * TPB - 1, SPAN // 6), (87 * TPB, SPAN // 6 + 1), (258 * TPB + 1, 3 * SPAN // 6)]      # 6 F = SPAN - 4, SPAN + 2, 3 SPAN


@pytest.mark.parametrize("V,nf", SMALL)
def test_sizes_around_the_workgroup(V, nf):
    v, f = sm.trimmed_grid(V, nf, seed=V + nf)
    assert v.shape == (V, 3) and f.shape == (nf, 3)
    _check_mesh(v, f, iterations=(1, 2), full=False)


@pytest.mark.parametrize("V,nf", LARGE)
def test_sizes_around_the_scan_span(V, nf):
    from binocular3dgs_amd import mesh_tools
    assert SPAN % 6 == 4 and (6 * LARGE[0][1] < SPAN < 6 * LARGE[1][1]) and 6 * LARGE[2][1] == 3 * SPAN
    v, f = sm.trimmed_grid(V, nf, seed=nf)
    topo = sm.topology(v, f)
    dv, df = _dev(v, F), _dev(f, np.int32)
    adj = mesh_tools.adjacency(dv, df)
    _check_adjacency(adj, topo, V)
    _same(mesh_tools.smooth(dv, df, 1, adjacency=adj), sm.smooth(v, f, 1, topo=topo), "smooth")
    _same(mesh_tools.vertex_normals(dv, df, adjacency=adj), sm.vertex_normals(v, f, topo=topo), "vertex normals")


def test_bad_faces_and_a_nan_vertex_are_counted_and_the_next_call_is_right():
    from binocular3dgs_amd import mesh_tools
    v, f = sm.with_bad_face(sm.grid(9, 7, noise=0.2, seed=3))
    v = v.copy()
    v[17, 1] = np.nan
    topo = sm.topology(v, f)
    assert topo["bad_faces"] == 2 and topo["nonfinite_vertices"] == 1
    dv, df = _dev(v, F), _dev(f, np.int32)
    adj = mesh_tools.adjacency(dv, df)
    _check_adjacency(adj, topo, len(v))                                # the lists do not depend on the coordinates
    with pytest.raises(ValueError, match="2 triangles name a vertex outside"):
        mesh_tools.smooth(dv, df, 2, adjacency=adj)
    with pytest.raises(ValueError, match="2 triangles name a vertex outside"):
        mesh_tools.vertex_normals(dv, df)
    info = mesh_tools.topology(dv, df, adjacency=adj)
    assert info["bad_faces"] == 2 and info["nonfinite_vertices"] == 1 and info["good_faces"] == len(f) - 2
    good = _dev(f[:-2], np.int32)
    with pytest.raises(ValueError, match="1 vertices have a coordinate that is not finite"):
        mesh_tools.smooth(dv, good, 1)
    with pytest.raises(ValueError, match="built for another mesh"):
        mesh_tools.smooth(dv, good, 1, adjacency=adj)
    # the calls returned: a valid mesh on the same stream, and the same holder with finite vertices
    _check_mesh(*sm.grid(9, 7, noise=0.2, seed=3), iterations=(2,), full=False)
    v[17, 1] = 0.5
    out = mesh_tools.smooth(_dev(v, F), df, 2, adjacency=adj, check=False)
    assert adj.totals.tolist()[:2] == [2, 0]
    _same(out, sm.smooth(v, f, 2, topo=topo), "smooth past the bad faces")


# ---- the shaded resolve --------------------------------------------------------------------------------------------------
W, H = 37, 29
BG = (0.25, 0.5, 0.75)


def _shaded_scene(name):
    if name == "icosphere":
        v, f = sm.icosphere(2, noise=0.03, seed=5)
        return v, f, rr.orbit_cameras(2, (0.0, 0.0, 0.0), 3.0, 36.0, height=0.4)
    v, f = sm.TWO_TRIANGLES
    return v, f, rr.orbit_cameras(2, (0.5, 0.5, 0.1), 2.5, 30.0, height=0.3)           # the two views see the two sides


@pytest.fixture(scope="module", params=["icosphere", "two_triangles"])
def shaded(request):
    v, f, cams = _shaded_scene(request.param)
    n = sm.vertex_normals(v, f)
    ref = rr.render(v, None, f, cams, W, H, shading="normal")
    if request.param == "two_triangles":
        windings = set()
        for k in range(2):
            X, Y = rr.project(v, cams[k], W, H)[:2]
            windings.add(rr.setup([int(X[q]) for q in f[0]], [int(Y[q]) for q in f[0]], W, H)["winding"])
        assert windings == {1, -1} and all((ref["triangle_id"][k] >= 0).sum() > 20 for k in range(2))
    return {"v": v, "f": f, "n": n, "cams": cams, "ref": ref, "want": {m: {bg: sm.resolve_shaded(v, n, f, cams, W, H, ref, m, bg or (0.0, 0.0, 0.0))
                                                                          for bg in (None, BG)} for m in ("smooth", "lit")}}


@pytest.mark.parametrize("mode", ["smooth", "lit"])
@pytest.mark.parametrize("boxes", [(-1, -1), (0, 2 ** 31 - 1), (0, 0)])
def test_shaded_resolve(shaded, mode, boxes):
    from binocular3dgs_amd import mesh_render, mesh_tools
    s = shaded
    dv, df = _dev(s["v"], F), _dev(s["f"], np.int32)
    dn = mesh_tools.vertex_normals(dv, df)
    _same(dn, s["n"], "vertex normals")
    plain = mesh_render.raster_views(dv, None, df, s["cams"], W, H, shading="normal", small_box=boxes[0], wave_box=boxes[1])
    for bg in (None, BG):
        dbg = None if bg is None else torch.tensor(bg, device=DEV)
        fp = torch.zeros(len(s["f"]), dtype=torch.int32, device=DEV)
        tid, depth, alpha, colour, counts = mesh_render.raster_views_shaded(dv, dn, df, s["cams"], W, H, dbg, mode=mode, face_pixels=fp,
                                                                            small_box=boxes[0], wave_box=boxes[1])
        for got, old, key in ((tid, plain[0], "triangle_id"), (depth, plain[1], "depth"), (alpha, plain[2], "alpha")):
            _same(got, old, key + " against the existing resolve")
            _same(got, s["ref"][key], key)
        _same(counts, plain[4], "counts")
        _same(fp, s["ref"]["face_pixels"], "face_pixels")
        _same(colour, s["want"][mode][bg], f"colour {mode} bg={bg}")
    if mode == "lit":
        c = colour.cpu().numpy()
        covered = s["ref"]["triangle_id"] >= 0
        grey = c[:, 0][covered]
        assert (grey >= 0.15).all() and (grey <= 1.0).all() and np.array_equal(grey, c[:, 1][covered]) and np.array_equal(grey, c[:, 2][covered])
    outs, rejected = mesh_render.render_mesh_shaded(dv, dn, df, s["cams"], None, mode=mode, size=(W, H))
    _same(torch.stack([o["render"] for o in outs]), s["want"][mode][None], "render_mesh_shaded")
    assert rejected.tolist() == [0, 0, 0]
    idx, batch = next(mesh_render.batches_shaded(dv, dn, df, s["cams"], None, mode=mode, size=(W, H)))
    assert idx == [0, 1]
    _same(torch.stack([o["render"] for o in batch]), s["want"][mode][None], "batches_shaded")


# ---- captured in a graph -------------------------------------------------------------------------------------------------
def test_adjacency_smooth_and_normals_in_one_graph_read_nothing():
    """a host read during capture would fail it; two replays give the same bits, for changed vertices too"""
    from binocular3dgs_amd import mesh_tools
    v, f = sm.grid(23, 17, noise=0.3, seed=11)
    topo = sm.topology(v, f)
    dv, df = _dev(v, F), _dev(f, np.int32)

    def calls():
        adj = mesh_tools.adjacency(dv, df)
        out = mesh_tools.smooth(dv, df, 3, adjacency=adj, check=False)
        return adj, out, mesh_tools.vertex_normals(out, df, adjacency=adj, check=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        adj, out, nrm = calls()
    v2 = sm.grid(23, 17, noise=0.3, seed=12)[0]
    for verts in (v, v, v2):
        dv.copy_(torch.from_numpy(verts))
        out.zero_()
        nrm.zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = sm.smooth(verts, f, 3, topo=topo)
        _same(out, want, "smooth in the graph")
        _same(nrm, sm.vertex_normals(want, f, topo=topo), "normals in the graph")
        _check_adjacency(adj, topo, len(v))


# ---- the command lines ---------------------------------------------------------------------------------------------------
def test_extract_mesh_smooth_normals_and_spiral_lit(tmp_path, capsys):
    from binocular3dgs_amd import extract_mesh, frames, mesh, mesh_tools, spiral
    from test_gpu_meshraster import _shell_model
    path, model, cams = _shell_model(tmp_path)
    bg = torch.zeros(3, device=DEV)
    v, c, f = mesh.fuse_model(model, cams, bg, resolution=24)
    out_dir = os.path.join(path, "mesh", "iteration_7")
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24", "--smooth", "3", "--normals"]) == 0
    printed = capsys.readouterr().out
    want_v = mesh_tools.smooth(v, f, 3)
    want_n = mesh_tools.vertex_normals(want_v, f)
    assert f"smoothed: {v.shape[0]} vertices, 6 steps (lambda 0.5, mu -0.53, boundary pinned)" in printed
    assert mesh_tools.topology_line(mesh_tools.topology(want_v, f)) in printed and "topology: " in printed
    ply = os.path.join(out_dir, "mesh.ply")
    pv, pc, pf, pn = mesh.read_mesh_ply(ply, return_normals=True)
    _same(pv, want_v, "the smoothed vertices of the file")
    _same(pn, want_n, "the normals of the file")
    assert np.array_equal(pc, c.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy()) and (pv != v.cpu().numpy()).any()
    _same(want_v, sm.smooth(v.cpu().numpy(), f.cpu().numpy(), 3), "smooth of the extraction against the yardstick")
    # the Laplacian filter with a free boundary, and no normals in the file
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24", "--smooth", "2", "--smooth_mu", "0", "--free_boundary"]) == 0
    assert "2 steps (lambda 0.5, mu 0, boundary free)" in capsys.readouterr().out
    pv, _, _, pn = mesh.read_mesh_ply(ply, return_normals=True)
    assert pn is None
    _same(pv, mesh_tools.smooth(v, f, 2, mu=0.0, pin_boundary=False), "the Laplacian filter of the file")
    # spiral --shading lit / smooth: normals from the file, or computed on load
    src = os.path.join(ROOT, "tests", "golden", "scene_llff")
    assert spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "4", "--mesh", ply, "--shading", "lit"]) == 0
    assert "(lit)" in capsys.readouterr().out
    render_dir = os.path.join(path, "render", "mesh_scene_llff")
    pngs = sorted(os.listdir(render_dir))
    assert len(pngs) == 12
    lit = frames.read_png(os.path.join(render_dir, "00000.png"))
    assert lit.ndim == 3 and np.array_equal(lit[..., 0], lit[..., 1]) and np.array_equal(lit[..., 0], lit[..., 2]) and lit.max() > 38
    mesh.write_mesh_ply(ply, want_v, c, f, want_n)
    assert spiral.main(["-m", path, "-s", src, "-r", "8", "--frames", "4", "--mesh", ply, "--shading", "smooth"]) == 0
    assert "(smooth)" in capsys.readouterr().out and len(os.listdir(render_dir)) == 12


def test_eval_mesh_prints_the_topology_line(tmp_path, capsys):
    from binocular3dgs_amd import eval_mesh, mesh, mesh_tools
    from binocular3dgs_amd.matcher_cloud import write_cloud_ply
    v, f = sm.icosphere(2)
    ply, cloud = str(tmp_path / "sphere.ply"), str(tmp_path / "gt.ply")
    mesh.write_mesh_ply(ply, v, np.zeros(v.shape, np.uint8), f)
    write_cloud_ply(cloud, v, np.zeros(v.shape, np.uint8))
    assert eval_mesh.main(["--mesh", ply, "--gt", cloud, "--spacing", "0.2", "--max_dist", "0.5", "--tau", "0.1"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[0] == "topology: 162 vertices (0 isolated), 480 edges (0 boundary, 0 non-manifold), 320 triangles, euler 2, closed"
    assert lines[-1].startswith("{")
