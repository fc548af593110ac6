"""Screened Poisson reconstruction on the device (csrc/poisson.hip, binocular3dgs_amd/poisson.py) against the numpy restatement
of tests/poisson_ref.py.  Every float statement is one correctly rounded operation on both sides and every sum across nodes one
fixed fp64 tree, so samples, density, right-hand side, operator, solution, the solver's scalars, the level, the support plane and
the extracted mesh are compared bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402
import poisson_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
GRIDS = {"odd": (20, 17, 13), "row65": (65, 3, 2), "cube33": (33, 33, 33)}       # no size a multiple of 64 or 256; 65: a wave seam in a row
ORIGIN, VOXEL = (-1.25, 0.5, 2.0), 0.125
W, H = 24, 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, f"{what}: shape {g.shape} != {w.shape}"
    assert np.array_equal(g, w), f"{what}: {(g != w).sum()} of {g.size} words differ"


def _cloud(dims, n, seed, origin=ORIGIN, voxel=VOXEL):
    """n oriented samples: grid coordinates uniform over the cells (a tenth of them beyond the grid), random unit normals and
    weights, every eighth weight zero"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.6, np.asarray(dims, np.float64) - 0.4, (n, 3))
    p = (np.asarray(origin) + (c + 0.5) * voxel).astype(F)
    nr = rng.standard_normal((n, 3))
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
    w = rng.uniform(0.1, 1.0, n).astype(F)
    w[::8] = 0.0
    return p, nr, w


def _volume(dims, origin=ORIGIN, voxel=VOXEL):
    from binocular3dgs_amd.poisson import PoissonVolume
    return PoissonVolume.from_dims(origin, dims, voxel, device=DEV)


def _head(vol):
    """int64 [8] head of the workspace: dropped, samples, status, iterations, done, bits of r.r, bits of b.b"""
    return vol._ws[:64].view(torch.int64).cpu().numpy()


# ---- oriented samples --------------------------------------------------------------------------------------------------
def _views(n, seed=0):
    """n views of a tilted plane in front of turned cameras with everything the rule tests for: an alpha hole at a neighbour
    only, a band below alpha_min, a depth step, a patch of depth 0 (|n| = 0 and |P| = 0), a patch of tiny depth (|n| = 0 alone), a grazing region"""
    rng = np.random.default_rng(seed)
    cams, depths, alphas, colours, medians = np.zeros((n, 14), F), [], [], [], []
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    for k in range(n):
        yaw = 0.07 * (k - 3)
        R = np.array([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]])
        centre = np.array([0.2 * (k - 3), 0.05 * k, 0.0])
        cams[k, :9], cams[k, 9:12], cams[k, 12], cams[k, 13] = R.reshape(9), -R @ centre, 18.0 + k, 19.0 - 0.5 * k
        z = 3.0 + 0.04 * (u - W / 2) * (1 + 0.2 * k) + 0.03 * (v - H / 2) + 0.002 * rng.standard_normal((H, W))
        z[:, 16:] += 0.5                                             # a depth step between columns 15 and 16
        z[12:16, 2:6] = 0.0                                          # zero depth: the five points coincide, |n| = |P| = 0, c = 0 / 0
        z[12:16, 8:12] = 3e-12                                       # tiny depth: |P| > 0 but n n underflows, |n| = 0 and c = x / 0 = +inf
        z[2:5, 18:22] += 0.12 * (u[2:5, 18:22] - 18)                  # steep: seen at a grazing angle
        alpha = np.full((H, W), 0.9)
        alpha[5, 7 + k % 3] = 0.2                                    # a hole: its four neighbours lose their sample too
        alpha[16:18, :] = 0.45                                       # below alpha_min
        alpha, z = alpha.astype(F), z.astype(F)
        depths.append((z * alpha).astype(F)), alphas.append(alpha), medians.append(z)
        colours.append(rng.uniform(size=(3, H, W)).astype(F))
    return cams, depths, alphas, colours, medians


@pytest.fixture(scope="module")
def views():
    cams, depths, alphas, colours, medians = _views(8)
    return {"cams": cams, "host": (depths, alphas, colours, medians), "dev": tuple([_dev(a) for a in arrs] for arrs in (depths, alphas, colours, medians))}


@pytest.mark.parametrize("nviews,stride,median", [(8, 1, False), (8, 3, False), (1, 1, False), (1, 3, True), (8, 1, True)])
def test_oriented_points_match_the_yardstick(views, nviews, stride, median):
    from binocular3dgs_amd.poisson import oriented_points
    hd, ha, hc, hm = views["host"]
    dd, da, dc, dm = views["dev"]
    kw = dict(stride=stride, alpha_min=0.5, rel_jump=0.05, min_cos=0.9, median=median)
    want = pr.oriented_points(views["cams"][:nviews], (hm if median else hd)[:nviews], ha[:nviews], hc[:nviews], **kw)
    got = oriented_points(views["cams"][:nviews], (dm if median else dd)[:nviews], da[:nviews], dc[:nviews], **kw)
    full = (W - 2) // stride * ((H - 2) // stride) * nviews
    assert 0 < len(want[2]) < full                                   # the count: some pixels pass, the planted ones do not
    for g, w, name in zip(got, want, ("points", "normals", "weights", "colours")):
        _same(g, w, name)                                            # (the order too: rows are compared in place)
    if stride == 1 and not median and nviews == 8:
        # every planted reason rejects something: loosening one rule at a time admits more pixels
        base = len(want[2])
        for loose in (dict(rel_jump=1.0), dict(min_cos=-1.0), dict(alpha_min=0.1)):
            assert len(pr.oriented_points(views["cams"], hd, ha, hc, **dict(kw, **loose))[2]) > base, loose
        zero = pr.oriented_points(views["cams"][:1], hd[:1], ha[:1], hc[:1], **dict(kw, rel_jump=1e9, min_cos=-1.0))
        mutant = pr.oriented_points(views["cams"][:1], hd[:1], ha[:1], hc[:1], **dict(kw, rel_jump=1e9, min_cos=-1.0), zero_normal_rule=False)
        assert len(mutant[2]) > len(zero[2])                         # the |n| > 0 rule alone refuses the tiny-depth patch (c = +inf there)
        assert len(zero[2]) < (W - 2) * (H - 2) - 2 * (W - 2) - 5    # the zero-depth patch is still refused: |n| = 0, and c is NaN


def test_nine_views_go_in_two_launches(views):
    from binocular3dgs_amd.poisson import oriented_points
    hd, ha, hc, _ = views["host"]
    dd, da, dc, _ = views["dev"]
    cams = np.concatenate([views["cams"], views["cams"][:1]])
    want = pr.oriented_points(cams, hd + hd[:1], ha + ha[:1], hc + hc[:1], 2, 0.5, 0.05, 0.9)
    got = oriented_points(cams, dd + dd[:1], da + da[:1], dc + dc[:1], stride=2, alpha_min=0.5, rel_jump=0.05, min_cos=0.9)
    for g, w, name in zip(got, want, ("points", "normals", "weights", "colours")):
        _same(g, w, name)


# ---- splat -------------------------------------------------------------------------------------------------------------
def _splat_case(name, dims):
    if name == "random":
        return _cloud(dims, 900, 1)
    rng = np.random.default_rng(2)
    if name == "integer":                                            # samples exactly on nodes: every fraction is 0
        c = np.stack([rng.integers(0, d, 200) for d in dims], axis=1).astype(np.float64)
    elif name == "last_cell":                                        # the last admissible cell and just beyond it
        hi = np.asarray(dims, np.float64) - 1.0
        c = np.concatenate([hi - rng.uniform(0.001, 0.999, (60, 3)), hi + rng.uniform(0.0, 0.5, (20, 3)), -rng.uniform(0.001, 0.4, (20, 3))])
    else:                                                            # 300 samples in one cell
        c = np.asarray([min(3, d - 2) for d in dims], np.float64) + rng.uniform(0.0, 0.999, (300, 3))
    p = c.astype(F)                                                  # origin -0.5, voxel 1: grid coordinate = position
    nr = rng.standard_normal((len(p), 3)).astype(F)
    w = rng.uniform(0.0, 2.0, len(p)).astype(F)
    w[::5] = 0.0
    return p, nr, w


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("case", ["random", "integer", "last_cell", "one_cell"])
def test_splat_matches_the_yardstick(grid, case):
    dims = GRIDS[grid]
    origin, voxel = (ORIGIN, VOXEL) if case == "random" else ((-0.5, -0.5, -0.5), 1.0)
    p, nr, w = _splat_case(case, dims)
    density, vector, dropped = pr.splat(p, nr, w, dims, origin, voxel)
    if case in ("random", "last_cell"):
        assert 0 < dropped < len(p)
    if case == "integer":
        assert dropped > 0 and (density > 0).sum() <= len(p)         # (nodes of the last plane have no cell above them)
    vol = _volume(dims, origin, voxel)
    vol.splat(_dev(p), _dev(nr), _dev(w))
    _same(vol.density, density, "density")
    _same(vol.vector, vector, "vector")
    assert _head(vol)[:2].tolist() == [dropped, len(p)]


# ---- operator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(GRIDS))
def test_operator_matches_the_yardstick(grid):
    from binocular3dgs_amd import _C
    dims = GRIDS[grid]
    rng = np.random.default_rng(3)
    shape = dims[::-1]
    x = rng.standard_normal(shape).astype(F)                          # every face, edge and corner node carries a value
    density = (rng.uniform(size=shape) * (rng.uniform(size=shape) < 0.4)).astype(F)
    _same(_C.poisson_apply(_dev(density), 4.0, _dev(x)), pr.apply(density, 4.0, x), "A x")


# ---- solver ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solved():
    """Per grid: the cloud, the yardstick's splat and its solutions, computed once"""
    out = {}
    for name, dims in GRIDS.items():
        p, nr, w = _cloud(dims, 1500 if name == "cube33" else 400, 4)
        density, vector, dropped = pr.splat(p, nr, w, dims, ORIGIN, VOXEL)
        out[name] = {"dims": dims, "cloud": (p, nr, w), "density": density, "vector": vector, "dropped": dropped, "sol": {}}
    return out


def _ref_solve(s, iters, tol):
    key = (iters, tol)
    if key not in s["sol"]:
        s["sol"][key] = pr.solve(s["density"], s["vector"], 4.0, iters, tol, len(s["cloud"][2]) - s["dropped"])
    return s["sol"][key]


def _device_solve(s, iters, tol, **kw):
    vol = _volume(s["dims"])
    vol.splat(*[_dev(a) for a in s["cloud"]])
    info = vol.solve(4.0, iters, tol, **kw)
    return vol, info


def _assert_solution(vol, info, ref):
    _same(vol.rhs, ref["rhs"], "rhs")
    _same(vol.x, ref["x"], "x")
    head = _head(vol)
    assert head[3] == info["iterations"] == ref["iterations"] and int(vol.iterations().item()) == ref["iterations"]
    assert bool(head[4]) == ref["done"] and head[2] == 0
    assert head[5:7].view(np.float64).tolist() == [ref["rr"], ref["bb"]]


@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("iters", [0, 1, 40])
def test_conjugate_gradients_match_the_yardstick(solved, grid, iters):
    s = solved[grid]
    ref = _ref_solve(s, iters, 0.0)
    assert ref["iterations"] == iters
    vol, info = _device_solve(s, iters, 0.0)
    _assert_solution(vol, info, ref)


@pytest.mark.parametrize("grid", ["odd", "cube33"])
def test_tolerance_stops_early_and_later_launches_change_nothing(solved, grid):
    s = solved[grid]
    ref = _ref_solve(s, 40, 0.05)
    assert 0 < ref["iterations"] < 40 and ref["done"]
    vol, info = _device_solve(s, 40, 0.05)                            # all 40 iterations are launched: the rest return at once
    _assert_solution(vol, info, ref)
    assert info["residual"] <= 0.05


@pytest.mark.parametrize("grid", ["odd", "cube33"])
def test_launch_geometry_changes_no_bit(solved, grid):
    s = solved[grid]
    ref = _ref_solve(s, 40, 0.0)
    for max_blocks in (1, 7):                                         # one workgroup walks every chunk; 7: an uneven share
        vol, info = _device_solve(s, 40, 0.0, max_blocks=max_blocks)
        _assert_solution(vol, info, ref)


def test_a_grid_no_sample_fits_is_refused():
    from binocular3dgs_amd._lib import B3gsError
    vol = _volume((1, 1, 1))
    vol.splat(_dev(np.asarray([[-1.2, 0.55, 2.05]], F)), _dev(np.asarray([[0.0, 0.0, 1.0]], F)), _dev(np.ones(1, F)))
    assert _head(vol)[:2].tolist() == [1, 1] and float(vol.density.abs().max()) == 0.0
    with pytest.raises(B3gsError, match="8 nodes"):
        vol.solve()
    assert _head(vol)[2] == 1 and _head(vol)[3] == 0


# ---- volume and end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [0, 2])
@pytest.mark.parametrize("grid", ["odd", "row65"])
def test_level_and_support_match_the_yardstick(solved, grid, spread):
    s = solved[grid]
    ref = _ref_solve(s, 40, 0.0)
    want, iso = pr.to_volume(s["density"], ref["x"], spread, ORIGIN, VOXEL)
    vol, _ = _device_solve(s, 40, 0.0)
    tv = vol.to_tsdf(spread)
    _same(tv.tsdf, want["tsdf"], "tsdf")
    _same(tv.weight, want["weight"], "weight")
    assert float(tv.rgb.abs().max()) == 0.0
    if spread == 0:
        _same(tv.weight, s["density"] + F(0.0), "weight at spread 0 is the density")


@pytest.fixture(scope="module")
def sphere():
    case = pr.sphere_case(3000, 32, 4)
    v, c, f, info = pr.reconstruct(case["points"], case["normals"], case["weights"], case["dims"], case["origin"], case["voxel"], spread=1)
    return case, (v, c, f), info


def test_sphere_mesh_equals_the_yardstick(sphere):
    case, (rv, rc, rf), info = sphere
    vol = _volume(case["dims"], case["origin"], case["voxel"])
    vol.splat(_dev(case["points"]), _dev(case["normals"]), _dev(case["weights"]))
    got = vol.solve()
    assert got["iterations"] == info["iterations"] and got["dropped"] == 0
    _same(vol.x, info["x"], "x")
    v, c, f = vol.extract(0.0, 1)
    assert np.array_equal(f.cpu().numpy(), rf)
    _same(v, rv, "vertices")
    assert np.array_equal(c.cpu().numpy(), rc)


def test_reconstruct_gives_a_closed_sphere(sphere):
    from binocular3dgs_amd import mesh_tools
    from binocular3dgs_amd.poisson import reconstruct
    case = sphere[0]
    colours = np.clip(case["points"] * 0.5 + 0.5, 0.0, 1.0).astype(F)
    v, c, f, vol, info = reconstruct(_dev(case["points"]), _dev(case["normals"]), None, _dev(colours), resolution=32, return_volume=True)
    topo = mesh_tools.topology(v, f)
    assert topo["closed"] and topo["euler"] == 2 and info["residual"] <= 1e-4
    radius = v.double().norm(dim=1)
    assert float((radius - 1.0).abs().mean()) / vol.voxel_size <= 0.0171 + 0.5       # (the bound of tests/test_poisson_ref_cpu.py)
    want = (v * 0.5 + 0.5).clamp(0, 1) * 255.0                                        # a vertex takes its nearest sample's colour
    assert float((c.float() - want).abs().max()) <= 0.5 * 255.0 * 4 * vol.voxel_size + 1.0


# ---- through fuse_model ------------------------------------------------------------------------------------------------
def test_fuse_model_poisson_closes_what_tsdf_leaves_open():
    from binocular3dgs_amd import mesh, mesh_tools, synth
    from binocular3dgs_amd.evaluate import _batches
    Ws, Hs = 160, 120
    model = synth.synth_model(4000, seed=3, device=DEV, width=Ws, height=Hs, requires_grad=False)
    cams = synth.synth_cameras(Ws, Hs, yaws=(-8.0, 0.0, 8.0), device=DEV)
    bg = torch.zeros(3, device=DEV)
    v0, c0, f0, vol0 = mesh.fuse_model(model, cams, bg, resolution=32, return_volume=True)
    v1, c1, f1, vol1 = mesh.fuse_model(model, cams, bg, resolution=32, return_volume=True, method="tsdf")
    assert torch.equal(v0, v1) and torch.equal(c0, c1) and torch.equal(f0, f1) and torch.equal(vol0.tsdf, vol1.tsdf)
    # method="tsdf" is the path of mesh.py as it was: the yardstick of tests/mesh_ref.py, fed the same renders
    table = mesh.camera_table(cams)
    ref = mr.new_volume(vol0.dims, vol0.origin, vol0.voxel_size)
    for idx, outs in _batches(model, cams, bg, 8, full=True):
        host = [[o[key].cpu().numpy() for o in outs] for key in ("rendered_depth", "rendered_alpha", "render")]
        mr.integrate(ref, table[idx], host[0], host[1], host[2], vol0.truncation)
    rv, rc, rf = mr.extract(ref)
    assert np.array_equal(f1.cpu().numpy(), rf) and np.array_equal(_bits(v1), _bits(rv)) and np.array_equal(c1.cpu().numpy(), rc)
    info = {}
    v2, c2, f2, vol2 = mesh.fuse_model(model, cams, bg, resolution=32, return_volume=True, method="poisson", info=info)
    assert vol2.dims == vol0.dims and f2.shape[0] > 0 and info["samples"] > info["dropped"] and c2.dtype == torch.uint8
    open_tsdf = mesh_tools.topology(v1, f1)["boundary_edges"]
    open_poisson = mesh_tools.topology(v2, f2)["boundary_edges"]
    print(f"boundary edges: tsdf {open_tsdf}, poisson {open_poisson}; {info}")
    assert open_poisson < open_tsdf
    v3, _, f3 = mesh.fuse_model(model, cams, bg, resolution=32, method="poisson", depth="median", sample_stride=2, trim=0.5)
    assert f3.shape[0] > 0


# ---- argument errors ---------------------------------------------------------------------------------------------------
def test_argument_errors(views):
    from binocular3dgs_amd import _C, _lib
    from binocular3dgs_amd.poisson import oriented_points
    L = _lib.lib()
    dd, da, dc, _ = views["dev"]
    g = _lib.B3gsTsdfVolume()
    g.nx, g.ny, g.nz, g.voxel = 4, 4, 4, 1.0
    one = C.c_void_p(256)                                            # never dereferenced: the checks come first
    for screen in (0.0, -1.0, float("nan")):
        assert L.b3gs_poisson_solve(C.byref(g), one, one, screen, 1, 1e-4, 0, one, one, one, None) == -1
        assert b"screening" in L.b3gs_last_error()
        assert L.b3gs_poisson_apply(C.byref(g), one, screen, one, C.c_void_p(512), None) == -1
    vol = _volume((4, 4, 4))
    vol.splat(*[_dev(a) for a in _cloud((4, 4, 4), 20, 0)])
    with pytest.raises(ValueError, match="screening"):
        vol.solve(0.0)
    with pytest.raises(ValueError, match="share one H x W"):
        _C.oriented_points_count([dd[0], dd[1][:10]], [da[0], da[1][:10]], [dc[0], dc[1][:, :10]], torch.from_numpy(views["cams"][:2]), 1, 0.5, 0.05, 0.1)
    nine = [dd[0]] * 9
    with pytest.raises(ValueError, match="1 .. 8 views"):
        _C.oriented_points_count(nine, [da[0]] * 9, [dc[0]] * 9, torch.from_numpy(np.repeat(views["cams"][:1], 9, axis=0)), 1, 0.5, 0.05, 0.1)
    tv = _lib.B3gsTsdfView()
    assert L.b3gs_oriented_points_batch(9, C.byref(tv), W, H, 1, 0.5, 0.05, 0.1, 0, one, None) == -1
    # sizes no workspace exists for are a 0 size; a workspace that is too small is refused
    assert L.b3gs_poisson_workspace_bytes(0, 4, 4, 10) == 0 and L.b3gs_poisson_workspace_bytes(4, 4, 1025, 10) == 0
    assert L.b3gs_poisson_workspace_bytes(4, 4, 4, -1) == 0 and L.b3gs_oriented_points_workspace_bytes(9, W, H) == 0
    need = L.b3gs_poisson_workspace_bytes(4, 4, 4, 20)
    assert need > 0 and need % 256 == 0 and L.b3gs_poisson_workspace_bytes(4, 4, 4, 2000) > need
    small = torch.empty(need - 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="workspace is too small"):
        _C.poisson_splat(*[_dev(a) for a in _cloud((4, 4, 4), 20, 0)], [4, 4, 4], [0.0, 0.0, 0.0], 1.0, small)
    with pytest.raises(ValueError):
        oriented_points(views["cams"][:2], dd[:1], da[:1], dc[:1])
