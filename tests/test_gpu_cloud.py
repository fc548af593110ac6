"""The matcher cloud on the device (csrc/cloud.hip, binocular3dgs_amd/matcher_cloud.py) against golden G15
(tests/golden/cloud.npz: the statements of the reference's triangulate.py, recorded on CPU tensors) and the float64
restatements of tests/cloud_ref.py.  Masks, orders and candidate positions are exact; every tolerance is derived in the
issue or stored by the maker from the reference's own rounding noise.  Measured on an MI355X:
points 3.3e-7 of the distance (bound 1e-6), sheet 9.5e-7 (bound 4.3e-6), SSIM 7.2e-6 (bound d = 3.05e-5)."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "cloud.npz"))


def _colors_match(got_u8, want_f):
    """equal as uint8 except where the recorded float colour lies within 1e-3 of an integer (at most 1 % of the entries)"""
    near = np.abs(want_f - np.round(want_f)) < 1e-3
    assert near.mean() <= 0.01
    return np.array_equal(got_u8[~near], want_f.astype(np.uint8)[~near])


def test_triangulation_mask_order_points_and_colours(g):
    from binocular3dgs_amd import matcher_cloud as mc
    K, c2ws, imgs = g["scene/K"], g["scene/c2ws"], g["scene/images"]
    worst = 0.0
    for name in g["pair/names"].tolist():
        ref, src = (int(v) for v in name.split("_"))
        tag = f"pair/{name}"
        kp0, kp1, kept = g[tag + "/kp_ref"], g[tag + "/kp_src"], g[tag + "/kept"]
        pts, col = mc.triangulate_pair(mc.PinholeView(K, c2ws[ref]), mc.PinholeView(K, c2ws[src]), kp0, kp1, imgs[ref], device=DEV)
        pts, col = pts.cpu().numpy(), col.cpu().numpy()
        assert len(pts) == int(kept.sum()), name
        # order and identity: every kept row is the float64 DLT of ITS match, within 1e-6 of its distance to the reference camera
        want = g[tag + "/dlt64"][kept]
        dist = np.linalg.norm(want - c2ws[ref][:3, 3].astype(np.float64), axis=1)
        rel = np.abs(pts - want).max(1) / dist
        worst = max(worst, float(rel.max()))
        assert rel.max() < 1e-6, (name, rel.max())
        assert np.abs(pts - g[tag + "/points"]).max() <= 1e-6 * dist.max()
        assert _colors_match(col, g[tag + "/colors_f"]), name
    print("triangulation: largest |point - float64 DLT| / distance =", worst)
    # the match exactly on the W-1 edge is kept
    ref, src, row = g["pair/edge"].tolist()
    assert g[f"pair/{ref}_{src}/kept"][row]


def test_triangulation_of_nothing_and_of_many():
    from binocular3dgs_amd import matcher_cloud as mc
    cam = mc.PinholeView(np.array([[64, 0, 32], [0, 64, 24], [0, 0, 1]], np.float32), np.eye(4, dtype=np.float32))
    c2 = np.eye(4, dtype=np.float32)
    c2[0, 3] = 5.0
    img = np.full((48, 64, 3), 7, np.uint8)
    p, c = mc.triangulate_pair(cam, mc.PinholeView(cam.intrinsic, c2), np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), img, device=DEV)
    assert p.shape == (0, 3) and c.shape == (0, 3)
    # 3000 matches of points at depth 50 (several blocks of the scan), every third one pushed out of the threshold
    rng = np.random.default_rng(1)
    X = np.stack([rng.uniform(-10, 10, 3000), rng.uniform(-8, 8, 3000), np.full(3000, 50.0)], 1)
    k0, k1 = cloud_ref.project_f64(X, cam.intrinsic, cam.c2w), cloud_ref.project_f64(X, cam.intrinsic, c2)
    k1[::3, 1] += 9.0
    p, c = mc.triangulate_pair(cam, mc.PinholeView(cam.intrinsic, c2), k0.astype(np.float32), k1.astype(np.float32), img, device=DEV)
    keep = np.ones(3000, bool)
    keep[::3] = False
    assert len(p) == keep.sum() and np.abs(p.cpu().numpy() - X[keep]).max() < 1e-2
    # a constant image: the four fp32 weights sum to 1 within an ulp, and the cast truncates as astype(np.uint8) does
    col = c.cpu().numpy()
    assert ((col == 7) | (col == 6)).all() and (col == 7).mean() > 0.5


def test_background_sheet(g):
    from binocular3dgs_amd import matcher_cloud as mc
    v = int(g["sheet/view"])
    pts, col = mc.background_sheet(g["sheet/image"], g["scene/K"], g["scene/c2ws"][v], 10.0, device=DEV)
    mask = g["sheet/mask"]
    assert len(pts) == int(mask.sum()) and (col.cpu().numpy() == 255).all() and np.array_equal(col.cpu().numpy(), g["sheet/colors"])
    err = float(np.abs(pts.cpu().numpy() - g["sheet/points"]).max())
    print("background sheet: max |point - recorded| =", err, "bound", float(g["sheet/bound"]), "(reference fp32 vs float64:",
          float(g["sheet/max_ref_err"]), ")")
    assert err <= float(g["sheet/bound"])
    # order: the float64 points of exactly the masked pixels, in pixel order
    f64 = cloud_ref.sheet_points_f64(64, 48, g["scene/K"], g["scene/c2ws"][v], 10.0)[mask]
    assert np.abs(pts.cpu().numpy() - f64).max() < 1e-4


def test_background_sheet_across_the_seam_of_the_block_scan():
    """520 x 512 pixels are 1040 blocks of 256: two steps of the 1024-wide scan of the block counts.  The count and every row,
    in pixel order, against the float64 restatement.  Bound: a coordinate goes through about 20 float32 roundings on the device
    and two float32 matrix inversions on the host, each 2^-24 of a value no larger than scale = depth (W / fx + H / fy + 1) +
    |t|; 64 * 2^-24 * scale (1.2e-4 here) covers them.  Neighbouring pixels' points lie depth / fx = 0.02 apart, 160 times
    that, so a row out of order cannot pass."""
    from binocular3dgs_amd import matcher_cloud as mc
    W, H, depth = 520, 512, 10.0
    K = np.array([[500.0, 0, 260.0], [0, 500.0, 256.0], [0, 0, 1]], np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, :3] = [[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]]
    c2w[:3, 3] = [1.0, -2.0, 0.5]
    rng = np.random.default_rng(5)
    img = rng.integers(0, 254, (H, W, 3), dtype=np.uint8)
    # white pixels at a density that changes from row to row (block counts from 0 to 256), 254 and 255 both
    white = rng.random((H, W)) < np.linspace(0.0, 1.0, H)[:, None] ** 2
    white[200:203] = True
    white[300:303] = False
    img[white, rng.integers(0, 3, int(white.sum()))] = rng.integers(254, 256, int(white.sum()), dtype=np.uint8)
    mask = (img.max(axis=2) >= 254).ravel()
    assert np.array_equal(mask, white.ravel()) and 0.2 < mask.mean() < 0.5
    pts, col = mc.background_sheet(img, K, c2w, depth, device=DEV)
    assert len(pts) == int(mask.sum()) and (col.cpu().numpy() == 255).all()
    want = cloud_ref.sheet_points_f64(W, H, K, c2w, depth)[mask]
    scale = depth * (W / 500.0 + H / 500.0 + 1.0) + float(np.abs(c2w[:3, 3]).max())
    err = float(np.abs(pts.cpu().numpy() - want).max())
    print("sheet across the seam: kept", len(pts), "max |point - float64| =", err, "bound", 64 * 2.0 ** -24 * scale)
    assert err <= 64 * 2.0 ** -24 * scale


def _grower(g, capacity=None):
    from binocular3dgs_amd import matcher_cloud as mc
    refs = g["grow/ref_indices"].tolist()
    pts = torch.from_numpy(g["grow/start_points"]).to(DEV)
    col = torch.from_numpy(g["grow/start_colors"]).to(DEV)
    imgs = [g["scene/images"][i] for i in refs]
    return mc.CloudGrower(pts, col, imgs, g["scene/K"], g["scene/c2ws"][refs], capacity=capacity), {v: k for k, v in enumerate(refs)}


def _draw(g, i):
    ref, src, length = g[f"grow/{i}/views"].tolist()
    return ref, src, length, torch.from_numpy(g[f"grow/{i}/seed_idx"]).to(DEV, torch.int32), torch.from_numpy(g[f"grow/{i}/noise"]).to(DEV)


def _recount(gr, n):
    """the count grids of the first n points of the cloud, by torch"""
    fx, fy, cx, cy = gr.focal_center
    V, Hp, Wp = gr.grids.shape
    out = torch.zeros_like(gr.grids)
    p = gr.points[:n]
    for v in range(V):
        m = gr.w2c[v]
        q = p @ m[:3, :3].T + m[:3, 3]
        u, w = torch.round(q[:, 0] / q[:, 2] * fx + cx), torch.round(q[:, 1] / q[:, 2] * fy + cy)
        ok = (u >= -1) & (u <= Wp - 2) & (w >= -1) & (w <= Hp - 2)
        cell = ((w[ok] + 1) * Wp + (u[ok] + 1)).long()
        out[v].view(-1).index_add_(0, cell, torch.ones_like(cell, dtype=torch.int32))
    return out


def test_patch_ssim_of_round_one(g):
    gr, slot = _grower(g)
    ref, src, _, si, nz = _draw(g, 0)
    n = nz.shape[0] * nz.shape[1]
    ssim, mask = torch.full((n,), -1.0, device=DEV), torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    gr.round(slot[ref], slot[src], si, nz, debug_ssim=ssim, debug_mask=mask)
    want_mask, want = g["grow/0/mask"], g["grow/0/ssim"]
    assert np.array_equal(mask.cpu().numpy().astype(bool), want_mask)
    err = float(np.abs(ssim.cpu().numpy() - want)[want_mask].max())
    print("patch SSIM: max |ssim - recorded fp32| =", err, "bound d =", float(g["grow/ssim_bound"]), "(reference fp32 vs float64:",
          float(g["grow/ssim_max_ref_err"]), ")")
    assert err <= float(g["grow/ssim_bound"])
    assert (ssim.cpu().numpy()[~want_mask] == 0).all()


def _check_final(g, pts, col):
    want_p, want_c = g["grow/points"], g["grow/colors_f"]
    assert pts.shape == want_p.shape and np.array_equal(pts, want_p)                     # seed + noise * alpha, bit for bit
    n0 = len(g["grow/start_points"])
    assert np.array_equal(col[:n0], want_c[:n0])
    assert _colors_match(col[n0:].astype(np.uint8), want_c[n0:])


def test_growth_round_by_round(g):
    gr, slot = _grower(g)
    n0 = len(g["grow/start_points"])
    rounds = int(g["grow/rounds"])
    for i in range(rounds):
        ref, src, length, si, nz = _draw(g, i)
        before = int(gr.length.item())
        gr.round(slot[ref], slot[src], si, nz)
        assert int(gr.length.item()) == length, i
        # candidate identity and order of this round's appended points
        cand = (torch.from_numpy(g["grow/start_points"])[g[f"grow/{i}/seed_idx"]][:, None, :] + torch.from_numpy(g[f"grow/{i}/noise"]) * 10.0)
        want = cand.reshape(-1, 3)[g[f"grow/{i}/accepted"]].numpy()
        assert np.array_equal(gr.points[before:length].cpu().numpy(), want), i
        assert torch.equal(gr.grids, _recount(gr, length)), f"after round {i} a grid does not hold exactly the cloud"
    assert int(gr.length.item()) > n0 + 10
    pts, col = gr.result()
    _check_final(g, pts.cpu().numpy(), col.cpu().numpy())


def test_growth_in_one_graph_reads_nothing(g):
    """the 12 rounds captured in one graph: a host read during capture would fail it"""
    gr, slot = _grower(g)
    draws = [_draw(g, i) for i in range(int(g["grow/rounds"]))]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for ref, src, _, si, nz in draws:
            gr.round(slot[ref], slot[src], si, nz)
    graph.replay()
    torch.cuda.synchronize()
    pts, col = gr.result()
    _check_final(g, pts.cpu().numpy(), col.cpu().numpy())


def test_growth_with_a_small_capacity_grows_and_gives_the_same(g):
    from binocular3dgs_amd import matcher_cloud as mc
    refs = g["grow/ref_indices"].tolist()
    draws = [(g[f"grow/{i}/views"][0], g[f"grow/{i}/views"][1], g[f"grow/{i}/seed_idx"], g[f"grow/{i}/noise"]) for i in range(int(g["grow/rounds"]))]
    n0 = len(g["grow/start_points"])
    gr, slot = _grower(g, capacity=n0 + 7)
    for ref, src, si, nz in draws:
        gr.round(slot[int(ref)], slot[int(src)], torch.from_numpy(si).to(DEV, torch.int32), torch.from_numpy(nz).to(DEV))
    with pytest.raises(mc.CloudOverflow) as e:
        gr.result()
    assert e.value.needed == len(g["grow/points"])
    pts, col = mc.grow_cloud(torch.from_numpy(g["grow/start_points"]).to(DEV), torch.from_numpy(g["grow/start_colors"]).to(DEV),
                             list(g["scene/images"]), g["scene/K"], g["scene/c2ws"], refs, draws=draws, capacity=n0 + 7)
    _check_final(g, pts.cpu().numpy(), col.cpu().numpy())


def test_build_cloud_cli_scene_and_three_training_iterations(tmp_path, monkeypatch):
    from binocular3dgs_amd import keypoints_to_3d, train
    from binocular3dgs_amd import matcher_cloud as mc
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    views = mc.read_views(str(src), 1)
    refs = mc.select_views(len(views.names), "LLFF", 3)
    rng = np.random.default_rng(3)
    matches = {}
    for r, s in mc.view_pairs(refs)[:-1]:                                        # the last pair has no matches: skipped
        X = rng.normal(0, 0.5, (160, 3)) + np.array([0, 0, 4.0])
        a, b = mc.match_keys(views.names[r], views.names[s])
        matches[a] = cloud_ref.project_f64(X, views.intrinsics[0], views.c2ws[r]).astype(np.float32)
        matches[b] = cloud_ref.project_f64(X, views.intrinsics[0], views.c2ws[s]).astype(np.float32)
    np.savez(tmp_path / "matches.npz", **matches)
    monkeypatch.chdir(tmp_path)
    assert keypoints_to_3d.main(["--data_path", str(src), "--matches", str(tmp_path / "matches.npz"), "--resolution", "1", "--output_path",
                                 "keypoints_to_3d/LLFF", "--iterations", "4", "--seed", "1"]) == 0
    ply = tmp_path / "keypoints_to_3d" / "LLFF" / "scene_llff_keypoints_to_3d.ply"
    assert ply.exists()
    xyz, rgb = mc.build_cloud(str(src), matches, dataset_name="LLFF", n_views=3, resolution=1, iterations=0)
    assert 100 < len(xyz) <= 5 * 160 and rgb.dtype == np.uint8 and xyz.dtype == np.float32
    scene = Scene.from_dataset(str(src), GaussianModel(1), n_views=3, dataset_name="LLFF", init_points="matcher", resolution=1)
    assert scene.gaussians.get_xyz.shape[0] >= len(xyz)
    args = train.parser().parse_args(["-s", str(src), "-m", str(tmp_path / "out"), "--eval", "--init_points", "matcher", "--iterations", "3",
                                      "--quiet"])
    res = train.run(args)
    assert res["iterations"] == 3 and np.isfinite(res["loss"]) and res["points"] > 0
