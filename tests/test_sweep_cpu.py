"""CPU: the plane-sweep matcher's yardstick on golden G16 (tests/golden/sweep.npz), the host rules of
binocular3dgs_amd/sweep_matcher.py and the command lines, and the argument checks of the two new entry points, which return
before the first HIP call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as sr  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "sweep.npz"))


def test_the_restatement_meets_the_makers_conditions_on_the_stored_scene(g):
    """(a)-(d) from the stored arrays, and the stored arrays of one pair from the restatement itself"""
    tot = dict(nodes=0, ties=0, returned=0, off=0, eligible=0, eligible_returned=0, striped=0, striped_returned=0)
    dirs = [(a, b) for x, y in g["pairs"].tolist() for a, b in ((x, y), (y, x))]
    assert len(dirs) == 6
    for a, b in dirs:
        t = f"dir/{a}_{b}/"
        keep = g[t + "keep"]
        tot["nodes"] += len(keep)
        tot["ties"] += int(g[t + "near_tie"].sum())
        tot["returned"] += int(keep.sum())
        tot["off"] += int((np.linalg.norm(g[t + "q"] - g[t + "true_q"], axis=1)[keep] > 1.0).sum())
        tot["eligible"] += int(g[t + "eligible"].sum())
        tot["eligible_returned"] += int((g[t + "eligible"] & keep).sum())
        tot["striped"] += int(g[t + "striped"].sum())
        tot["striped_returned"] += int((g[t + "striped"] & keep).sum())
    assert tot["ties"] < 0.02 * tot["nodes"]                                       # (a)
    assert tot["off"] < 0.05 * tot["returned"]                                     # (b)
    assert tot["eligible_returned"] >= 0.5 * tot["eligible"] > 0                   # (c)
    assert tot["striped"] > 100 and tot["striped_returned"] == 0                   # (d)
    assert 0 < 4 * float(g["err32"]) < sr.NEAR_TIE                                 # (e)
    imgs, K, c2ws = g["images"], g["K"], g["c2ws"]
    p = sr.Params(stride=int(g["stride"]), hypotheses=int(g["hypotheses"]))
    r = sr.match_pair(imgs[0], imgs[1], K, np.linalg.inv(c2ws[0]), np.linalg.inv(c2ws[1]), float(g["near"]), float(g["far"]), p)
    for d, t in enumerate(("dir/0_1/", "dir/1_0/")):
        assert np.array_equal(r.dirs[d].keep, g[t + "keep"]) and np.array_equal(r.sel[d].k, g[t + "k"])
        assert np.array_equal(r.sel[d].invd, g[t + "invd"]) and np.array_equal(r.dirs[d].q, g[t + "q"], equal_nan=True)
    sc = sr.make_scene()
    assert np.array_equal(sr.render(sc, 2), imgs[2]) and np.array_equal(sc.c2ws, c2ws)


def test_the_gray_is_the_integer_luma():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (5, 6, 3)).astype(np.uint8)
    img[0, 0], img[0, 1] = 255, 0
    want = np.floor((77.0 * img[..., 0] + 150.0 * img[..., 1] + 29.0 * img[..., 2] + 128.0) / 256.0)
    assert np.array_equal(sr.gray(img), want.astype(np.uint8)) and sr.gray(img)[0, 0] == 255


def test_the_library_plans_the_homographies_the_yardstick_plans(g):
    from binocular3dgs_amd import sweep_matcher as sm
    K, c2ws = g["K"], g["c2ws"]
    got = sm.pair_plan(K, c2ws[0], c2ws[2], 1.6, 6.5, 32)
    for d, (a, b) in enumerate(((0, 2), (2, 0))):
        want = sr.plan(K, np.linalg.inv(c2ws[a]), np.linalg.inv(c2ws[b]), 1.6, 6.5, 32)
        assert np.array_equal(got.homographies[d], want.homographies) and np.array_equal(got.proj[d], want.proj)
        assert got.inv_far == float(want.inv_far) and got.step == float(want.step)
    assert got.homographies.dtype == np.float32 and got.homographies.shape == (2, 32, 3, 3)
    # a point of depth 1 / invd[k] in a lands where H_k sends its pixel
    k, p = 7, np.array([40.0, 30.0, 1.0])
    z = 1.0 / (got.inv_far + got.step * k)
    X = np.linalg.inv(c2ws[2]) @ c2ws[0] @ np.append(np.linalg.inv(K) @ p * z, 1.0)
    q = K @ X[:3]
    h = got.homographies[0, k].astype(np.float64) @ p
    assert np.allclose(h[:2] / h[2], q[:2] / q[2], atol=1e-3)
    assert sm.node_count(96, 72, 2) == 45 * 33 and sm.node_count(7, 7, 3) == 1 and sm.node_count(50, 37, 3) == 15 * 11
    with pytest.raises(ValueError):
        sm.pair_plan(K, c2ws[0], c2ws[1], 3.0, 2.0, 32)
    with pytest.raises(ValueError):
        sm.pair_plan(K, c2ws[0], c2ws[1], 1.0, 2.0, 1)
    assert sm.SweepParams() == (2, 128, 0.8, 0.05, 4.0, 1.5, None, None)


def test_matches_round_trip_through_the_file_the_cloud_reads(tmp_path):
    from binocular3dgs_amd import matcher_cloud as mc, sweep_matcher as sm
    a = np.arange(12, dtype=np.float32).reshape(6, 2)
    ka, kb = mc.match_keys("IMG_001.png", "IMG_002.png"), mc.match_keys("IMG_002.png", "IMG_001.png")
    m = {ka[0]: a, ka[1]: a + 0.25, kb[0]: np.zeros((0, 2), np.float32), kb[1]: np.zeros((0,), np.float32)}
    path = str(tmp_path / "sub" / "m.npz")
    sm.write_matches(path, m)
    assert os.path.exists(path)
    back = mc.load_matches(path)
    assert sorted(back) == sorted(m)
    assert np.array_equal(back[ka[0]], a) and np.array_equal(back[ka[1]], a + 0.25)
    assert back[kb[0]].shape == (0, 2) and back[kb[1]].shape == (0, 2)
    assert mc.pair_matches(back, "IMG_002.png", "IMG_001.png") is None and mc.pair_matches(back, "IMG_001.png", "IMG_002.png") is not None


def _folder(tmp_path, points):
    root = tmp_path / "scene"
    os.makedirs(root / "sparse" / "0")
    (root / "sparse" / "0" / "cameras.txt").write_text("1 PINHOLE 96 72 100.0 100.0 47.5 35.5\n")
    (root / "sparse" / "0" / "images.txt").write_text("".join(f"{i + 1} 1 0 0 0 {-0.3 * i} 0 0 1 view_{i}.png\n\n" for i in range(4)))
    if points is not None:
        (root / "sparse" / "0" / "points3D.txt").write_text("".join(f"{i + 1} {x} {y} {z} 9 9 9 0.1\n" for i, (x, y, z) in enumerate(points)))
    return str(root)


def test_depth_range_of_a_folder_with_points_and_without(tmp_path):
    from binocular3dgs_amd import matcher_cloud as mc, sweep_matcher as sm
    depths = np.linspace(2.0, 6.0, 201)
    folder = _folder(tmp_path, [(0.1, -0.2, z) for z in depths] + [(0.0, 0.0, -3.0)])     # one point behind the cameras
    views = mc.read_views(folder, 1)
    near, far = sm.depth_range(folder, views, [0, 1, 2])
    assert near == pytest.approx(0.8 * np.percentile(depths, 1)) and far == pytest.approx(1.2 * np.percentile(depths, 99))
    assert sm.resolve_range(folder, views, [0, 1, 2], sm.SweepParams(near=1.0, far=9.0)) == (1.0, 9.0)
    assert sm.resolve_range(folder, views, [0, 1, 2], sm.SweepParams(far=9.0)) == (near, 9.0)
    empty = _folder(tmp_path / "other", None)
    with pytest.raises(ValueError, match="--near/--far"):
        sm.depth_range(empty, mc.read_views(empty, 1), [0, 1, 2])
    assert sm.resolve_range(empty, views, [0, 1, 2], sm.SweepParams(near=1.0, far=9.0)) == (1.0, 9.0)


def test_command_lines():
    from binocular3dgs_amd import keypoints_to_3d as k, match
    with pytest.raises(SystemExit):
        k.parser().parse_args(["--data_path", "d/fern"])                           # --matcher file (the default) needs --matches
    with pytest.raises(SystemExit):
        k.parser().parse_args(["--data_path", "d/fern", "--matcher", "file"])
    with pytest.raises(SystemExit):
        k.parser().parse_args(["--data_path", "d/fern", "--matcher", "sweep", "--matches", "m.npz"])
    a = k.parser().parse_args(["--data_path", "d/fern", "--matches", "m.npz"])
    assert (a.matcher, a.matches, a.save_matches) == ("file", "m.npz", None)
    b = k.parser().parse_args(["--data_path", "d/fern", "--matcher", "sweep"])
    assert (b.matcher, b.matches, b.sweep_stride, b.sweep_hypotheses, b.near, b.far, b.min_score) == ("sweep", None, 2, 128, None, None, 0.8)
    assert k.sweep_params(b) == (2, 128, 0.8, 0.05, 4.0, 1.5, None, None)
    c = k.parser().parse_args(["--data_path", "d/fern", "--matcher", "sweep", "--sweep_stride", "3", "--sweep_hypotheses", "64", "--near", "1.5",
                               "--far", "20", "--min_score", "0.9", "--save_matches", "out.npz"])
    assert k.sweep_params(c) == (3, 64, 0.9, 0.05, 4.0, 1.5, 1.5, 20.0) and c.save_matches == "out.npz"
    m = match.parser().parse_args(["--data_path", "d/fern", "--output", "f.npz", "--sweep_hypotheses", "48"])
    assert (m.output, m.sweep_hypotheses, m.dataset_name, m.n_views, m.resolution) == ("f.npz", 48, "LLFF", 3, 4)
    with pytest.raises(SystemExit):
        match.parser().parse_args(["--data_path", "d/fern"])
    from binocular3dgs_amd.dataset_readers import INIT_POINTS_HELP
    assert "--matcher sweep" in INIT_POINTS_HELP


def test_build_cloud_refuses_contradicting_arguments():
    from binocular3dgs_amd.matcher_cloud import build_cloud
    with pytest.raises(ValueError, match="file"):
        build_cloud("nowhere")
    with pytest.raises(ValueError, match="sweep"):
        build_cloud("nowhere", {}, matcher="sweep")
    with pytest.raises(ValueError, match="matcher"):
        build_cloud("nowhere", {}, matcher="network")


def test_new_entry_points_report_argument_errors_without_touching_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    ERR_ARG = -1
    assert L.b3gs_sweep_workspace_bytes(96, 72, 32, 2) % 256 == 0 and L.b3gs_sweep_workspace_bytes(96, 72, 32, 2) >= 2 * 96 * 72
    assert L.b3gs_sweep_workspace_bytes(6, 72, 32, 2) == 0 and L.b3gs_sweep_workspace_bytes(96, 72, 1, 2) == 0
    assert L.b3gs_sweep_workspace_bytes(96, 72, 32, 0) == 0
    assert L.b3gs_sweep_match_pair(None, None) == ERR_ARG and b"NULL" in L.b3gs_last_error()

    def io(**kw):
        s = _lib.B3gsSweepPair()
        s.W, s.H, s.D, s.stride, s.radius = 96, 72, 32, 2, 3
        s.near, s.far, s.inv_far, s.step, s.min_score, s.margin, s.min_var, s.cyc_steps = 2.0, 6.0, 1 / 6.0, (0.5 - 1 / 6.0) / 31, 0.8, 0.05, 4.0, 1.5
        for f in ("image_a", "image_b", "homographies", "proj", "kp_source", "kp_target", "score", "count", "node_invd", "node_score", "node_k",
                  "workspace"):
            setattr(s, f, 4096)                            # never dereferenced: every check comes before the first launch
        for k, v in kw.items():
            setattr(s, k, v)
        return L.b3gs_sweep_match_pair(C.byref(s), None)

    assert io(D=1) == ERR_ARG and b"hypotheses" in L.b3gs_last_error()
    assert io(near=6.0) == ERR_ARG and io(near=7.0) == ERR_ARG and b"near" in L.b3gs_last_error()
    assert io(near=0.0) == ERR_ARG and io(near=-1.0) == ERR_ARG
    assert io(stride=0) == ERR_ARG and b"stride" in L.b3gs_last_error()
    assert io(W=6, H=6) == ERR_ARG and b"7 x 7" in L.b3gs_last_error()
    assert io(W=96, H=6) == ERR_ARG
    assert io(radius=2) == ERR_ARG and b"7x7" in L.b3gs_last_error()
    for f in ("image_a", "image_b", "homographies", "proj", "kp_source", "kp_target", "score", "count", "node_invd", "workspace"):
        assert io(**{f: None}) == ERR_ARG, f
    assert io(workspace=4100) == ERR_ARG
    assert C.sizeof(_lib.B3gsSweepPair) == 5 * 4 + 8 * 4 + 4 + 12 * 8            # 13 words, padding, 12 pointers


def test_host_tensors_raise():
    import torch
    from binocular3dgs_amd import _C, _lib
    z = torch.zeros
    img = z(72, 96, 3, dtype=torch.uint8)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.sweep_match_pair(img, img, z(2, 32, 3, 3), z(2, 12), 2.0, 6.0, 1 / 6.0, 0.01)
