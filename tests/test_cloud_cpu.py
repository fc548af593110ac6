"""CPU: the host rules of the matcher cloud (binocular3dgs_amd/matcher_cloud.py, keypoints_to_3d.py) against golden G15
(tests/golden/cloud.npz: the statements of the reference's triangulate.py, recorded), and the argument checks of the three new
entry points, which return before the first HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "cloud.npz"))


def test_view_selection_and_pair_order_equal_the_recorded_lists(g):
    from binocular3dgs_amd import matcher_cloud as mc
    cases = g["select/cases"].tolist()
    assert len(cases) >= 6
    for i, case in enumerate(cases):
        name, n_images, n_views = case.split(":")
        refs = mc.select_views(int(n_images), name, int(n_views))
        assert refs == g[f"select/{i}/refs"].tolist(), case
        assert mc.view_pairs(refs) == [tuple(p) for p in g[f"select/{i}/pairs"].tolist()], case
    with pytest.raises(NotImplementedError):
        mc.select_views(10, "Blender", 3)


def test_every_pair_uses_the_intrinsic_matrix_of_camera_zero():
    from binocular3dgs_amd import matcher_cloud as mc
    views = mc.read_views(os.path.join(GOLD, "scene_llff"), resolution=2)
    assert (views.width, views.height) == (16, 12) and len(views.names) == 10
    # image ids order the views (IMG_003 has id 1), and one camera is SIMPLE_PINHOLE with another focal length
    assert views.names[0] == "IMG_003.png" and views.names[1] == "IMG_000.png"
    assert len({tuple(k.ravel()) for k in views.intrinsics}) == 2
    simple = views.names.index("IMG_004.png")
    assert np.array_equal(views.intrinsics[simple], np.array([[29.5 / 2, 0, 8], [0, 29.5 / 2, 6], [0, 0, 1]], np.float32))
    assert np.array_equal(views.intrinsics[0], np.array([[15, 0, 8], [0, 15.5, 6], [0, 0, 1]], np.float32))
    refs = [0, simple, 8]
    plan = mc.plan_pairs(views, refs)
    assert [(r, s) for r, s, _, _ in plan] == mc.view_pairs(refs)
    for r, s, a, b in plan:
        assert np.array_equal(a.intrinsic, views.intrinsics[0]) and np.array_equal(b.intrinsic, views.intrinsics[0])
        assert np.array_equal(a.c2w, views.c2ws[r]) and np.array_equal(b.c2w, views.c2ws[s])


def test_window_table_equals_the_recorded_one(g):
    from binocular3dgs_amd.matcher_cloud import ssim_window
    w = ssim_window()
    assert w.dtype == torch.float32 and w.shape == (121,)
    assert (w.numpy() == g["window"]).all()


def test_matches_file_parsing(tmp_path):
    from binocular3dgs_amd import matcher_cloud as mc
    a = np.arange(10, dtype=np.float64).reshape(5, 2)
    path = tmp_path / "m.npz"
    np.savez(path, kp_IMG_001_IMG_002_source=a, kp_IMG_001_IMG_002_target=a + 1, kp_IMG_002_IMG_001_source=np.zeros((0, 2)),
             kp_IMG_002_IMG_001_target=np.zeros((0, 2)), other=np.ones(3))
    m = mc.load_matches(str(path))
    assert sorted(m) == ["kp_IMG_001_IMG_002_source", "kp_IMG_001_IMG_002_target", "kp_IMG_002_IMG_001_source", "kp_IMG_002_IMG_001_target"]
    assert all(v.dtype == np.float32 for v in m.values())
    assert mc.match_keys("dir/IMG_001.png", "IMG_002.v2.jpg") == ("kp_IMG_001_IMG_002_source", "kp_IMG_001_IMG_002_target")
    k0, k1 = mc.pair_matches(m, "IMG_001.png", "IMG_002.png")
    assert np.array_equal(k0, a.astype(np.float32)) and np.array_equal(k1, (a + 1).astype(np.float32))
    assert mc.pair_matches(m, "IMG_002.png", "IMG_001.png") is None          # empty: skipped
    assert mc.pair_matches(m, "IMG_001.png", "IMG_003.png") is None          # missing: skipped
    with pytest.raises(ValueError, match="_target"):
        mc.load_matches({"kp_a_b_source": a})
    with pytest.raises(ValueError, match=r"\[N, 2\]"):
        mc.load_matches({"kp_a_b_source": np.zeros((4, 3)), "kp_a_b_target": np.zeros((4, 3))})


def test_cloud_ply_round_trip(tmp_path):
    from binocular3dgs_amd.init_points import fetch_point_cloud, read_ply_vertices
    from binocular3dgs_amd.matcher_cloud import write_cloud_ply
    rng = np.random.default_rng(0)
    xyz, rgb = rng.normal(size=(37, 3)).astype(np.float32), rng.integers(0, 256, (37, 3)).astype(np.uint8)
    path = tmp_path / "keypoints_to_3d" / "LLFF" / "x_keypoints_to_3d.ply"
    write_cloud_ply(str(path), xyz, rgb)
    assert read_ply_vertices(str(path)).dtype.names == ("x", "y", "z", "red", "green", "blue")
    pts, col = fetch_point_cloud(str(path))[:2]
    assert np.array_equal(pts, xyz) and np.array_equal(col, rgb.astype(np.float32) / 255.0)
    with pytest.raises(ValueError):
        write_cloud_ply(str(path), xyz, rgb[:5])


def test_default_draws_follow_the_recorded_order(g):
    from binocular3dgs_amd.matcher_cloud import default_draws
    refs = g["grow/ref_indices"].tolist()
    n_start = len(g["grow/start_points"])
    rec = g["order/draws"]
    n_seeds, n_samples = rec.shape[1] - 2, g["grow/0/noise"].shape[1]
    torch.manual_seed(int(g["order/seed"]))
    got = list(default_draws(refs, n_start, 3, n_seeds, n_samples, "cpu"))
    assert len(got) == 3
    for (ref, src, seed_idx, noise), want in zip(got, rec):
        assert [ref, src] == want[:2].tolist() and seed_idx.tolist() == want[2:].tolist()
        assert noise.shape == (n_seeds, n_samples, 3)


def test_cli_parser_and_output_file():
    from binocular3dgs_amd import keypoints_to_3d as k
    a = k.parser().parse_args(["--data_path", "/data/nerf_llff_data/fern", "--matches", "m.npz"])
    assert (a.dataset_name, a.n_views, a.resolution, a.output_path, a.seed, a.iterations) == ("LLFF", 3, 4, "keypoints_to_3d", 0, 1000)
    assert a.dtu_sparse_indices == [25, 22, 28, 40, 44, 48, 0, 8, 13]
    assert k.output_file(a) == os.path.join("keypoints_to_3d", "fern_keypoints_to_3d.ply")
    b = k.parser().parse_args(["--data_path", "d/scan5/", "--matches", "m.npz", "--dataset_name", "DTU", "--output_path", "keypoints_to_3d/DTU",
                               "--n_views", "6", "--resolution", "1", "--seed", "3"])
    assert k.output_file(b) == "keypoints_to_3d/DTU/scan5_keypoints_to_3d.ply" and (b.n_views, b.resolution, b.seed) == (6, 1, 3)
    from binocular3dgs_amd.dataset_readers import matcher_ply_path
    assert k.output_file(b) == matcher_ply_path("d/scan5", "DTU", None)
    with pytest.raises(SystemExit):
        k.parser().parse_args(["--matches", "m.npz"])


def test_help_text_points_at_the_new_command():
    from binocular3dgs_amd.dataset_readers import INIT_POINTS_HELP
    assert "binocular3dgs_amd.keypoints_to_3d" in INIT_POINTS_HELP


def test_grid_margin_is_one_cell():
    from binocular3dgs_amd.matcher_cloud import grid_margin
    for wh in ((2, 2), (64, 48), (504, 378), (4032, 3024)):
        assert grid_margin(*wh) == 1
    with pytest.raises(ValueError):
        grid_margin(1, 5)


def test_new_entry_points_report_argument_errors_without_touching_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    ERR_ARG = -1
    assert L.b3gs_cloud_workspace_bytes(0) >= 256 and L.b3gs_cloud_workspace_bytes(-1) == 0
    assert L.b3gs_cloud_workspace_bytes(20000) % 256 == 0 and L.b3gs_cloud_workspace_bytes(20000) >= 20000 * 17
    p = C.c_void_p(4096)                                   # never dereferenced: every check comes before the first launch
    tri = lambda N, W, H, thr, ws, img=p: L.b3gs_triangulate_matches(N, p, p, p, p, p, p, p, img, W, H, thr, p, p, p, ws, None)  # noqa: E731
    assert tri(-1, 64, 48, 2.0, p) == ERR_ARG
    assert tri(10, 1, 48, 2.0, p) == ERR_ARG and b"2 x 2" in L.b3gs_last_error()
    assert tri(10, 64, 48, 0.0, p) == ERR_ARG
    assert tri(10, 64, 48, 2.0, None) == ERR_ARG and b"workspace" in L.b3gs_last_error()
    assert tri(10, 64, 48, 2.0, C.c_void_p(4100)) == ERR_ARG
    assert tri(10, 64, 48, 2.0, p, None) == ERR_ARG
    assert L.b3gs_background_sheet(None, 64, 48, p, p, 10.0, p, p, p, p, None) == ERR_ARG
    assert L.b3gs_background_sheet(p, 64, 1, p, p, 10.0, p, p, p, p, None) == ERR_ARG
    assert L.b3gs_background_sheet(p, 64, 48, p, p, -1.0, p, p, p, p, None) == ERR_ARG
    assert L.b3gs_background_sheet(p, 64, 48, p, p, 10.0, p, p, p, None, None) == ERR_ARG
    assert L.b3gs_cloud_grow_round(None, None) == ERR_ARG

    def io(**kw):
        s = _lib.B3gsCloudGrow()
        s.W, s.H, s.n_views, s.ref, s.src, s.n_seeds, s.n_samples, s.n_start, s.h_patch_size = 64, 48, 3, 0, 1, 16, 32, 100, 5
        s.capacity, s.ssim_threshold, s.alpha = 200, 0.95, 10.0
        for f in ("images", "w2c", "window", "seed_idx", "noise", "points", "colors", "length", "overflow", "grids", "workspace"):
            setattr(s, f, 4096)
        for k, v in kw.items():
            setattr(s, k, v)
        return L.b3gs_cloud_grow_round(C.byref(s), None)

    assert io(h_patch_size=3) == ERR_ARG and b"11x11" in L.b3gs_last_error()
    assert io(src=0) == ERR_ARG and io(ref=3) == ERR_ARG and io(n_views=1) == ERR_ARG and io(n_views=17) == ERR_ARG
    assert io(capacity=50) == ERR_ARG and io(n_start=0) == ERR_ARG and io(n_seeds=0) == ERR_ARG
    assert io(grids=None) == ERR_ARG and io(workspace=None) == ERR_ARG and io(workspace=4100) == ERR_ARG and io(W=1) == ERR_ARG
    assert C.sizeof(_lib.B3gsCloudGrow) == 10 * 4 + 6 * 4 + 7 * 8 + 8 + 6 * 8


def test_host_tensors_raise():
    from binocular3dgs_amd import _C, _lib
    from binocular3dgs_amd import matcher_cloud as mc
    z = torch.zeros
    img = z(48, 64, 3, dtype=torch.uint8)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.triangulate_matches(z(3, 4), z(3, 4), z(3, 3), z(4, 4), z(4, 4), z(5, 2), z(5, 2), img, 2.0)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.background_sheet(img, z(3, 3), z(4, 4), 10.0)
    i32 = lambda *s: z(*s, dtype=torch.int32)  # noqa: E731
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.cloud_grow_round(z(3, 48, 64, 3, dtype=torch.uint8), z(3, 4, 4), z(121), i32(16), z(16, 32, 3), z(200, 3), z(200, 3), i32(1), i32(1),
                            i32(3, 50, 66), 0, 1, 100, 5, True, 64.0, 64.0, 32.0, 24.0)
    cam = mc.PinholeView(np.eye(3, dtype=np.float32), np.eye(4, dtype=np.float32))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mc.triangulate_pair(cam, cam, np.zeros((5, 2), np.float32), np.zeros((5, 2), np.float32), img)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mc.background_sheet(img, np.eye(3), np.eye(4))
