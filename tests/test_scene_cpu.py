"""Dataset loading on the host against golden G14 (tests/golden/scene_prep.npz, recorded from the reference's readers, loadCam
and the DTU statements of its train.py): COLMAP / Blender readers and splits, the PNG reader, the output-size rule, the resize
coefficient tables and their numpy restatement, the 49-row rule, cfg_args, and the DTU branch of IterationSchedule."""
import json
import os
import struct
import sys
import types
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "scene_prep.npz"))


def _copy(src, dst):
    import shutil
    shutil.copytree(src, dst)
    return str(dst)


SCENES = (("llff_n3", "scene_llff", dict(eval=True, n_views=3, dataset_name="LLFF")),
          ("llff_n0", "scene_llff", dict(eval=True, n_views=0, dataset_name="LLFF")),
          ("llff_txt_n3", "scene_llff_txt", dict(eval=True, n_views=3, dataset_name="LLFF")),
          ("dtu_n3", os.path.join("scene_dtu", "scan5"), dict(eval=True, n_views=3, dataset_name="DTU")),
          ("blender_n3", "scene_blender", dict(eval=True, n_views=3, dataset_name="Blender")),
          ("blender_all", "scene_blender", dict(eval=False, n_views=3, dataset_name="Blender")))


@pytest.mark.parametrize("tag,folder,kw", SCENES)
def test_readers_match_the_recorded_scene(g, tmp_path, tag, folder, kw):
    from binocular3dgs_amd import dataset_readers as dr
    src = _copy(os.path.join(GOLD, folder), tmp_path / os.path.basename(folder))
    if tag.startswith("blender"):
        np.random.seed(0)
    si = dr.read_scene(src, init_points="sparse", **kw)
    assert [c.image_name for c in si.train_cameras] == list(g[f"scene/{tag}/train"])
    assert [c.image_name for c in si.test_cameras] == list(g[f"scene/{tag}/test"])
    cams = {c.image_name: c for c in si.train_cameras + si.test_cameras}
    names = sorted(cams)
    assert names == list(g[f"scene/{tag}/names"])
    for key, fn in (("R", lambda c: c.R), ("T", lambda c: c.T), ("fov", lambda c: [c.FovX, c.FovY]),
                    ("wh", lambda c: [c.width, c.height]), ("uid", lambda c: c.uid)):
        got = np.array([fn(cams[n]) for n in names])
        assert got.dtype == g[f"scene/{tag}/{key}"].dtype and np.array_equal(got, g[f"scene/{tag}/{key}"]), key   # the same bits
    assert np.array_equal(np.array(si.radius), g[f"scene/{tag}/radius"])
    assert np.array_equal(si.translate, g[f"scene/{tag}/translate"])
    entries = [dr.camera_json(i, c) for i, c in enumerate(si.test_cameras + si.train_cameras)]
    assert json.loads(json.dumps(entries)) == json.loads(str(g[f"scene/{tag}/cameras_json"]))
    # the point cloud: COLMAP's points converted once to points3D.ply, which later runs read; Blender: seeded random points
    assert os.path.exists(si.ply_path) and si.points.dtype == np.float32 and si.points.shape[1] == 3
    if tag.startswith("blender"):
        assert si.points.shape[0] == 100_000 and np.abs(si.points).max() <= 1.3
    else:
        assert si.ply_path.endswith("sparse/0/points3D.ply")
        rule = dr.matcher_ply_path(os.path.join(GOLD, folder), kw["dataset_name"], None)
        if kw["n_views"] > 0:
            assert rule == str(g[f"scene/{tag}/ply_path"])


def test_initial_points_errors_and_other_datasets(tmp_path):
    from binocular3dgs_amd import dataset_readers as dr
    src = _copy(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    with pytest.raises(FileNotFoundError, match="matcher.*sparse.*path"):
        dr.read_scene(src, eval=True, n_views=3, init_points="matcher")
    with pytest.raises(FileNotFoundError, match="matcher.*sparse.*path"):
        dr.read_scene(src, eval=True, n_views=3, init_points=str(tmp_path / "nothing.ply"))
    with pytest.raises(NotImplementedError):
        dr.read_scene(src, eval=True, n_views=3, dataset_name="MipNeRF360", init_points="sparse")
    si = dr.read_scene(src, eval=True, n_views=3, init_points="sparse")
    xyz, rgb = dr.read_points3d_bin(os.path.join(src, "sparse/0/points3D.bin"))
    assert np.array_equal(si.points, xyz.astype(np.float32)) and np.array_equal(si.colors, rgb.astype(np.float32) / 255.0)
    # a camera model with distortion is refused by name
    with open(os.path.join(src, "sparse/0/cameras.bin"), "wb") as fp:
        fp.write(struct.pack("<Q", 2) + struct.pack("<iiQQ", 1, 2, 32, 24) + struct.pack("<dddd", 30, 16, 12, 0.1)
                 + struct.pack("<iiQQ", 2, 0, 32, 24) + struct.pack("<ddd", 30, 16, 12))
    with pytest.raises(ValueError, match="SIMPLE_RADIAL"):
        dr.read_scene(src, eval=False, init_points="sparse")


def _png(a, ctype, filters):
    """A PNG of `a` [H, W, C] with the given filter type per row, built by hand"""
    from binocular3dgs_amd.frames import _chunk
    H, W, C = a.shape
    flat = a.reshape(H, W * C).astype(np.int64)
    rows = b""
    for y in range(H):
        f = filters[y % len(filters)]
        cur, up = flat[y], flat[y - 1] if y else np.zeros(W * C, dtype=np.int64)
        left = np.concatenate([np.zeros(C, dtype=np.int64), cur[:-C]])
        ul = np.concatenate([np.zeros(C, dtype=np.int64), up[:-C]])
        if f == 0:
            pred = 0
        elif f == 1:
            pred = left
        elif f == 2:
            pred = up
        elif f == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        rows += bytes([f]) + ((cur - pred) % 256).astype(np.uint8).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)) + _chunk(b"tEXt", b"k\x00v")
            + _chunk(b"IDAT", zlib.compress(rows)[:40]) + _chunk(b"IDAT", zlib.compress(rows)[40:]) + _chunk(b"IEND", b""))


@pytest.mark.parametrize("ctype,C", [(0, 1), (4, 2), (2, 3), (6, 4)])
@pytest.mark.parametrize("filters", [(0,), (1,), (2,), (3,), (4,), (4, 3, 1, 2, 0)])
def test_read_png_all_colour_types_and_filters(tmp_path, ctype, C, filters):
    from binocular3dgs_amd.frames import png_size, read_png
    a = np.random.default_rng(ctype * 10 + len(filters) + filters[0]).integers(0, 256, (9, 13, C), dtype=np.uint8)
    path = str(tmp_path / "x.png")
    with open(path, "wb") as fp:
        fp.write(_png(a, ctype, filters))
    got = read_png(path)
    assert got.dtype == np.uint8 and np.array_equal(got, a[..., 0] if C == 1 else a)
    assert tuple(png_size(path)) == (13, 9)


def test_read_png_round_trip_and_refusals(tmp_path):
    from binocular3dgs_amd.frames import _chunk, read_png, write_png
    a = np.random.default_rng(0).integers(0, 256, (24, 32, 3), dtype=np.uint8)
    assert np.array_equal(read_png(write_png(str(tmp_path / "a.png"), a)), a)
    for name, ihdr in (("16-bit", (4, 4, 16, 2, 0, 0, 0)), ("interlaced", (4, 4, 8, 2, 0, 0, 1)), ("palette", (4, 4, 8, 3, 0, 0, 0))):
        p = str(tmp_path / (name + ".png"))
        with open(p, "wb") as fp:
            fp.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", *ihdr)) + _chunk(b"IDAT", zlib.compress(b"\0" * 200))
                     + _chunk(b"IEND", b""))
        with pytest.raises(ValueError, match="8-bit non-interlaced"):
            read_png(p)
    # the fixture images decode to what Pillow sees
    PIL = pytest.importorskip("PIL.Image")
    for rel in ("scene_llff/images/IMG_003.png", "scene_blender/train/r_2.png"):
        p = os.path.join(GOLD, rel)
        assert np.array_equal(read_png(p), np.array(PIL.open(p)))


def test_output_size_rule(g):
    from binocular3dgs_amd.camera_path import render_size
    from binocular3dgs_amd.ground_truth import output_size
    for W0, H0, r, w, h in g["sizes"].tolist():
        assert output_size(W0, H0, r) == (w, h), (W0, H0, r)
    assert render_size(4032, 3024, -1) == (4032, 3024) and render_size(8000, 6000, -1) == (6400, 4800)
    assert render_size(504.0, 378.0, 4) == (126, 94)


def _prep_cases(g):
    for name in g["prep/names"].tolist():
        yield name, g[f"prep/{name}/src"], tuple(int(v) for v in g[f"prep/{name}/size"])


def _gold(g, name, white, key):
    k = f"prep/{name}/w{white}/{key}"
    if k not in g.files and white:
        k = f"prep/{name}/w0/{key}"            # no alpha channel: white_background changes nothing (recorded once)
    return g[k] if k in g.files else None


def test_tables_and_numpy_restatement_match_the_recorded_ground_truth(g):
    from binocular3dgs_amd.ground_truth import DTU_THRESHOLD, DTU_THRESHOLD_SCAN110, resize_table
    seen = 0
    for name, src, (w, h) in _prep_cases(g):
        Hs, Ws = src.shape[:2]
        assert np.array_equal(resize_table(Ws, w), R.table(Ws, w)) and np.array_equal(resize_table(Hs, h), R.table(Hs, h))
        resized = R.resize(src, (w, h))
        for white in (0, 1):
            image, alpha, _ = R.float_statements(resized, bool(white))
            assert np.array_equal(image.numpy(), _gold(g, name, white, "image")), (name, white)      # zero differing values
            ga = _gold(g, name, white, "alpha")
            assert (alpha is None) == (ga is None) and (alpha is None or np.array_equal(alpha.numpy(), ga))
            for tag, thr in (("30", DTU_THRESHOLD), ("15", DTU_THRESHOLD_SCAN110)):
                gb = _gold(g, name, white, "bg" + tag)
                if gb is not None:
                    bg = R.float_statements(resized, bool(white), thr)[2]
                    assert np.array_equal(bg.numpy(), gb.astype(np.float32)), (name, white, tag)
                    seen += 1
    assert seen >= 8
    for a, b in ((4032, 504), (3024, 378), (800, 400), (5, 1), (1, 5), (1601, 1600)):
        assert np.array_equal(resize_table(a, b), R.table(a, b))
        assert 255 * np.abs(resize_table(a, b)[2:].astype(np.int64)).sum(0).max() < 2 ** 31


def test_numpy_restatement_matches_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for (W, H), (w, h), C in (((403, 302), (50, 38), 3), ((127, 99), (63, 49), 4), ((64, 48), (100, 75), 4), ((64, 48), (64, 30), 3),
                              ((64, 48), (64, 48), 4), ((50, 40), (25, 20), 1)):
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        if C == 4:
            a[..., 3] = np.where(rng.random((H, W)) < 0.3, 0, np.where(rng.random((H, W)) < 0.5, 255, a[..., 3]))
        a = a[..., 0] if C == 1 else a
        assert np.array_equal(R.resize(a, (w, h)), np.array(Image.fromarray(a).resize((w, h)))), ((W, H), (w, h), C)


def test_the_49_row_rule(g):
    """The recorded mask of a constant dark column is 1 everywhere; of a dark run of n rows: from its 50th row on (or from
    the top edge); the brightest channel at exactly 30 (15) is not dark."""
    src = g["prep/dtu_same/src"]
    m30, m15 = g["prep/dtu_same/w0/bg30"][0], g["prep/dtu_same/w0/bg15"][0]
    assert m30[:, 0].all() and m30[:, 3].all() and not m30[:, 4].any() and not m30[:, 5].any()      # 14, 29 | 30, 31
    assert m15[:, 0].all() and not m15[:, 1].any() and not m15[:, 2].any()                          # 14 | 15, 16
    assert not m30[:, 14].any()                                       # 40 dark rows: never 50 in a row
    assert m30[79:130, 20].all() and not m30[:79, 20].any() and not m30[130:, 20].any()     # rows 30..129 dark
    assert m30[:55, 26].all() and not m30[55:, 26].any()              # from the top edge: the window is shorter there
    assert m30[54:56, 30].all() and m30[:, 30].sum() == 2 and m30[:, 32].sum() == 1 and m30[:, 34].sum() == 0
    dark = torch.from_numpy(src.max(-1) < 30)[None]
    assert np.array_equal(R.dtu_rows(dark).numpy()[0], m30.astype(bool))


def test_cfg_args_round_trip(tmp_path):
    from binocular3dgs_amd import spiral, train
    a = train.parser().parse_args(["-s", "/data/llff/fern", "-m", str(tmp_path), "--eval", "-r", "8", "--n_views", "3",
                                   "--test_iterations", "10", "20", "--init_points", "sparse"])
    assert (a.iterations, a.shift_cam_start, a.cam_trans_dist, a.opacity_decay_factor, a.sh_degree, a.dataset_name) == \
        (30_000, 20000, 0.4, 0.995, 1, "LLFF") and a.binocular_consistency and a.opacity_decay and not a.white_background
    with open(tmp_path / "cfg_args", "w") as fp:
        fp.write(train.cfg_args_text(a))
    cfg = spiral.read_cfg_args(str(tmp_path))
    assert cfg == vars(a)


def test_schedule_adds_the_bg_mask_term_exactly_when_a_camera_has_one():
    from binocular3dgs_amd.schedule import IterationSchedule
    H, W = 6, 8
    gen = torch.Generator().manual_seed(0)
    alpha = (torch.rand(1, H, W, generator=gen) - 0.3).requires_grad_(True)
    image = torch.rand(3, H, W, generator=gen).requires_grad_(True)
    bg = (torch.rand(1, H, W, generator=gen) < 0.5).float()
    quiet = lambda *a, **k: None    # noqa: E731
    ops = types.SimpleNamespace(render=lambda *a: {"render": image, "rendered_alpha": alpha, "rendered_depth": None,
                                                   "radii": torch.zeros(2), "visibility_filter": torch.zeros(2, dtype=torch.bool),
                                                   "viewspace_points": None},
                                l1_loss=lambda a, b, **k: (a - b).abs().mean(), ssim=lambda a, b: torch.tensor(1.0),
                                SmoothLoss=lambda: None, inverse_warp_images=None)
    model = types.SimpleNamespace(update_learning_rate=quiet, oneupSHdegree=quiet, opacity_decay=quiet, add_densification_stats=quiet,
                                  max_radii2D=torch.zeros(2), optimizer=types.SimpleNamespace(step=quiet, zero_grad=quiet))
    mk = lambda **kw: types.SimpleNamespace(image_height=H, image_width=W, original_image=torch.zeros(3, H, W), **kw)  # noqa: E731
    totals = {}
    for name, cam in (("none", mk()), ("attr_none", mk(gt_alpha_mask=None, bg_mask=None)), ("bg", mk(gt_alpha_mask=None, bg_mask=bg)),
                      ("alpha_wins", mk(gt_alpha_mask=bg, bg_mask=bg))):
        scene = types.SimpleNamespace(getTrainCameras=lambda c=cam: [c], cameras_extent=1.0)
        s = IterationSchedule(model, scene, None, torch.zeros(3), ops=ops, iterations=10, binocular=False, opacity_decay_factor=None,
                              lambda_dssim=0.0, densify_until_iter=0)
        alpha.grad = None
        totals[name] = float(s.run_iteration(1, 0))
        if name == "bg":
            assert torch.equal(alpha.grad, torch.sign(alpha.detach()) * bg / (H * W))
        if name in ("none", "attr_none"):
            assert alpha.grad is None
    base = float(image.detach().abs().mean())
    assert totals["none"] == totals["attr_none"] == pytest.approx(base)
    assert totals["bg"] == pytest.approx(base + float((alpha.detach().abs() * bg).mean()))
    assert totals["alpha_wins"] == pytest.approx(base + float((alpha.detach().abs() * (1 - bg)).mean()))


def test_camera_takes_prepared_tensors_as_they_are():
    from binocular3dgs_amd.camera import Camera
    img, a, bg = torch.full((3, 4, 5), 0.5), torch.full((1, 4, 5), 0.5), torch.ones(1, 4, 5)
    c = Camera(np.eye(3), np.zeros(3), 0.8, 0.6, 5, 4, image=img, gt_alpha_mask=a, prepared=True, image_name="v", colmap_id=7, bg_mask=bg)
    assert torch.equal(c.original_image, img) and c.image_name == "v" and c.colmap_id == 7 and c.bg_mask is bg
    d = Camera(np.eye(3), np.zeros(3), 0.8, 0.6, 5, 4, image=img, gt_alpha_mask=a)
    assert torch.equal(d.original_image, img * a) and d.bg_mask is None and d.image_name is None
