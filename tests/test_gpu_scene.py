"""Ground truth prepared on the device (csrc/gt_prep.hip, _C.prepare_gt), Scene.from_dataset and train.run against golden G14
(tests/golden/scene_prep.npz: the reference's loadCam / Camera / DTU statements) and the numpy restatement of Pillow's resize.
Every comparison of ground truth is torch.equal: the resize is integer work, every float statement one rounded operation."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pil_resize_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "scene_prep.npz"))


def _gold(g, name, white, key):
    k = f"prep/{name}/w{white}/{key}"
    if k not in g.files and white:
        k = f"prep/{name}/w0/{key}"            # no alpha channel: white_background changes nothing (recorded once)
    return g[k] if k in g.files else None


def _prepare(srcs, size, white=False, thr=0.0):
    from binocular3dgs_amd import _C
    from binocular3dgs_amd.ground_truth import device_table
    dev = torch.device("cuda")
    t = [torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in srcs]
    tx = [device_table(s.shape[1], size[0], dev) for s in t]
    ty = [device_table(s.shape[0], size[1], dev) for s in t]
    return _C.prepare_gt(t, tx, ty, size[0], size[1], white, thr)


def test_prepare_gt_equals_the_recorded_reference_output(g):
    from binocular3dgs_amd.ground_truth import DTU_THRESHOLD, DTU_THRESHOLD_SCAN110
    checked = 0
    for name in g["prep/names"].tolist():
        src, size = g[f"prep/{name}/src"], tuple(int(v) for v in g[f"prep/{name}/size"])
        for white in (0, 1):
            for tag, thr in (("", 0.0), ("30", DTU_THRESHOLD), ("15", DTU_THRESHOLD_SCAN110)):
                gb = _gold(g, name, white, "bg" + tag) if tag else None
                if tag and gb is None:
                    continue
                image, alpha, bg = _prepare([src], size, bool(white), thr)[0]
                ref = torch.from_numpy(_gold(g, name, white, "image"))
                print(name, white, tag, "differing values:", int((image.cpu() != ref).sum()))
                assert torch.equal(image.cpu(), ref), (name, white, tag)
                ga = _gold(g, name, white, "alpha")
                assert (alpha is None) == (ga is None)
                if ga is not None:
                    assert torch.equal(alpha.cpu(), torch.from_numpy(ga)), (name, white)
                assert (bg is None) == (gb is None)
                if gb is not None:
                    assert torch.equal(bg.cpu(), torch.from_numpy(gb.astype(np.float32))), (name, white, tag)
                checked += 1
    assert checked >= 30


def _seeded(rng, H, W, C):
    a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if C == 4:
        u = rng.random((H, W))
        a[..., 3] = np.where(u < 0.3, 0, np.where(u < 0.6, 255, a[..., 3]))
    return a


def test_full_size_sources_equal_the_cpu_restatement():
    rng = np.random.default_rng(7)
    a = _seeded(rng, 3024, 4032, 3)
    got = _prepare([a], (504, 378))[0]
    ref = R.ground_truth(a, (504, 378))
    assert torch.equal(got[0].cpu(), ref[0]) and got[1] is None and got[2] is None
    b = _seeded(rng, 800, 800, 4)
    for white in (False, True):
        got = _prepare([b], (400, 400), white, 30 / 255)[0]
        ref = R.ground_truth(b, (400, 400), white, 30 / 255)
        assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1]) and torch.equal(got[2].cpu(), ref[2])


def test_batches_mixed_sizes_and_workspace_independence():
    rng = np.random.default_rng(8)
    shapes = [(240, 320, 3), (120, 161, 4), (60, 80, 1), (90, 120, 3), (60, 80, 4), (333, 444, 3), (60, 81, 4), (61, 80, 3)]
    srcs = [_seeded(rng, *s) for s in shapes]
    srcs[2] = srcs[2][..., 0]
    size = (80, 60)
    batch = _prepare(srcs, size, True, 15 / 255)
    other = _prepare([_seeded(rng, *s) for s in shapes[:5]], size, False, 0.0)      # different contents in the workspace
    again = _prepare(srcs, size, True, 15 / 255)
    del other
    for i, s in enumerate(srcs):
        one = _prepare([s], size, True, 15 / 255)[0]
        ref = R.ground_truth(s, size, True, 15 / 255)
        for k in range(3):
            assert (batch[i][k] is None) == (ref[k] is None) == (one[k] is None)
            if ref[k] is not None:
                assert torch.equal(batch[i][k].cpu(), ref[k]), (i, k)
                assert torch.equal(batch[i][k], one[k]) and torch.equal(batch[i][k], again[i][k]), (i, k)


def test_prepare_ground_truth_host_sources_and_errors():
    from binocular3dgs_amd import _C
    from binocular3dgs_amd.ground_truth import prepare_ground_truth
    rng = np.random.default_rng(9)
    srcs = [_seeded(rng, 48, 64, 3 if i % 2 else 4) for i in range(11)]                # more than one batch, from the host
    out = prepare_ground_truth(iter(srcs), (32, 24), white_background=True)
    assert len(out) == 11
    for s, o in zip(srcs, out):
        ref = R.ground_truth(s, (32, 24), True)
        assert torch.equal(o[0].cpu(), ref[0]) and (o[1] is None) == (ref[1] is None) and o[2] is None
    with pytest.raises(ValueError):
        _C.prepare_gt([torch.zeros(4, 4, 3, dtype=torch.uint8, device="cuda")], [None], [None], 2, 2, False, 0.0)   # tables missing
    with pytest.raises(ValueError):
        _C.prepare_gt([torch.zeros(4, 4, 2, dtype=torch.uint8, device="cuda")], [None], [None], 4, 4, False, 0.0)   # 2 channels


@pytest.mark.parametrize("tag,folder,kw,res,white", [
    ("llff_n3", "scene_llff", dict(eval=True, n_views=3, dataset_name="LLFF"), 2, False),
    ("blender_n3", "scene_blender", dict(eval=True, n_views=3, dataset_name="Blender"), 4, True)])
def test_scene_from_dataset(g, tmp_path, tag, folder, kw, res, white):
    from binocular3dgs_amd.camera import Camera
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    src = shutil.copytree(os.path.join(GOLD, folder), tmp_path / folder)
    out = str(tmp_path / "model")
    model = GaussianModel(1)
    np.random.seed(0)
    scene = Scene.from_dataset(str(src), model, resolution=res, white_background=white, init_points="sparse", model_path=out,
                               shuffle=False, **kw)
    names = g[f"scene/{tag}/names"].tolist()
    assert [c.image_name for c in scene.getTrainCameras()] == g[f"scene/{tag}/train"].tolist()
    assert [c.image_name for c in scene.getTestCameras()] == g[f"scene/{tag}/test"].tolist()
    assert scene.cameras_extent == float(g[f"scene/{tag}/radius"])
    for cam in scene.getTrainCameras() + scene.getTestCameras():
        k = names.index(cam.image_name)
        img = torch.from_numpy(g[f"scene/{tag}/gt/{cam.image_name}/image"])
        ref = Camera(g[f"scene/{tag}/R"][k], g[f"scene/{tag}/T"][k], *g[f"scene/{tag}/fov"][k], img.shape[2], img.shape[1], device="cuda")
        for m in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            assert torch.equal(getattr(cam, m), getattr(ref, m)), m
        assert (cam.image_width, cam.image_height) == (img.shape[2], img.shape[1])
        assert torch.equal(cam.original_image.cpu(), img), cam.image_name
        ak = f"scene/{tag}/gt/{cam.image_name}/alpha"
        assert (cam.gt_alpha_mask is None) == (ak not in g.files)
        if ak in g.files:
            assert torch.equal(cam.gt_alpha_mask.cpu(), torch.from_numpy(g[ak]))
        assert cam.bg_mask is None and cam.colmap_id == int(g[f"scene/{tag}/uid"][k])
    with open(os.path.join(out, "cameras.json")) as fp:
        assert json.load(fp) == json.loads(str(g[f"scene/{tag}/cameras_json"]))
    with open(os.path.join(out, "input.ply"), "rb") as a, open(scene.scene_info.ply_path, "rb") as b:
        assert a.read() == b.read()
    assert model.get_xyz.shape[0] == scene.scene_info.points.shape[0] and model.get_xyz.is_cuda


def _train_args(src, out, extra=()):
    from binocular3dgs_amd import train
    return train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "60",
                                      "--shift_cam_start", "20", "--densify_from_iter", "10", "--densification_interval", "10",
                                      "--test_iterations", "40", "--save_iterations", "40", "--checkpoint_iterations", "40",
                                      "--quiet", *extra])


def test_train_end_to_end_resume_and_consumers(tmp_path):
    from binocular3dgs_amd import evaluate, spiral, train
    from binocular3dgs_amd.gaussian_model import GaussianModel
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "out"
    res = train.run(_train_args(src, out))
    assert res["first_iteration"] == 1 and res["iterations"] == 60 and np.isfinite(res["loss"]) and res["points"] > 0
    assert set(res["reports"]) == {40} and set(res["reports"][40]) == {"test", "train"}
    assert all(np.isfinite(v) for pair in res["reports"][40].values() for v in pair)
    for rel in ("cfg_args", "input.ply", "cameras.json", "point_cloud/iteration_40/point_cloud.ply",
                "point_cloud/iteration_60/point_cloud.ply", "chkpnt40.pth"):
        assert os.path.exists(out / rel), rel
    cfg = spiral.read_cfg_args(str(out))
    assert cfg["source_path"] == str(src) and cfg["n_views"] == 3 and cfg["init_points"] == "sparse"
    # resume: continues at 41
    out2 = tmp_path / "out2"
    res2 = train.run(_train_args(src, out2, ("--start_checkpoint", str(out / "chkpnt40.pth"))))
    assert res2["first_iteration"] == 41 and np.isfinite(res2["loss"])
    assert os.path.exists(out2 / "point_cloud/iteration_60/point_cloud.ply") and not os.path.exists(out2 / "point_cloud/iteration_40")
    # the saved model is what the other entry points read, without further arguments
    frames_dir = spiral.run(str(out), n_frames=8)
    assert len([f for f in os.listdir(frames_dir) if f.endswith(".png")]) == 24
    model = GaussianModel(1)
    model.load_ply(str(out / "point_cloud/iteration_60/point_cloud.ply"))
    assert model.get_xyz.shape[0] == res["points"]
    cams = res["scene"].getTestCameras()
    bg = torch.zeros(3, device="cuda")
    per_view = evaluate.evaluate_views(model, cams, bg, mode="png")["per_view"]
    written = evaluate.write_results(str(out), "ours_60", per_view, [c.image_name for c in cams])
    assert os.path.exists(out / "results.json") and np.isfinite(written["results"]["ours_60"]["PSNR"])


def test_train_on_a_dtu_scene_drives_the_background_mask(tmp_path):
    from binocular3dgs_amd import train
    from binocular3dgs_amd.render import PipelineParams, render
    src = shutil.copytree(os.path.join(GOLD, "scene_dtu", "scan5"), tmp_path / "scan5")
    res = train.run(_train_args(src, tmp_path / "out", ("--dataset_name", "DTU", "-r", "1")))
    assert np.isfinite(res["loss"])
    scene, model = res["scene"], res["model"]
    assert len(scene.getTrainCameras()) == 3 and len(scene.getTestCameras()) == 25
    cam = scene.getTrainCameras()[0]
    assert cam.bg_mask is not None and cam.bg_mask.shape == (1, 6, 8) and cam.gt_alpha_mask is None
    from binocular3dgs_amd.frames import read_png
    ref = R.float_statements(read_png(os.path.join(src, "images", cam.image_name + ".png")), False, 30 / 255)
    assert torch.equal(cam.original_image.cpu(), ref[0]) and torch.equal(cam.bg_mask.cpu(), ref[2])
    assert cam.bg_mask.sum() > 0                                            # the fixture's dark left border
    # the coverage term reaches the alpha channel where the mask is 1
    pkg = render(cam, model, PipelineParams(), torch.zeros(3, device="cuda"))
    alpha = pkg["rendered_alpha"]
    alpha.retain_grad()
    ((alpha.abs() * cam.bg_mask).mean()).backward()
    assert (alpha.grad[cam.bg_mask > 0] != 0).any() and (alpha.grad[cam.bg_mask == 0] == 0).all()
