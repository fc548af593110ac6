"""CPU: evaluate.training_report against the reference's own training_report (golden G12, tests/golden/eval_metrics.npz):
camera selection (3 train views -> 2,1,0,2,1), the skipped empty test config, the clamp and the float64 averaging, driven
with stand-in renders and the PyTorch statements of loss.py.  write_results: the reference's results.json / per_view.json
layout without LPIPS.  The optional report hook of IterationSchedule."""
import json
import os
import types

import numpy as np
import pytest
import torch

from binocular3dgs_amd import evaluate, loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))


def _views(img, gt, base):
    return [types.SimpleNamespace(uid=base + i, original_image=torch.from_numpy(gt[i]), _render=torch.from_numpy(img[i]))
            for i in range(len(img))]


def _cpu_statements(image, gt):
    # train.py:246-247 with loss.py's copies of utils/loss_utils.l1_loss and utils/image_utils.psnr
    return loss.l1_loss(image, gt).mean().double(), loss.psnr(image, gt).mean().double()


def _report(train, test):
    seen = []

    def render_fn(cams):
        seen.append([c.uid for c in cams])
        return [c._render for c in cams]
    res = evaluate.training_report(None, test, train, None, render_fn=render_fn, view_metrics=_cpu_statements)
    return res, seen


def test_training_report_reproduces_the_reference(g):
    train = _views(g["rep_train_img"], g["rep_train_gt"], 0)
    test = _views(g["rep_test_img"], g["rep_test_gt"], 100)
    res, seen = _report(train, test)
    assert list(res) == list(g["tr_full_configs"]) == ["test", "train"]
    assert seen == [[100, 101], [2, 1, 0, 2, 1]]
    for name in ("test", "train"):
        np.testing.assert_allclose(res[name], g[f"tr_full_{name}"], rtol=0, atol=1e-12)


def test_training_report_skips_an_empty_test_set(g):
    train = _views(g["rep_train_img"], g["rep_train_gt"], 0)
    res, seen = _report(train, [])
    assert list(res) == list(g["tr_no_test_configs"]) == ["train"]
    assert seen == [[2, 1, 0, 2, 1]]
    np.testing.assert_allclose(res["train"], g["tr_no_test_train"], rtol=0, atol=1e-12)
    assert evaluate.report_configs(None, [])[1] == ("train", [])


def test_report_statements_match_the_reference_per_view(g):
    # the per-view values the device path reproduces from its sums: clamp, mean |d|, mean of per-channel PSNRs
    for v in range(len(g["img"])):
        a = torch.clamp(torch.from_numpy(g["img"][v]), 0, 1)
        b = torch.clamp(torch.from_numpy(g["gt"][v]), 0, 1)
        l1, ps = _cpu_statements(a, b)
        assert float(l1) == g["report_l1"][v] and float(ps) == g["report_psnr"][v]
        d = (a - b).double()
        per_channel = 20 * np.log10(1 / np.sqrt((d ** 2).reshape(3, -1).mean(1).numpy()))
        assert abs(per_channel.mean() - g["report_psnr"][v]) < 1e-4
        whole = 20 * np.log10(1 / np.sqrt(float((d ** 2).mean())))
        assert abs(whole - g["report_psnr"][v]) > 1e-3     # the image's PSNR is a different number


def test_write_results_layout(tmp_path):
    per_view = [{"SSIM": 0.91, "PSNR": 20.5, "L1": 0.02}, {"SSIM": 0.87, "PSNR": 19.25, "L1": 0.03}]
    names = ["00000.png", "00001.png"]
    out = evaluate.write_results(str(tmp_path), "ours_30000", per_view, names)
    full = json.load(open(tmp_path / "results.json"))
    per = json.load(open(tmp_path / "per_view.json"))
    assert full == out["results"] and per == out["per_view"]
    assert list(full) == ["ours_30000"] and sorted(full["ours_30000"]) == ["PSNR", "SSIM"]
    assert full["ours_30000"]["SSIM"] == torch.tensor([0.91, 0.87]).mean().item()
    assert full["ours_30000"]["PSNR"] == torch.tensor([20.5, 19.25]).mean().item()
    assert sorted(per["ours_30000"]) == ["PSNR", "SSIM"]
    assert per["ours_30000"]["SSIM"] == {"00000.png": torch.tensor(0.91).item(), "00001.png": torch.tensor(0.87).item()}
    assert per["ours_30000"]["PSNR"] == {"00000.png": 20.5, "00001.png": 19.25}
    # json.dump(..., indent=True) as metrics.py:119-122 writes it: one space of indentation
    assert open(tmp_path / "results.json").read().startswith('{\n "ours_30000": {\n  "')
    with pytest.raises(ValueError):
        evaluate.write_results(str(tmp_path), "m", per_view, names[:1])


def test_evaluate_views_rejects_an_unknown_mode():
    with pytest.raises(ValueError):
        evaluate.evaluate_views(None, [], None, mode="jpeg")
    assert evaluate.evaluate_views(None, [], None)["per_view"] == []


def test_schedule_calls_the_report_before_decay_statistics_and_step():
    """IterationSchedule(test_iterations=...): the report runs after backward() and before opacity_decay, the
    densification statistics and optimizer.step() (train.py:166 vs :170-198); other iterations do not report."""
    from binocular3dgs_amd.schedule import IterationSchedule
    calls = []

    class Model:
        max_radii2D = torch.zeros(4)
        optimizer = types.SimpleNamespace(step=lambda: calls.append("step"), zero_grad=lambda set_to_none: None)

        def opacity_decay(self, factor):
            calls.append("decay")

        def add_densification_stats(self, *a):
            calls.append("stats")

    cam = types.SimpleNamespace(image_height=4, image_width=4)
    scene = types.SimpleNamespace(getTrainCameras=lambda: [cam])

    def report(model, test, train, bg):
        calls.append("report")
        return {"train": (len(test), len(train))}
    s = IterationSchedule(Model(), scene, None, torch.zeros(3), ops=types.SimpleNamespace(SmoothLoss=lambda: None),
                          densify_from_iter=0, test_cameras=["t0", "t1"], test_iterations=(7,), report_fn=report)
    first = {"visibility_filter": torch.ones(4, dtype=torch.bool), "radii": torch.ones(4), "viewspace_points": None}
    s._after_backward(7, first)
    assert calls == ["report", "decay", "stats", "step"] and s.reports == {7: {"train": (2, 1)}}
    calls.clear()
    s._after_backward(8, first)
    assert calls == ["decay", "stats", "step"] and list(s.reports) == [7]


def test_metrics_entry_points_check_their_arguments_without_a_device():
    import ctypes as C
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    assert L.b3gs_image_metrics_workspace_bytes(8, 3, 600, 800) > 0
    assert L.b3gs_image_metrics_workspace_bytes(0, 3, 600, 800) == 0
    assert L.b3gs_image_metrics_batch(0, None, 3, 4, 4, 1, None, None, None) == -1
    v = (_lib.B3gsMetricView * 1)()
    out = C.c_void_p(16)                   # never dereferenced: the checks come first
    assert L.b3gs_image_metrics_batch(1, v, 3, 4, 4, 1, out, out, None) == -1          # no image / gt
    assert b"b3gs_image_metrics_batch" in L.b3gs_last_error()
    v[0].image, v[0].gt = 16, 16
    assert L.b3gs_image_metrics_batch(1, v, 5, 4, 4, 1, out, out, None) == -1          # 5 channels
    assert L.b3gs_image_metrics_batch(1, v, 3, 4, 4, 4, out, out, None) == -1          # unknown mode bit
    v[0].mask, v[0].mask_channels = 16, 2
    assert L.b3gs_image_metrics_batch(1, v, 3, 4, 4, 1, out, out, None) == -1          # mask of 2 channels
    v[0].mask_channels, v[0].prepared_image = 1, 16
    assert L.b3gs_image_metrics_batch(1, v, 3, 4, 4, 1, out, out, None) == -1          # half a prepared pair
