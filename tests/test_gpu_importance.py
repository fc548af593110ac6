"""binocular3dgs_amd.importance and the prune command line on the device: contributions() against the fold of direct ABI
calls, scores and selection, prune(), and the property the module's docstring promises -- where no pixel saturates, removing the
Gaussians with zero hits leaves the renders of the same cameras bit-identical."""
import ctypes as C
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_SYNTH = 400


def _scene():
    """400 faint Gaussians (opacity 0.02 .. 0.1: no pixel comes near saturation) in front of three cameras of two sizes, and one
    more -- the last row -- behind all of them."""
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.gaussian_model import GaussianModel, inverse_sigmoid
    p = synth.synth_gaussians(P_SYNTH, seed=5, width=96, height=64, scale_mult=8.0)
    g = torch.Generator().manual_seed(11)
    p["opacity"] = inverse_sigmoid(0.02 + 0.08 * torch.rand(P_SYNTH, 1, generator=g))
    for k in p:
        p[k] = torch.cat([p[k], p[k][:1]])
    p["xyz"][-1] = torch.tensor([0.0, 0.0, -50.0])
    model = GaussianModel.from_tensors(p["xyz"], p["features_dc"], p["features_rest"], p["scaling"], p["rotation"], p["opacity"],
                                       sh_degree=1, active_sh_degree=1, device="cuda", requires_grad=False)
    cams = synth.synth_cameras(96, 64, yaws=(0.0, 7.0), device="cuda") + synth.synth_cameras(75, 33, yaws=(-5.0,), device="cuda")
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    return model, cams, bg


def _direct(model, cams, bg):
    """One ABI call per camera on the evaluation renderer's slot 0, folded on the host: weight_q, hits, wmax bits, dominant."""
    from binocular3dgs_amd import _lib, evaluate
    L = _lib.lib()
    P = model.get_xyz.shape[0]
    fold = dict(wq=np.zeros(P, np.int64), hits=np.zeros(P, np.int64), wmax=np.zeros(P, np.uint32), dom=np.zeros(P, np.int64))
    final_T_min = 1.0
    for cam in cams:
        for _idx, _outs in evaluate._batches(model, [cam], bg, 1, None, full=True):
            W, H = int(cam.image_width), int(cam.image_height)
            s = model.__dict__["_b3gs_eval_renderers"][(W, H)].slots[0]
            sc = _lib.B3gsScene()
            sc.P, sc.W, sc.H = P, W, H
            view = (_lib.B3gsContribView * 1)(_lib.B3gsContribView(C.pointer(sc), s.geom.data_ptr(), s.binning.data_ptr(),
                                                                   s.img.data_ptr(), None))
            out = [torch.zeros(P, dtype=torch.int64, device="cuda")] + [torch.zeros(P, dtype=torch.int32, device="cuda") for _ in range(3)]
            co = _lib.B3gsContribOut(*(t.data_ptr() for t in out))
            _lib.check(L.b3gs_blend_contribution_batch(1, view, C.byref(co), torch.cuda.current_stream().cuda_stream),
                       "b3gs_blend_contribution_batch")
            torch.cuda.synchronize()
            u32 = [t.cpu().numpy().view(np.uint32) for t in out[1:]]
            fold["wq"] += out[0].cpu().numpy()
            fold["hits"] += u32[0]
            fold["wmax"] = np.maximum(fold["wmax"], u32[1])
            fold["dom"] += u32[2]
            from binocular3dgs_amd.debug import state_views
            final_T_min = min(final_T_min, float(state_views(P, W, H, s.capacity, s.geom, s.binning, s.img)["final_T"].min()))
    return fold, final_T_min


@pytest.fixture(scope="module")
def scene():
    from binocular3dgs_amd import importance
    model, cams, bg = _scene()
    return model, cams, bg, importance.contributions(model, cams, bg, batch=2)


def test_contributions_equal_the_fold_of_direct_calls_whatever_the_batch(scene):
    from binocular3dgs_amd import importance
    model, cams, bg, c = scene
    fold, _ = _direct(model, cams, bg)
    assert fold["hits"].sum() > 1000
    assert c.weight.dtype == torch.float64 and c.hits.dtype == c.dominant.dtype == torch.int64 and c.wmax.dtype == torch.float32
    assert np.array_equal(c.weight.cpu().numpy(), fold["wq"] / 4294967296.0)
    assert np.array_equal(c.hits.cpu().numpy(), fold["hits"]) and np.array_equal(c.dominant.cpu().numpy(), fold["dom"])
    assert np.array_equal(c.wmax.cpu().numpy().view(np.uint32), fold["wmax"])
    for batch in (1, 8):
        o = importance.contributions(model, cams, bg, batch=batch)
        for k in ("weight", "hits", "dominant", "wmax"):
            assert torch.equal(getattr(o, k), getattr(c, k)), (batch, k)
    # the Gaussian behind every camera
    assert c.weight[-1] == 0 and c.hits[-1] == 0 and c.dominant[-1] == 0 and c.wmax[-1] == 0
    # a mask of nothing for one camera takes exactly that camera's share out
    masks = [None, torch.zeros(64, 96, dtype=torch.bool, device="cuda"), None]
    part = importance.contributions(model, cams, bg, masks=masks)
    only = importance.contributions(model, [cams[0], cams[2]], bg)
    for k in ("weight", "hits", "dominant", "wmax"):
        assert torch.equal(getattr(part, k), getattr(only, k)), k


def test_scores_and_selection(scene):
    from binocular3dgs_amd import importance
    model, _cams, _bg, c = scene
    P = c.hits.shape[0]
    assert importance.score(c, model, "weight") is c.weight
    sig = importance.score(c, model, "significance")
    vol = torch.prod(model.get_scaling.double(), 1)
    v = torch.clamp(vol / torch.sort(vol).values[int(0.9 * P)], 0, 1) ** 0.1
    assert torch.equal(sig, c.hits.double() * model.get_opacity.double().reshape(-1) * v) and (sig[c.hits == 0] == 0).all()
    with pytest.raises(ValueError):
        importance.score(c, model, "other")
    half = importance.select(c.weight, keep=0.5)
    assert half.dtype == torch.bool and int(half.sum()) == math.ceil(P / 2)
    assert c.weight[half].min() >= c.weight[~half].max()
    tie = importance.select(torch.tensor([1.0, 3.0, 3.0, 3.0, 0.0], dtype=torch.float64), keep=0.4)
    assert tie.tolist() == [False, True, True, False, False]
    both = importance.select(c, keep=0.5, min_hits=50, never_dominant=True)
    assert torch.equal(both, half & (c.hits >= 50) & (c.dominant > 0)) and 0 < int(both.sum()) <= int(half.sum())
    assert torch.equal(importance.select(c.weight, min_score=1.0), c.weight >= 1.0)
    with pytest.raises(ValueError):
        importance.select(c.weight, min_hits=1)


def test_prune_carries_rows_and_degrees(scene):
    from binocular3dgs_amd import importance
    model, _cams, _bg, c = scene
    mask = importance.select(c, keep=0.3)
    small = importance.prune(model, mask)
    assert small.get_xyz.shape[0] == int(mask.sum())
    assert (small.max_sh_degree, small.active_sh_degree) == (model.max_sh_degree, model.active_sh_degree)
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity"):
        assert torch.equal(getattr(small, name).detach(), getattr(model, name).detach()[mask]), name
    assert small.optimizer is None


def test_pruning_zero_hit_gaussians_leaves_unsaturated_renders_bit_identical(scene):
    from binocular3dgs_amd import evaluate, importance
    model, cams, bg, c = scene
    _fold, final_T_min = _direct(model, cams, bg)
    assert final_T_min > 1e-4, "a pixel saturates: the scene is not what this test needs"
    mask = importance.select(c, min_hits=1)
    assert 0 < int((~mask).sum()) < mask.shape[0] and not bool(mask[-1])
    small = importance.prune(model, mask)

    def renders(m):
        out = {}
        for idx, outs in evaluate._batches(m, cams, bg, 8, None, full=True):
            for i, o in zip(idx, outs):
                out[i] = tuple(o[k].clone() for k in ("render", "rendered_depth", "rendered_alpha"))
        return out
    a, b = renders(model), renders(small)
    for i in range(len(cams)):
        assert a[i][2].max() > 0.05
        for x, y, k in zip(a[i], b[i], ("colour", "depth", "alpha")):
            assert torch.equal(x, y), (i, k)


def test_command_line_writes_a_pruned_iteration(tmp_path, capsys):
    from binocular3dgs_amd import prune, spiral
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.init_points import load_ply
    from binocular3dgs_amd.scene import Scene
    src = shutil.copytree(os.path.join(ROOT, "tests", "golden", "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "model"
    np.random.seed(0)
    model = GaussianModel(1)
    scene = Scene.from_dataset(str(src), model, eval=True, n_views=3, dataset_name="LLFF", resolution=1, init_points="sparse",
                               model_path=str(out), shuffle=False)
    scene.save(7)
    P = model.get_xyz.shape[0]
    with open(out / "cfg_args", "w") as fp:
        fp.write(f"Namespace(source_path={str(src)!r}, images='images', eval=True, n_views=3, dataset_name='LLFF', resolution=1, "
                 "white_background=False, sh_degree=1, init_points='sparse')")
    npz = str(tmp_path / "stats.npz")
    assert prune.main(["-m", str(out), "--views", "all", "--keep", "0.6", "--min_hits", "1", "--evaluate", "--stats", npz]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["P_before"] == P and 0 < res["P_after"] <= math.ceil(0.6 * P)
    assert 0.0 <= res["zero_hit_share"] <= res["never_dominant_share"] <= 1.0 and 0.0 < res["weight_share_kept"] <= 1.0
    for tag in ("before", "after"):
        assert set(res[tag]) == {"PSNR", "SSIM", "L1"} and all(np.isfinite(v) for v in res[tag].values())
    ply = out / "point_cloud" / "iteration_7_pruned" / "point_cloud.ply"
    assert res["ply"] == str(ply) and load_ply(str(ply), 1).get_xyz.shape[0] == res["P_after"]
    st = np.load(npz)
    assert all(st[k].shape == (P,) for k in ("weight", "hits", "dominant", "wmax", "kept")) and int(st["kept"].sum()) == res["P_after"]
    assert spiral.max_iteration(str(out)) == 7      # the pruned folder is not taken for a later iteration
