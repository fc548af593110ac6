"""Device: the depth-derived normals, their loss and the prior resize (csrc/normalprior.hip) against the numpy yardstick
(tests/normal_prior_ref.py) bit for bit -- block sums, parts, both gradient planes, the normals and the validity --, batches
against single calls, the self-resetting arrival counter, the term inside one training iteration of IterationSchedule and
McmcSchedule, GraphTrainer with the term in its captured step, and the command line with a folder of priors."""
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch

import normal_prior_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WEIGHTS = {"cos": (0.7, 0.0), "l1": (0.0, 0.3), "both": (0.7, 0.3)}
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = ref.make_case(*ref.CASES[name])
    return _CASES[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32 if a.dtype == np.float32 else a.dtype)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} words differ, max |d| {np.abs(got.astype(np.float64) - want.astype(np.float64)).max():.3e}"


def _dev(planes):
    return [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in planes]


def _device_loss(case, w_cos, w_l1, slot=0, mask=True):
    from binocular3dgs_amd import normal_prior as npr
    d, a, t, m = _dev(case)
    d.requires_grad_(True)
    a.requires_grad_(True)
    loss, parts, normals, valid = npr.normal_prior_loss(d, a, t, m if mask else None, ref.TANFOV, w_cos=w_cos, w_l1=w_l1,
                                                        alpha_min=ref.ALPHA_MIN, slot=slot, return_normals=True)
    loss.backward()
    H, W = d.shape[-2:]
    ws = npr._Workspace.get(d.device, W, H, slot)["ws"].view(torch.float64).cpu().numpy()
    return dict(loss=loss.detach().cpu().numpy(), parts=parts.cpu().numpy(), g_depth=d.grad[0].cpu().numpy(), g_alpha=a.grad[0].cpu().numpy(),
                normals=normals.cpu().numpy(), valid=valid[0].cpu().numpy(), ws=ws)


def _compare(got, want, W, H, what):
    sums, inv, counter = ref.workspace_views(got["ws"], W, H)
    _same(sums, want["block_sums"], what + ": block sums")
    _same(got["parts"], want["parts"], what + ": parts")
    _same(got["valid"], want["valid"], what + ": validity")
    _same(got["normals"], want["normals"], what + ": normals")
    _same(got["g_depth"], want["g_depth"], what + ": dL_ddepth")
    _same(got["g_alpha"], want["g_alpha"], what + ": dL_dalpha")
    assert got["loss"] == np.float32(want["parts"][0])
    assert inv == (1.0 / want["parts"][3] if want["parts"][3] > 0 else 0.0)
    assert counter == 0, "the arrival counter did not reset itself"


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("name", list(ref.CASES))
def test_loss_matches_the_yardstick_bit_for_bit(name, weights):
    W, H = ref.CASES[name]
    case = _case(name)
    wc, wl = WEIGHTS[weights]
    want = ref.loss(*case, *ref.TANFOV, w_cos=wc, w_l1=wl, alpha_min=ref.ALPHA_MIN)
    got = _device_loss(case, wc, wl)
    _compare(got, want, W, H, f"{name} {weights}")
    if name == "2x5":
        assert want["parts"][3] == 0 and got["loss"] == 0 and not got["g_depth"].any() and not got["g_alpha"].any()
        assert np.isfinite(got["g_depth"]).all() and np.isfinite(got["g_alpha"]).all()
    else:
        assert want["parts"][3] >= (W - 2) * (H - 2) / 2 and np.abs(got["g_depth"]).max() > 0 and np.abs(got["g_alpha"]).max() > 0


def test_two_calls_on_one_workspace_and_no_mask():
    W, H = ref.CASES["37x29"]
    case = _case("37x29")
    want = ref.loss(*case, *ref.TANFOV, w_cos=0.7, w_l1=0.3, alpha_min=ref.ALPHA_MIN)
    _compare(_device_loss(case, 0.7, 0.3, slot=3), want, W, H, "first call")
    _compare(_device_loss(case, 0.7, 0.3, slot=3), want, W, H, "second call")
    open_mask = ref.loss(case[0], case[1], case[2], None, *ref.TANFOV, w_cos=0.7, w_l1=0.3, alpha_min=ref.ALPHA_MIN)
    assert open_mask["parts"][3] > want["parts"][3]
    _compare(_device_loss(case, 0.7, 0.3, slot=3, mask=False), open_mask, W, H, "without a mask, the same workspace")


def test_batch_of_eight_sizes_equals_single_calls():
    from binocular3dgs_amd import normal_prior as npr
    sizes = [(3, 3), (2, 5), (37, 29), (300, 260), (17, 16), (16, 17), (64, 5), (5, 64)]
    cases = [ref.make_case(W, H, seed=k) for k, (W, H) in enumerate(sizes)]
    singles = [_device_loss(c, 0.7, 0.3, slot=8 + k) for k, c in enumerate(cases)]
    views = []
    for c in cases:
        d, a, t, m = _dev(c)
        views.append(dict(depth=d.requires_grad_(True), alpha=a.requires_grad_(True), target=t, mask=m, cam=ref.TANFOV))
    out = npr.normal_prior_loss_batch(views, w_cos=0.7, w_l1=0.3, alpha_min=ref.ALPHA_MIN, slot=16, return_parts=True)
    torch.stack([o[0] for o in out]).sum().backward()
    for k, ((W, H), c) in enumerate(zip(sizes, cases)):
        what = f"{W}x{H}"
        _same(out[k][1].cpu().numpy(), singles[k]["parts"], what + ": parts of the batch")
        _same(views[k]["depth"].grad[0].cpu().numpy(), singles[k]["g_depth"], what + ": dL_ddepth of the batch")
        _same(views[k]["alpha"].grad[0].cpu().numpy(), singles[k]["g_alpha"], what + ": dL_dalpha of the batch")
        want = ref.loss(*c, *ref.TANFOV, w_cos=0.7, w_l1=0.3, alpha_min=ref.ALPHA_MIN)
        _same(singles[k]["g_depth"], want["g_depth"], what + ": against the yardstick")
        _same(singles[k]["parts"], want["parts"], what + ": parts against the yardstick")


def test_a_slot_reused_before_backward_is_an_error_and_cpu_tensors_are_refused():
    from binocular3dgs_amd import normal_prior as npr
    from binocular3dgs_amd._lib import B3gsError
    d, a, t, m = _dev(_case("37x29"))
    d.requires_grad_(True)
    first = npr.normal_prior_loss(d, a, t, m, ref.TANFOV, slot=30)
    second = npr.normal_prior_loss(d, a, t, m, ref.TANFOV, slot=30)
    with pytest.raises(B3gsError, match="slot"):
        first.backward()
    second.backward()
    assert d.grad.abs().sum() > 0
    with pytest.raises(B3gsError):
        npr.normal_prior_loss(*[torch.from_numpy(x) for x in _case("3x3")], ref.TANFOV)
    with pytest.raises(ValueError, match="alpha_min"):
        npr.normal_prior_loss(d, a, t, m, ref.TANFOV, alpha_min=0.0)


@pytest.mark.parametrize("name", ["3x3", "2x5", "37x29"])
def test_depth_normals_match_the_yardstick_bit_for_bit(name):
    from binocular3dgs_amd import normal_prior as npr
    d, a, _, m = _case(name)
    for mask in (None, m):
        wn, wv = ref.depth_normals(d, a, *ref.TANFOV, ref.ALPHA_MIN, mask)
        gn, gv = npr.depth_normals(*_dev([d, a]), ref.TANFOV, alpha_min=ref.ALPHA_MIN, mask=None if mask is None else _dev([mask])[0])
        assert gn.shape == (3,) + d.shape[-2:] and gv.dtype == torch.uint8 and gv.shape == d.shape
        _same(gv[0].cpu().numpy(), wv, name + ": valid")
        _same(gn.cpu().numpy(), wn, name + ": normals")


@pytest.mark.parametrize("src_size", [(23, 11), (141, 75), (37, 29)])
def test_resize_matches_the_yardstick_bit_for_bit(src_size):
    from binocular3dgs_amd import normal_prior as npr
    Ws, Hs = src_size
    rng = np.random.default_rng(Ws)
    src = rng.standard_normal((3, Hs, Ws))
    src = (src / np.sqrt((src * src).sum(0))).astype(np.float32)
    src[:, Hs // 3:Hs // 3 + 3, Ws // 4:Ws // 4 + 5] = np.nan
    src[0, 0, 0], src[1, Hs - 1, Ws - 1] = np.inf, -np.inf
    src[:, Hs - 2, 2] = -src[:, Hs - 2, 1]           # opposite neighbours: a short interpolated vector between them
    user = (rng.random((Hs, Ws)) >= 0.05).astype(np.uint8)
    for mask in (None, user):
        wn, wm = ref.resize(src, 37, 29, mask)
        (gn, gm), = npr.resize_normals(_dev([src]), (37, 29), None if mask is None else _dev([mask]))
        assert gn.shape == (3, 29, 37) and gm.shape == (1, 29, 37) and gm.dtype == torch.uint8
        _same(gm[0].cpu().numpy(), wm, f"{src_size}: M")
        _same(gn.cpu().numpy(), wn, f"{src_size}: n")
        assert 0 < wm.sum() < wm.size
        length = np.sqrt((wn.astype(np.float64) ** 2).sum(0))
        assert np.abs(length[wm == 1] - 1).max() <= 1e-6 and not wn[:, wm == 0].any()


# ---- the trainers ------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SCENES = {}
TERM = dict(cos=0.5, l1=0.25, alpha_min=0.02)       # (alpha_min: the initial model has opacity 0.1, its rendered alpha stays low)


def _train_scene():
    """tests/ref_schedule.py's synthetic scene (computed once): 64x48"""
    import ref_schedule as rs
    if "small" not in _SCENES:
        _SCENES["small"] = rs.make_scene(W=64, H=48, P_gt=600)
    return _SCENES["small"]


def _targets(H, W, seed):
    rng = np.random.default_rng(seed)
    t = 0.3 * rng.standard_normal((3, H, W)) + np.array([0.0, 0.0, -1.0])[:, None, None]
    return (t / np.sqrt((t * t).sum(0))).astype(np.float32), (rng.random((1, H, W)) > 0.1).astype(np.uint8)


def _trainable(scene, prior_views=(0, 1, 2), iterations=500):
    """-> model (with its optimiser), Scene, cameras: the set-up of tests/test_gpu_depth_prior.py"""
    import ref_schedule as rs
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    i0, LR = scene["init"], rs.LR
    m = GaussianModel.from_tensors(i0["xyz"], i0["features_dc"], i0["features_rest"], i0["scaling"], i0["rotation"], i0["opacity"],
                                   sh_degree=1, active_sh_degree=0, device="cuda")
    cams = synth.synth_cameras(scene["W"], scene["H"], yaws=synth.YAWS_6, device="cuda")[:3]
    for k, (cam, gt) in enumerate(zip(cams, scene["gts"])):
        cam.original_image, cam.gt_alpha_mask = gt.cuda(), None
        if k in prior_views:
            t, valid = _targets(scene["H"], scene["W"], 7 + k)
            cam.normal_prior, cam.normal_prior_mask = torch.from_numpy(t).cuda(), torch.from_numpy(valid).cuda()
    m.spatial_lr_scale = scene["extent"]
    m.training_setup(types.SimpleNamespace(
        percent_dense=0.01, position_lr_init=LR["position_lr_init"], position_lr_final=LR["position_lr_final"],
        position_lr_delay_mult=LR["position_lr_delay_mult"], position_lr_max_steps=iterations, feature_lr=LR["feature_lr"],
        opacity_lr=LR["opacity_lr"], scaling_lr=LR["scaling_lr"], rotation_lr=LR["rotation_lr"]))
    return m, Scene(cams, m, cameras_extent=scene["extent"]), cams


class _RestatedTerm:
    """NormalTerm's `add` with the torch restatement supplying the term, in float64 on the device's own valid set (central
    differences cancel: in float32 the restatement, not the kernel, would set the error)"""

    def add(self, total, it, cam, pkg):
        from binocular3dgs_amd import normal_prior as npr
        d, a = pkg["rendered_depth"], pkg["rendered_alpha"]
        _, valid = npr.depth_normals(d, a, cam, alpha_min=TERM["alpha_min"], mask=cam.normal_prior_mask)
        extra, _ = ref.torch_loss(d.double(), a.double(), cam.normal_prior.double(), valid[0] != 0, *npr.tanfov(cam), w_cos=TERM["cos"],
                                  w_l1=TERM["l1"])
        return total + extra.float()


@pytest.mark.parametrize("which", ["IterationSchedule", "McmcSchedule"])
def test_one_training_iteration_with_a_normal_prior_against_the_restatement(which):
    """run_iteration of the schedule with a NormalTerm against the same iteration where the float64 torch restatement supplies
    the term: the parameter gradients (read where the schedule reports, before the optimiser step) agree to the relative L2
    bound of the project's parity checks of the drop-in path (1e-4, as tests/test_gpu_depth_prior.py uses); without the term
    they differ."""
    from binocular3dgs_amd.mcmc import McmcSchedule
    from binocular3dgs_amd.normal_prior import NormalTerm
    from binocular3dgs_amd.render import PipelineParams
    from binocular3dgs_amd.schedule import IterationSchedule
    scene = _train_scene()
    grads, losses = {}, {}
    for name, term in (("device", NormalTerm(**TERM)), ("restatement", _RestatedTerm()), ("none", None)):
        m, sc, cams = _trainable(scene)
        keep = []
        kw = dict(iterations=500, shift_cam_start=0, binocular=True, opacity_decay_factor=None, normal_prior=term,
                  after_report=lambda it: keep.append([q.grad.detach().clone() for q in m.parameters()]))
        sched = IterationSchedule(m, sc, PipelineParams(), scene["bg"].cuda(), **kw) if which == "IterationSchedule" else \
            McmcSchedule(m, sc, PipelineParams(), scene["bg"].cuda(), cap_max=400, seed=3, **kw)
        losses[name] = float(sched.run_iteration(1, 1, 0.2).detach())
        grads[name] = keep[0]
    print(f"{which}: total {losses['device']:.7f} / {losses['restatement']:.7f}, without the term {losses['none']:.7f}")
    assert abs(losses["device"] - losses["restatement"]) <= 1e-5 * abs(losses["restatement"]) and losses["device"] > losses["none"] + 0.01
    moved = 0
    for k, (a, b, c) in enumerate(zip(grads["device"], grads["restatement"], grads["none"])):
        if float(b.norm()) == 0.0:
            assert float(a.norm()) == 0.0
            continue
        rel, off = float((a - b).norm() / b.norm()), float((c - b).norm() / b.norm())
        print(f"  parameter {k}: rel L2 {rel:.3e} (without the term {off:.3e})")
        assert rel <= 1e-4, (k, rel)
        moved += off > 1e-2
    assert moved >= 3


def _graph_trainer(scene, term, prior_views=(0, 1, 2), **kw):
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    from binocular3dgs_amd.render import PipelineParams
    m, sc, cams = _trainable(scene, prior_views)
    events = []
    args = dict(iterations=500, shift_cam_start=0, binocular=True, opacity_decay_factor=None, lambda_dssim=0.2, densify_from_iter=60,
                densify_until_iter=501, densification_interval=50, sh_interval=100, events=events, normal_prior=term)
    args.update(kw)
    return GraphTrainer(m, sc, PipelineParams(), scene["bg"].cuda(), **args), m, events


def _flat(m):
    return torch.cat([q.detach().reshape(-1) for q in m.parameters()])


def test_graph_trainer_replays_over_different_views_equal_eager_steps():
    """Three replayed iterations of the pair shape with the term over three different views against three eager
    ViewShardedStep iterations staged the same way: updated parameters to 1e-3 relative L2 (the bar of
    tests/test_gpu_graph_trainer.py); ONE capture, because the target and its mask are static planes."""
    from binocular3dgs_amd._lib import B3gsError
    from binocular3dgs_amd.graph_trainer import Draw
    from binocular3dgs_amd.normal_prior import NormalTerm
    scene = _train_scene()
    shifts = (0.21, -0.13, 0.3)
    tr, m, events = _graph_trainer(scene, NormalTerm(**TERM))
    start = _flat(m).clone()
    for it in (1, 2, 3):
        tr.run_iteration(it, (it - 1) % 3, shifts[it - 1])
    assert tr.captures == 1 and [e["event"] for e in events] == ["capture", "replay", "replay", "replay"]
    assert all(e["key"][4:] == ("normal",) and e["key"][0] is True for e in events)
    assert torch.equal(tr.backend.normal, tr.views[2].normal_prior) and torch.equal(tr.backend.normal_mask, tr.views[2].normal_prior_mask)
    te, me, _ = _graph_trainer(scene, NormalTerm(**TERM))
    b = te.backend
    for it in (1, 2, 3):
        key = (True, 0.0, True, None, "normal")
        b.stage(Draw(it, (it - 1) % 3, shifts[it - 1], te.background, me.xyz_scheduler_args(it), key, True))
        b._configure(key)
        b.st.step(loss_fn=b._loss_fn)
    assert te.captures == 0
    a, e = _flat(m), _flat(me)
    rel, moved = float((a - e).norm() / e.norm()), float((e - start).norm() / start.norm())
    print(f"graph against eager after three iterations: rel L2 {rel:.3e} (the iterations moved the parameters by {moved:.3e})")
    assert rel <= 1e-3 and moved > 0
    # ... and the term is in the captured step: the same three replays without it end elsewhere, under the four-entry key
    tn, mn, ev = _graph_trainer(scene, None)
    for it in (1, 2, 3):
        tn.run_iteration(it, (it - 1) % 3, shifts[it - 1])
    assert all(len(x["key"]) == 4 for x in ev if "key" in x)
    assert float((_flat(mn) - e).norm()) > 10 * float((a - e).norm())
    with pytest.raises(B3gsError, match="all or none"):
        _graph_trainer(scene, NormalTerm(**TERM), prior_views=(0, 2))


def test_cli_with_a_folder_of_priors_in_both_step_modes_and_normal_cos(tmp_path):
    """train --normal_priors DIR through Scene.from_dataset / attach_normal_priors in both --step modes (with --depth_priors and
    --exposure next to it in the graph run), and evaluate --normal_priors: NormalCos in results.json and per view."""
    from binocular3dgs_amd import evaluate, train
    from binocular3dgs_amd.frames import read_png, write_png
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    priors, depths = tmp_path / "normals", tmp_path / "depths"
    os.makedirs(priors)
    os.makedirs(depths)
    rng = np.random.default_rng(2)
    for k, f in enumerate(sorted(os.listdir(src / "images"))):
        h, w = read_png(str(src / "images" / f)).shape[:2]
        t, _ = _targets(h // 2, w // 2, k)
        t = t * np.array([1, -1, -1], np.float32)[:, None, None]                  # stored in the OpenGL frame
        stem = os.path.splitext(f)[0]
        if k % 2:
            np.save(priors / (stem + ".npy"), t.transpose(1, 2, 0).astype(np.float64))
        else:
            write_png(str(priors / (stem + ".png")), ((t.transpose(1, 2, 0) + 1) * 127.5 + 0.5).astype(np.uint8))
        np.save(depths / (stem + ".npy"), (1 + rng.random((h // 2, w // 2))).astype(np.float32))

    def args(out, *extra):
        return train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "12",
                                          "--shift_cam_start", "4", "--densify_from_iter", "100", "--quiet", *extra])
    flags = ("--normal_priors", str(priors), "--normal_prior_frame", "opengl", "--normal_prior_cos", "0.05", "--normal_prior_l1", "0.02",
             "--normal_prior_alpha_min", "0.05")
    more = ("--step", "graph", "--depth_priors", str(depths), "--depth_prior_weight", "0.05", "--exposure")
    res = {}
    for name, extra in (("plain", ()), ("schedule", flags), ("graph", flags + more)):
        res[name] = train.run(args(tmp_path / name, *extra))
        assert np.isfinite(res[name]["loss"]) and res[name]["points"] > 0
    assert res["schedule"]["loss"] > res["plain"]["loss"] and res["graph"]["loss"] > res["plain"]["loss"]
    views = res["graph"]["trainer"].views
    assert res["graph"]["captures"] >= 2 and all(c.normal_prior is not None and c.normal_prior_mask.dtype == torch.uint8 and
                                                tuple(c.normal_prior.shape) == (3, c.image_height, c.image_width) for c in views)
    assert all(float(c.normal_prior[2][c.normal_prior_mask[0] != 0].mean()) < -0.5 for c in views)      # converted: facing the camera
    with open(tmp_path / "graph" / "cfg_args") as fp:
        assert "normal_prior_frame='opengl'" in fp.read()
    out = evaluate.run(str(tmp_path / "graph"), normal_priors=str(priors))
    with open(tmp_path / "graph" / "results.json") as fp:
        full = json.load(fp)
    with open(tmp_path / "graph" / "per_view.json") as fp:
        per = json.load(fp)
    method, = full
    assert -1 <= full[method]["NormalCos"] <= 1 and len(per[method]["NormalCos"]) == len(per[method]["PSNR"]) >= 1
    assert abs(full[method]["NormalCos"] - np.mean(list(per[method]["NormalCos"].values()))) <= 1e-6
    assert abs(out["NormalCos"] - full[method]["NormalCos"]) <= 1e-6
    shutil.rmtree(priors)
    os.makedirs(priors)
    with pytest.raises(FileNotFoundError, match=".npy"):
        train.run(args(tmp_path / "missing", *flags))
