"""Device: the depth-prior loss and the prior resize (csrc/depthprior.hip) against the numpy yardstick (tests/depth_prior_ref.py)
bit for bit -- sums, skip decisions, parts and the gradient plane --, batches against single calls, the self-resetting arrival
counter, the term inside one training iteration of IterationSchedule and McmcSchedule, GraphTrainer with the term in its
captured step, and the command line with a folder of priors."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

import depth_prior_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KW = dict(w_global=0.7, w_local=1.3, min_valid=ref.MIN_VALID, alpha_min=ref.ALPHA_MIN)


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


def _device_loss(planes, slot=0, **kw):
    from binocular3dgs_amd import depth_prior as dp
    d, a, p, m = _dev(planes)
    d.requires_grad_(True)
    loss, parts = dp.depth_prior_loss(d, a, p, m, slot=slot, return_parts=True, **kw)
    loss.backward()
    H, W = d.shape[-2:]
    ws = dp._Workspace.get(d.device, W, H, kw.get("patch", 0), slot)["ws"].view(torch.float64).cpu().numpy()
    return dict(loss=loss.detach().cpu().numpy(), parts=parts.cpu().numpy(), grad=d.grad[0].cpu().numpy(), ws=ws)


def _compare(got, want, W, H, patch, what):
    img, psums, pflags = ref.workspace_views(got["ws"], W, H, patch)
    _same(img, want["image_sums"], what + ": image sums")
    _same(psums, want["patch_sums"], what + ": patch sums")
    _same(pflags, want["patch_flags"], what + ": skip decisions")
    _same(got["parts"], want["parts"], what + ": parts")
    _same(got["grad"], want["grad"], what + ": dL_ddepth")
    assert got["loss"] == np.float32(want["parts"][0])
    assert got["ws"].view(np.uint64)[0] == 0, "the arrival counter did not reset itself"


@pytest.mark.parametrize("mode", ["depth", "disparity"])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_loss_matches_the_yardstick_bit_for_bit(name, mode):
    W, H, p, off = ref.CASES[name]
    planes = ref.make_case(W, H, p, off)[:4]
    kw = dict(KW, mode=mode, patch=p, offset=off)
    want = ref.loss(*planes, **kw)
    assert want["parts"][4] > 0 and want["parts"][1] > 0
    _compare(_device_loss(planes, **kw), want, W, H, p, f"{name} {mode}")


def test_global_term_alone_and_two_calls_on_one_workspace():
    W, H, p, off = ref.CASES["70x37_o5_9"]
    planes = ref.make_case(W, H, p, off)[:4]
    kw = dict(KW, mode="depth", patch=0, w_local=0.0)
    want = ref.loss(*planes, **kw)
    one, two = _device_loss(planes, **kw), _device_loss(planes, **kw)
    _compare(one, want, W, H, 0, "first call")
    _compare(two, want, W, H, 0, "second call")
    # ... and a different offset on the same workspace moves the grid (the offsets are read on the device)
    kw = dict(KW, mode="depth", patch=p)
    for o in ((0, 0), (15, 15), (0, 0)):
        _compare(_device_loss(planes, offset=o, **kw), ref.loss(*planes, offset=o, **kw), W, H, p, f"offset {o}")


def test_an_image_that_is_skipped():
    W, H, p, off = ref.CASES["70x37_o0_0"]
    planes = ref.make_case(W, H, p, off)[:4]
    got = _device_loss(planes, **dict(KW, mode="depth", patch=p, offset=off, min_valid=W * H + 1))
    assert got["loss"] == 0 and not got["parts"][[0, 1, 2, 4, 5, 6, 7]].any() and not got["grad"].any()


def test_batch_of_two_sizes_equals_single_calls():
    from binocular3dgs_amd import depth_prior as dp
    names = ("70x37_o5_9", "300x7_p8")
    p = 8
    cases = [ref.make_case(*ref.CASES[n][:2], p, ref.CASES[n][3], seed=k)[:4] for k, n in enumerate(names)]
    kw = dict(KW, mode="disparity", patch=p)
    singles = [_device_loss(c, slot=4 + k, offset=ref.CASES[n][3], **kw) for k, (c, n) in enumerate(zip(cases, names))]
    views = []
    for c, n in zip(cases, names):
        d, a, pr, m = _dev(c)
        views.append(dict(depth=d.requires_grad_(True), alpha=a, prior=pr, mask=m, offset=ref.CASES[n][3]))
    out = dp.depth_prior_loss_batch(views, slot=8, return_parts=True, **kw)
    torch.stack([o[0] for o in out]).sum().backward()
    for k, (n, c) in enumerate(zip(names, cases)):
        W, H = ref.CASES[n][:2]
        _same(out[k][1].cpu().numpy(), singles[k]["parts"], n + ": parts of the batch")
        _same(views[k]["depth"].grad[0].cpu().numpy(), singles[k]["grad"], n + ": gradient of the batch")
        _same(singles[k]["grad"], ref.loss(*c, offset=ref.CASES[n][3], **kw)["grad"], n + ": against the yardstick")


@pytest.mark.parametrize("src_size", [(23, 11), (141, 75), (70, 37)])
def test_resize_matches_the_yardstick_bit_for_bit(src_size):
    from binocular3dgs_amd import depth_prior as dp
    Ws, Hs = src_size
    rng = np.random.default_rng(Ws)
    src = (0.5 + 4 * rng.random((Hs, Ws))).astype(np.float32)
    src[Hs // 3:Hs // 3 + 3, Ws // 4:Ws // 4 + 5] = np.nan
    src[0, 0], src[Hs - 1, Ws - 1], src[1, 2] = np.inf, 0.0, -2.0
    user = (rng.random((Hs, Ws)) >= 0.05).astype(np.uint8)
    for mask in (None, user):
        wp, wm = ref.resize(src, 70, 37, mask)
        (gp, gm), = dp.resize_priors(_dev([src]), (70, 37), None if mask is None else _dev([mask]))
        assert gp.shape == (1, 37, 70) and gm.dtype == torch.uint8
        _same(gm[0].cpu().numpy(), wm, f"{src_size}: M")
        _same(gp[0].cpu().numpy(), wp, f"{src_size}: P")
        assert 0 < wm.sum() < wm.size
        if src_size == (70, 37) and mask is None:
            ok = np.isfinite(src) & (src > 0)
            _same(gp[0].cpu().numpy()[ok], src[ok], "equal size is the identity")


def test_align_and_cpu_tensors():
    from binocular3dgs_amd import depth_prior as dp
    from binocular3dgs_amd._lib import B3gsError
    W, H, p, off = ref.CASES["70x37_o0_0"]
    planes = ref.make_case(W, H, p, off)[:4]
    d, a, pr, m = _dev(planes)
    _, parts = dp.depth_prior_loss(d, a, pr, m, mode="depth", return_parts=True, slot=12)
    fit = dp.align(pr, parts)
    used = planes[3][0] != 0
    # the least-squares line of numpy on the used pixels, in float64: the same (a, b) up to the rounding of two summation orders
    a_np, b_np = np.polyfit(planes[2][0][used].astype(np.float64), planes[0][0][used].astype(np.float64), 1)
    assert abs(float(parts[6]) - a_np) <= 1e-9 * abs(a_np) and abs(float(parts[7]) - b_np) <= 1e-9 * max(1.0, abs(b_np))
    want = (a_np * planes[2].astype(np.float64) + b_np).astype(np.float32)
    assert np.abs(fit.cpu().numpy() - want).max() <= 4 * np.spacing(np.abs(want).max())
    with pytest.raises(B3gsError):
        dp.depth_prior_loss(*[torch.from_numpy(x) for x in planes], mode="depth")


def _scene(prior_views):
    """a tiny synthetic scene at 64x48 with a few hundred Gaussians; `prior_views`: indices of the views that carry a prior"""
    import types
    from binocular3dgs_amd import synth
    W, H = 64, 48
    model = synth.synth_model(300, seed=3, device=DEV, width=W, height=H)
    cams = synth.synth_cameras(W, H, yaws=(0.0, 4.0), device=DEV)
    rng = np.random.default_rng(5)
    for i, c in enumerate(cams):
        c.original_image = torch.from_numpy(rng.random((3, H, W)).astype(np.float32)).to(DEV)
        if i in prior_views:
            c.depth_prior = torch.from_numpy((1 + rng.random((1, H, W))).astype(np.float32)).to(DEV)
            c.depth_prior_mask = torch.from_numpy((rng.random((1, H, W)) > 0.1).astype(np.uint8)).to(DEV)
    scene = types.SimpleNamespace(getTrainCameras=lambda: cams, getShiftedCamera=lambda c, s: c.shifted(s), cameras_extent=1.0)
    return model, scene, cams


def test_the_term_through_the_rasterizer_against_the_restatement():
    """One loss + backward of the drop-in render with the prior term from the device kernels, against the same with the torch
    restatement (float32) supplying the term: parameter gradients agree to the relative L2 bound of the project's parity
    checks of the drop-in path (1e-4, as __graft_entry__.smoke and the rasterizer parity tests use)."""
    from binocular3dgs_amd import depth_prior as dp
    from binocular3dgs_amd.render import PipelineParams, render
    model, scene, cams = _scene({0})
    cam, bg = cams[0], torch.zeros(3, device=DEV)
    term = dp.PriorTerm(mode="depth", weight=0.5, local=0.5, patch=16, alpha_min=0.3, seed=1)
    off = (5, 9)
    grads = []
    for which in ("device", "restatement"):
        for q in model.parameters():
            q.grad = None
        pkg = render(cam, model, PipelineParams(), bg)
        photo = (pkg["render"] - cam.original_image).abs().mean()
        if which == "device":
            extra = term.loss(cam, pkg, offset=off, slot=16)
        else:
            extra, _ = ref.torch_loss(pkg["rendered_depth"], pkg["rendered_alpha"], cam.depth_prior, cam.depth_prior_mask, mode="depth",
                                      w_global=0.5, w_local=0.5, patch=16, min_valid=16, alpha_min=0.3, offset=off)
        (photo + extra).backward()
        grads.append((float(extra.detach()), {n: q.grad.clone() for n, q in enumerate(model.parameters()) if q.grad is not None}))
    (ld, gd), (lr, gr) = grads
    print(f"term: device {ld:.7f}, restatement {lr:.7f}")
    assert ld > 0 and abs(ld - lr) <= 1e-5 * max(1.0, abs(lr))
    for n in gr:
        rel = float((gd[n] - gr[n]).norm() / gr[n].norm().clamp(min=1e-30))
        print(f"  {n}: rel L2 {rel:.3e}")
        assert rel <= 1e-4, (n, rel)


def test_the_term_adds_itself_only_for_views_with_a_prior_in_its_window():
    from binocular3dgs_amd import depth_prior as dp
    model, scene, cams = _scene({0})
    term = dp.PriorTerm(mode="disparity", weight=0.25, seed=1, from_iter=2)
    pkg = dict(rendered_depth=torch.full((1, 48, 64), 2.0, device=DEV).add_(torch.rand((1, 48, 64), device=DEV)).requires_grad_(True),
               rendered_alpha=torch.ones((1, 48, 64), device=DEV))
    base = torch.zeros((), device=DEV)
    assert term.add(base, 5, cams[1], pkg) is base          # no prior on this view: no call
    assert term.add(base, 1, cams[0], pkg) is base          # before the window
    total = term.add(base, 5, cams[0], pkg)
    assert total is not base and float(total) > 0
    total.backward()
    assert pkg["rendered_depth"].grad.abs().sum() > 0
    # the offset draws are the term's own: python's global generator does not move
    import random
    random.seed(3)
    a = random.random()
    random.seed(3)
    dp.PriorTerm(mode="depth", local=1.0, patch=16, seed=9).draw_offset()
    assert random.random() == a


# ---- the trainers ------------------------------------------------------------------------------------------------------
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_SCENES = {}


def _train_scene(small=True):
    """tests/ref_schedule.py's synthetic scene (computed once per size): 300 Gaussians at 64x48, or its own default"""
    import ref_schedule as rs
    if small not in _SCENES:
        _SCENES[small] = rs.make_scene(W=64, H=48, P_gt=600) if small else rs.make_scene()
    return _SCENES[small]


def _trainable(scene, prior_views=(0, 1, 2), iterations=500):
    """-> model (with its optimiser), Scene, cameras: the set-up of tests/test_gpu_graph_trainer.py::GraphLead"""
    import ref_schedule as rs
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    i0, LR = scene["init"], rs.LR
    m = GaussianModel.from_tensors(i0["xyz"], i0["features_dc"], i0["features_rest"], i0["scaling"], i0["rotation"], i0["opacity"],
                                   sh_degree=1, active_sh_degree=0, device="cuda")
    cams = synth.synth_cameras(scene["W"], scene["H"], yaws=synth.YAWS_6, device="cuda")[:3]
    rng = np.random.default_rng(7)
    for k, (cam, gt) in enumerate(zip(cams, scene["gts"])):
        cam.original_image, cam.gt_alpha_mask = gt.cuda(), None
        prior = (1 + rng.random((1, scene["H"], scene["W"]))).astype(np.float32)
        valid = (rng.random((1, scene["H"], scene["W"])) > 0.1).astype(np.uint8)
        if k in prior_views:
            cam.depth_prior, cam.depth_prior_mask = torch.from_numpy(prior).cuda(), torch.from_numpy(valid).cuda()
    m.spatial_lr_scale = scene["extent"]
    m.training_setup(types.SimpleNamespace(
        percent_dense=0.01, position_lr_init=LR["position_lr_init"], position_lr_final=LR["position_lr_final"],
        position_lr_delay_mult=LR["position_lr_delay_mult"], position_lr_max_steps=iterations, feature_lr=LR["feature_lr"],
        opacity_lr=LR["opacity_lr"], scaling_lr=LR["scaling_lr"], rotation_lr=LR["rotation_lr"]))
    return m, Scene(cams, m, cameras_extent=scene["extent"]), cams


# (alpha_min: the initial model has opacity 0.1, its rendered alpha stays low)
TERM = dict(mode="depth", weight=0.5, local=0.5, patch=16, alpha_min=0.02, seed=11)


class _RestatedTerm:
    """PriorTerm's `add` with the float32 torch restatement supplying the term (the same offset draws)"""

    def __init__(self):
        from binocular3dgs_amd.depth_prior import PriorTerm
        self.draws = PriorTerm(**TERM)

    def add(self, total, it, cam, pkg):
        extra, _ = ref.torch_loss(pkg["rendered_depth"], pkg["rendered_alpha"], cam.depth_prior, cam.depth_prior_mask, mode="depth",
                                  w_global=0.5, w_local=0.5, patch=16, min_valid=16, alpha_min=TERM["alpha_min"], offset=self.draws.draw_offset())
        return total + extra


@pytest.mark.parametrize("which", ["IterationSchedule", "McmcSchedule"])
def test_one_training_iteration_with_a_prior_against_the_restatement(which):
    """run_iteration of the schedule with a PriorTerm against the same iteration where the torch restatement supplies the term:
    the parameter gradients (read where the schedule reports, before the optimiser step) agree to the relative L2 bound of
    the project's parity checks of the drop-in path (1e-4, as __graft_entry__.smoke uses); without the term they differ."""
    from binocular3dgs_amd.depth_prior import PriorTerm
    from binocular3dgs_amd.mcmc import McmcSchedule
    from binocular3dgs_amd.render import PipelineParams
    from binocular3dgs_amd.schedule import IterationSchedule
    scene = _train_scene()
    grads, losses = {}, {}
    for name, term in (("device", PriorTerm(**TERM)), ("restatement", _RestatedTerm()), ("none", None)):
        m, sc, cams = _trainable(scene)
        keep = []
        kw = dict(iterations=500, shift_cam_start=0, binocular=True, opacity_decay_factor=None, depth_prior=term,
                  after_report=lambda it: keep.append([q.grad.detach().clone() for q in m.parameters()]))
        sched = IterationSchedule(m, sc, PipelineParams(), scene["bg"].cuda(), **kw) if which == "IterationSchedule" else \
            McmcSchedule(m, sc, PipelineParams(), scene["bg"].cuda(), cap_max=400, seed=3, **kw)
        losses[name] = float(sched.run_iteration(1, 1, 0.2).detach())
        grads[name] = keep[0]
    print(f"{which}: total {losses['device']:.7f} / {losses['restatement']:.7f}, without the term {losses['none']:.7f}")
    assert abs(losses["device"] - losses["restatement"]) <= 1e-5 * abs(losses["restatement"]) and losses["device"] > losses["none"] + 0.1
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
                densify_until_iter=501, densification_interval=50, sh_interval=100, events=events, depth_prior=term)
    args.update(kw)
    return GraphTrainer(m, sc, PipelineParams(), scene["bg"].cuda(), **args), m, events


def _flat(m):
    return torch.cat([q.detach().reshape(-1) for q in m.parameters()])


def test_graph_trainer_replays_with_moving_offsets_equal_eager_steps():
    """Three replayed iterations of the pair shape with the term, the patch grid moving with every draw, against three eager
    ViewShardedStep iterations staged the same way: updated parameters to 1e-3 relative L2 (the bar of
    tests/test_gpu_graph_trainer.py); ONE capture, because the offsets live in device memory."""
    from binocular3dgs_amd.depth_prior import PriorTerm
    from binocular3dgs_amd.graph_trainer import Draw
    scene = _train_scene()
    shifts = (0.21, -0.13, 0.3)
    tr, m, events = _graph_trainer(scene, PriorTerm(**TERM))
    start = _flat(m).clone()
    for it in (1, 2, 3):
        tr.run_iteration(it, (it - 1) % 3, shifts[it - 1])
    assert tr.captures == 1 and [e["event"] for e in events] == ["capture", "replay", "replay", "replay"]
    assert all(e["key"][4:] == ("prior",) and e["key"][0] is True for e in events)
    draws = PriorTerm(**TERM)
    offsets = [draws.draw_offset() for _ in range(3)]
    assert len(set(offsets)) == 3 and tr.backend.offset_dev.tolist() == list(offsets[-1])
    # eager: the same staging, ViewShardedStep.step outside any graph
    te, me, _ = _graph_trainer(scene, PriorTerm(**TERM))
    b = te.backend
    for it in (1, 2, 3):
        key = (True, 0.0, True, None, "prior")
        b.stage(Draw(it, (it - 1) % 3, shifts[it - 1], te.background, me.xyz_scheduler_args(it), key, True, te.depth_prior.draw_offset()))
        b._configure(key)
        b.st.step(loss_fn=b._loss_fn)
    assert te.captures == 0
    a, e = _flat(m), _flat(me)
    rel, moved = float((a - e).norm() / e.norm()), float((e - start).norm() / start.norm())
    print(f"graph against eager after three iterations: rel L2 {rel:.3e} (the iterations moved the parameters by {moved:.3e})")
    assert rel <= 1e-3 and moved > 0
    # ... and the term is in the captured step: the same three replays without it end elsewhere
    tn, mn, _ = _graph_trainer(scene, None)
    for it in (1, 2, 3):
        tn.run_iteration(it, (it - 1) % 3, shifts[it - 1])
    assert float((_flat(mn) - e).norm()) > 10 * float((a - e).norm())


def test_graph_trainer_refuses_a_mixed_prior_set():
    from binocular3dgs_amd._lib import B3gsError
    from binocular3dgs_amd.depth_prior import PriorTerm
    with pytest.raises(B3gsError, match="all or none"):
        _graph_trainer(_train_scene(), PriorTerm(**TERM), prior_views=(0, 2))


def _library_launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(e.count for e in dev), sum(e.count for e in dev if "depth_prior_" in e.key)


def test_a_run_without_priors_issues_what_it_always_did():
    """No prior on any camera: the events are the ones tests/test_gpu_graph_trainer.py asserts for its 210 iterations (the
    same scene and schedule), every key is the four-entry one, and an iteration launches no kernel of depthprior.hip; with the
    priors on, the same iteration launches exactly two of them (the issue's bar: at most 3 per call)."""
    from binocular3dgs_amd.depth_prior import PriorTerm
    from binocular3dgs_amd.graph_trainer import Draw
    scene = _train_scene(small=False)
    kw = dict(shift_cam_start=100, opacity_decay_factor=0.995, densify_grad_threshold=0.001, before_densify=None)
    shifts = np.random.default_rng(5).random(211) * 0.4
    tr, m, events = _graph_trainer(scene, None, prior_views=(), **kw)
    for it in range(1, 211):
        tr.densify_until_iter = 501
        tr.run_iteration(it, (it - 1) % 3, float(shifts[it]))
    caps = [(e["it"], e["why"]) for e in events if e["event"] == "capture"]
    assert caps == [(1, "first use"), (61, "first use"), (101, "densification"), (151, "densification"), (201, "densification")], caps
    assert tr.grown == 0 and all(len(e["key"]) == 4 for e in events if "key" in e)
    assert [e["event"] for e in events if e["event"] not in ("capture", "replay")] == \
        ["grads", "decay", "densify", "grads", "decay", "densify", "grads", "decay", "densify"]
    key = (True, 0.0, True, None)

    def eager(t, k, offset):
        def fn():
            t.backend.stage(Draw(211, 0, 0.2, t.background, 1e-4, k, False, offset))
            t.backend.grads_only(k)
        return fn
    total0, lib0 = _library_launches(eager(tr, key, None))
    tp, _, _ = _graph_trainer(scene, PriorTerm(**TERM), **kw)
    total1, lib1 = _library_launches(eager(tp, key + ("prior",), (3, 4)))
    print(f"device launches of one eager iteration: {total0} without priors ({lib0} of depthprior.hip), {total1} with ({lib1})")
    assert lib0 == 0 and lib1 == 2 and total1 > total0


def test_cli_with_a_folder_of_priors_in_both_step_modes_and_depth_pearson(tmp_path):
    """train --depth_priors DIR through Scene.from_dataset / attach_priors in both --step modes, the view and shift draws left
    where they were, and evaluate --depth_priors: DepthPearson in results.json and per view in per_view.json."""
    import json
    import random
    from binocular3dgs_amd import evaluate, train
    from binocular3dgs_amd.frames import read_png
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    priors = tmp_path / "priors"
    os.makedirs(priors)
    rng = np.random.default_rng(2)
    for f in sorted(os.listdir(src / "images")):
        h, w = read_png(str(src / "images" / f)).shape[:2]
        np.save(priors / (os.path.splitext(f)[0] + ".npy"), (1 + rng.random((h // 2, w // 2))).astype(np.float64))

    def args(out, *extra):
        return train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "12",
                                          "--shift_cam_start", "4", "--densify_from_iter", "100", "--quiet", *extra])
    flags = ("--depth_priors", str(priors), "--depth_prior_weight", "0.05", "--depth_prior_local", "0.05", "--depth_prior_patch", "16")
    res, after = {}, {}
    for name, extra in (("plain", ()), ("schedule", flags), ("graph", flags + ("--step", "graph"))):
        res[name] = train.run(args(tmp_path / name, *extra))
        after[name] = random.random()              # where the run left python's generator: the draws of views and shifts
        assert np.isfinite(res[name]["loss"]) and res[name]["points"] > 0
    assert after["plain"] == after["schedule"] == after["graph"]
    assert res["schedule"]["loss"] > res["plain"]["loss"] and res["graph"]["loss"] > res["plain"]["loss"]
    assert res["graph"]["captures"] >= 2 and all(c.depth_prior is not None and c.depth_prior_mask.dtype == torch.uint8
                                                for c in res["graph"]["trainer"].views)
    out = evaluate.run(str(tmp_path / "graph"), depth_priors=str(priors))
    with open(tmp_path / "graph" / "results.json") as fp:
        full = json.load(fp)
    with open(tmp_path / "graph" / "per_view.json") as fp:
        per = json.load(fp)
    method, = full
    assert -1 <= full[method]["DepthPearson"] <= 1 and len(per[method]["DepthPearson"]) == len(per[method]["PSNR"]) >= 1
    assert abs(full[method]["DepthPearson"] - np.mean(list(per[method]["DepthPearson"].values()))) <= 1e-6
    assert abs(out["DepthPearson"] - full[method]["DepthPearson"]) <= 1e-6
    shutil.rmtree(priors)
    os.makedirs(priors)
    with pytest.raises(FileNotFoundError, match=".npy"):
        train.run(args(tmp_path / "missing", *flags))
