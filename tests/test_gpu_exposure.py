"""GPU: exposure compensation (csrc/exposure.hip, binocular3dgs_amd/exposure.py) against tests/exposure_ref.py, bit for bit, at
1x1, 16x16 (exactly one block), 257x1 (one pixel into the second block), 37x29 (a partial last block) and 64x40 (ten
workgroups: the arrival fold matters); every call runs twice on the same workspace (the counters reset themselves); both
mutants of the yardstick are told apart.  Then the term inside both trainers and `evaluate --fit_exposure`."""
import json
import os
import types

import numpy as np
import pytest
import torch

import exposure_ref as ref

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (16, 16), (257, 1), (37, 29), (64, 40)]            # (W, H)
DEV = "cuda"


def _rand(seed, W, H):
    rng = np.random.default_rng(seed)
    image = rng.random((3, H, W), dtype=np.float32)
    g_out = (rng.standard_normal((3, H, W)) * 0.1).astype(np.float32)
    A = (np.eye(3, 4) + rng.standard_normal((3, 4)) * 0.2).astype(np.float32)
    return image, g_out, A


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(images, g_outs, mats, rows=None, slot=0):
    """apply + backward through the autograd Function -> (outs, g_ins, matrix grads float32) as numpy"""
    from binocular3dgs_amd.exposure import apply_exposure_batch
    xs = [x.clone().requires_grad_(True) for x in images]
    distinct = {id(m): m for m in mats}
    for m in distinct.values():
        m.requires_grad_(True)
        m.grad = None
    outs = apply_exposure_batch(xs, mats, rows, slot=slot)
    torch.autograd.backward(outs, g_outs)
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], [x.grad.cpu().numpy() for x in xs], [m.grad.cpu().numpy() for m in distinct.values()]


@pytest.mark.parametrize("W,H", SIZES)
def test_apply_and_backward_equal_the_yardstick_bit_for_bit(W, H):
    from binocular3dgs_amd.exposure import exposure_grad
    image, g_out, A = _rand(W * 131 + H, W, H)
    want_out = ref.apply(image, A)
    (want_gin,), want_G = ref.backward([image], [g_out], A)
    slot = ("parity", W, H)
    for _ in range(2):                                                # the second call finds the counters reset
        outs, gins, gA = _run([_t(image)], [_t(g_out)], [_t(A)], slot=slot)
        assert np.array_equal(outs[0], want_out)
        assert np.array_equal(gins[0], want_gin)
        G = exposure_grad(DEV, slot).cpu().numpy()
        assert np.array_equal(G, want_G), np.abs(G - want_G).max()
        assert np.array_equal(gA[0], want_G.astype(np.float32))
    if W * H > 1:
        (mut_gin,), _ = ref.backward([image], [g_out], A, mutant="transposed")
        assert not np.array_equal(gins[0], mut_gin)
    _, mut_G = ref.backward([image], [g_out], A, mutant="no_bias")
    assert not np.array_equal(G, mut_G)


def test_a_batch_of_eight_planes_of_mixed_sizes():
    from binocular3dgs_amd.exposure import exposure_grad
    sizes = SIZES + [(40, 64), (300, 2), (5, 7)]
    data = [_rand(900 + k, W, H) for k, (W, H) in enumerate(sizes)]
    for _ in range(2):
        outs, gins, gAs = _run([_t(d[0]) for d in data], [_t(d[1]) for d in data], [_t(d[2]) for d in data], slot="eight")
        for k, (image, g_out, A) in enumerate(data):
            (want_gin,), want_G = ref.backward([image], [g_out], A)
            assert np.array_equal(outs[k], ref.apply(image, A)), k
            assert np.array_equal(gins[k], want_gin), k
            assert np.array_equal(exposure_grad(DEV, "eight", k).cpu().numpy(), want_G), k
            assert np.array_equal(gAs[k], want_G.astype(np.float32)), k


def test_planes_that_share_a_matrix_get_one_combined_gradient():
    """The trainers' pair: the folds of the two planes added in fp64 in plane order, never two float32 gradients added."""
    from binocular3dgs_amd.exposure import exposure_grad
    (i0, g0, A), (i1, g1, _) = _rand(1, 64, 40), _rand(2, 64, 40)
    (w0, w1), want_G = ref.backward([i0, i1], [g0, g1], A)
    shared = _t(A)
    for _ in range(2):
        outs, gins, gA = _run([_t(i0), _t(i1)], [_t(g0), _t(g1)], [shared, shared], slot="pair")
        assert np.array_equal(gins[0], w0) and np.array_equal(gins[1], w1)
        G = exposure_grad(DEV, "pair").cpu().numpy()
        assert np.array_equal(G, want_G)
        assert len(gA) == 1 and np.array_equal(gA[0], want_G.astype(np.float32))
    _, mut = ref.backward([i0, i1], [g0, g1], A, mutant="no_bias")
    assert not np.array_equal(G, mut)
    (m0, _), _ = ref.backward([i0, i1], [g0, g1], A, mutant="transposed")
    assert not np.array_equal(gins[0], m0)


def test_the_table_form_follows_the_row_word_between_calls():
    from binocular3dgs_amd.exposure import apply_exposure, exposure_grad
    image, g_out, _ = _rand(5, 37, 29)
    rng = np.random.default_rng(6)
    table = (np.eye(3, 4)[None] + rng.standard_normal((4, 3, 4)) * 0.2).astype(np.float32)
    tab, row = _t(table), torch.zeros(1, dtype=torch.int32, device=DEV)
    for r in (2, 0, 3, 3):
        row.fill_(r)
        x = _t(image).requires_grad_(True)
        out = apply_exposure(x, tab, row=row, slot="table")
        out.backward(_t(g_out))
        (want_gin,), want_G = ref.backward([image], [g_out], table[r])
        assert np.array_equal(out.detach().cpu().numpy(), ref.apply(image, table[r])), r
        assert np.array_equal(x.grad.cpu().numpy(), want_gin), r
        assert np.array_equal(exposure_grad(DEV, "table").cpu().numpy(), want_G), r
        (mut,), _ = ref.backward([image], [g_out], table[r], mutant="transposed")
        assert not np.array_equal(x.grad.cpu().numpy(), mut)


def _fit_inputs(seed, W, H):
    rng = np.random.default_rng(seed)
    render = rng.random((3, H, W), dtype=np.float32)
    A = (np.eye(3, 4) * 1.2 + rng.standard_normal((3, 4)) * 0.05).astype(np.float32)
    gt = (ref.apply(render, A) + (rng.standard_normal((3, H, W)) * 0.01).astype(np.float32)).astype(np.float32)
    return render, gt


@pytest.mark.parametrize("W,H", SIZES)
def test_fit_equals_the_yardstick_bit_for_bit(W, H):
    from binocular3dgs_amd.exposure import fit_exposure
    render, gt = _fit_inputs(W * 7 + H, W, H)
    rng = np.random.default_rng(3)
    mask = (rng.random((H, W)) > 0.2).astype(np.uint8)
    for m in (None, mask):
        wantA, want_flag, want_sums = ref.fit(render, gt, m)
        for _ in range(2):
            (A, flag, sums), = fit_exposure([_t(render)], [_t(gt)], None if m is None else [_t(m)], return_sums=True)
            assert np.array_equal(sums.cpu().numpy(), want_sums)
            assert int(flag.item()) == want_flag
            assert np.array_equal(A.cpu().numpy(), wantA)
    assert ref.fit(render, gt, None)[1] == (1 if W * H < 16 else 0)


def test_fit_batch_of_mixed_sizes_with_a_mask_of_fewer_than_sixteen_pixels():
    from binocular3dgs_amd.exposure import fit_exposure
    sizes = SIZES + [(40, 64), (300, 2), (5, 7)]
    data = [_fit_inputs(50 + k, W, H) for k, (W, H) in enumerate(sizes)]
    masks = [None] * len(sizes)
    few = np.zeros((40, 64), np.uint8)
    few.reshape(-1)[::180] = 1                                        # 15 pixels of 2560
    assert int(few.sum()) == 15
    masks[4] = few
    for _ in range(2):
        got = fit_exposure([_t(d[0]) for d in data], [_t(d[1]) for d in data], [None if m is None else _t(m) for m in masks], return_sums=True)
        for k, ((render, gt), m) in enumerate(zip(data, masks)):
            wantA, want_flag, want_sums = ref.fit(render, gt, m)
            assert np.array_equal(got[k][2].cpu().numpy(), want_sums), k
            assert int(got[k][1].item()) == want_flag, k
            assert np.array_equal(got[k][0].cpu().numpy(), wantA), k
    assert int(got[4][1].item()) == 1 and np.array_equal(got[4][0].cpu().numpy(), ref.IDENTITY)
    assert int(got[3][1].item()) == 0 and not np.array_equal(got[3][0].cpu().numpy(), ref.IDENTITY)
    # a constant image: singular, the identity and the flag
    c = np.full((3, 29, 37), 0.25, np.float32)
    (A, flag), = fit_exposure([_t(c)], [_t(c * 2)])
    assert int(flag.item()) == 1 and np.array_equal(A.cpu().numpy(), ref.IDENTITY)


def _term_state(term):
    return dict(table=term.table.cpu().numpy(), exp_avg=term.exp_avg.cpu().numpy(), exp_avg_sq=term.exp_avg_sq.cpu().numpy(),
                steps=term.steps.cpu().numpy(), prods=term.prods.cpu().numpy())


def test_row_sparse_adam_equals_the_yardstick_and_obeys_the_skip_word():
    from binocular3dgs_amd.exposure import ExposureTerm
    term = ExposureTerm(["a", "b", "c"], device=DEV, iterations=100)
    want = ref.new_state(3)
    rng = np.random.default_rng(11)
    skip = torch.zeros(1, dtype=torch.int32, device=DEV)
    G = term.slot.grad(term.device, 0)
    for it, row in enumerate((1, 1, 2, 1, 0, 2), start=1):
        g = rng.standard_normal(12) * 0.3
        G[:12] = _t(g)
        term.stage(row, it)
        term.adam(skip)
        want = ref.adam(want, row, g, term.lr(it), *term.betas, term.eps)
        got = _term_state(term)
        for k in want:
            assert np.array_equal(got[k], want[k]), (it, k)
    assert list(want["steps"]) == [1, 3, 2]
    skip.fill_(1)
    term.stage(0, 7)
    term.adam(skip)
    got = _term_state(term)
    for k in want:                                                    # the raised word: nothing moved, bit for bit
        assert np.array_equal(got[k], want[k]), k
    skip.zero_()
    term.adam(skip)
    assert int(term.steps[0]) == 2


# ---- the trainers ----------------------------------------------------------------------------------------------------------
class Lead:
    """IterationSchedule or GraphTrainer on ref_schedule's synthetic scene (its smallest: the scene of the existing trainer
    tests), built as test_gpu_graph_trainer.GraphLead builds its trainer."""

    def __init__(self, cls, scene, gains=None, iterations=500, exposure=True, **extra):
        import ref_schedule as rs
        from binocular3dgs_amd import synth
        from binocular3dgs_amd.exposure import ExposureTerm
        from binocular3dgs_amd.gaussian_model import GaussianModel
        from binocular3dgs_amd.render import PipelineParams
        from binocular3dgs_amd.scene import Scene
        LR, i0 = rs.LR, scene["init"]
        m = self.model = GaussianModel.from_tensors(i0["xyz"], i0["features_dc"], i0["features_rest"], i0["scaling"], i0["rotation"],
                                                    i0["opacity"], sh_degree=1, active_sh_degree=0, device=DEV)
        self.cams = synth.synth_cameras(scene["W"], scene["H"], yaws=synth.YAWS_6, device=DEV)[:3]
        for k, (cam, gt) in enumerate(zip(self.cams, scene["gts"])):
            cam.original_image, cam.gt_alpha_mask = (gt.cuda() * (1.0 if gains is None else gains[k])).contiguous(), None
            cam.image_name = f"view{k}"
        self.bg = scene["bg"].cuda()
        m.spatial_lr_scale = scene["extent"]
        m.training_setup(types.SimpleNamespace(
            percent_dense=0.01, position_lr_init=LR["position_lr_init"], position_lr_final=LR["position_lr_final"],
            position_lr_delay_mult=LR["position_lr_delay_mult"], position_lr_max_steps=iterations, feature_lr=LR["feature_lr"],
            opacity_lr=LR["opacity_lr"], scaling_lr=LR["scaling_lr"], rotation_lr=LR["rotation_lr"]))
        self.term = ExposureTerm([c.image_name for c in self.cams], device=DEV, iterations=iterations) if exposure else None
        self.events = []
        if cls.__name__ == "GraphTrainer":
            extra = dict(extra, events=self.events)
        self.tr = cls(m, Scene(self.cams, m, cameras_extent=scene["extent"]), PipelineParams(), self.bg, iterations=iterations,
                      shift_cam_start=4, binocular=True, opacity_decay_factor=None, lambda_dssim=0.2, densify_from_iter=10 ** 6,
                      densify_until_iter=10 ** 6, sh_interval=10 ** 6, exposure=self.term, **extra)
        rng = np.random.default_rng(5)
        self.shifts = (rng.random(iterations + 1) * 0.4) * rng.choice([-1.0, 1.0], iterations + 1)
        self.views = rng.integers(0, 3, iterations + 1)

    def run(self, n, first=1):
        for it in range(first, n + 1):
            self.tr.run_iteration(it, int(self.views[it]), float(self.shifts[it]))
        self.tr.settle()
        torch.cuda.synchronize()

    def train_l1(self):
        from binocular3dgs_amd.render import PipelineParams, render
        total = 0.0
        with torch.no_grad():
            for k, cam in enumerate(self.cams):
                img = render(cam, self.model, PipelineParams(), self.bg)["render"]
                if self.term is not None:
                    img = self.term.apply(k, img.contiguous())
                total += float((img - cam.original_image).abs().mean())
        return total / len(self.cams)


def test_schedule_and_graph_agree_on_the_table_and_the_graph_captures_once_per_key():
    """The same draws (the view changes every few iterations) through both trainers: the table rows agree within the rule of
    test_gpu_graph_trainer.py::test_the_two_modes_agree_from_one_seed_before_chaos_sets_in -- 1e-3 relative L2 over the whole
    run of six iterations, three of them pair iterations -- and the graph run captured once per key."""
    import ref_schedule as rs
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    from binocular3dgs_amd.schedule import IterationSchedule
    scene = rs.make_scene()
    n = 6
    sched, graph = Lead(IterationSchedule, scene), Lead(GraphTrainer, scene)
    sched.run(n)
    graph.run(n)
    assert len(set(int(v) for v in graph.views[1:n + 1])) > 1
    a, b = graph.term.table.cpu().double(), sched.term.table.cpu().double()
    assert not torch.equal(b, torch.eye(3, 4, dtype=torch.float64)[None].repeat(3, 1, 1))
    rel = float((a - b).norm() / b.norm())
    relp = float((torch.cat([p.detach().reshape(-1) for p in graph.model.parameters()]).cpu()
                  - torch.cat([p.detach().reshape(-1) for p in sched.model.parameters()]).cpu()).norm())
    print(f"table rows, graph vs schedule after {n} iterations: rel L2 {rel:.3e} (parameters: abs L2 {relp:.3e})")
    assert rel <= 1e-3, rel
    assert torch.equal(graph.term.steps.cpu(), sched.term.steps.cpu())
    caps = [e["key"] for e in graph.events if e["event"] == "capture"]
    assert graph.tr.captures == 2 and len(set(caps)) == 2 and all(k[-1] == "exposure" for k in caps), caps
    assert [e["event"] for e in graph.events if e["event"] != "capture"] == ["replay"] * n


def test_a_run_without_the_term_keeps_its_keys():
    import ref_schedule as rs
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    graph = Lead(GraphTrainer, rs.make_scene(), exposure=False)
    graph.run(6)
    assert all(len(e["key"]) == 4 for e in graph.events if e["event"] in ("capture", "replay"))


def test_row_steps_after_an_overflow_equal_the_draws():
    """The capacity cut of test_gpu_graph_trainer.py::test_overflow_recovery_grows_repeats_and_matches_a_roomy_run (1000
    instances at iteration 20 of 45, check_every 8): the exposure Adam obeys the same word, and after settle() has repeated
    the dropped iterations every row's step count is the number of Adam-carrying iterations that drew its view."""
    import ref_schedule as rs
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    n = 45
    tight = Lead(GraphTrainer, rs.make_scene(), check_every=8)
    for it in range(1, n + 1):
        if it == 20:
            fr = tight.tr.backend.fused
            fr.capacity = 1000
            for i in range(len(fr.slots)):
                fr.slots[i] = fr._new_slot(fr.slots[i].stream, i)
            tight.tr._invalidate("test: new slots")
        tight.tr.run_iteration(it, int(tight.views[it]), float(tight.shifts[it]))
    tight.tr.settle()
    torch.cuda.synchronize()
    assert tight.tr.grown >= 1 and tight.tr.repeated >= 1
    want = np.bincount(tight.views[1:n + 1], minlength=3)
    assert tight.term.steps.cpu().tolist() == want.tolist()
    assert tight.tr.backend.steps() == n


def test_the_term_learns_the_gains_and_lowers_the_training_error():
    """Ground truths scaled by 0.7, 1.0, 1.3; the same draws with and without the term, 150 iterations.  With the term the
    mean diagonal per view is ordered as the gains, and the train-view L1 (exposure applied on the run that has the term) is
    lower.  Measured on the MI355X after 150 iterations: mean diagonals 0.919, 0.991, 1.068; train-view L1 0.072796 with the
    term against 0.121223 without it.  The assertion is the ordering and the strict inequality, not a margin."""
    import ref_schedule as rs
    from binocular3dgs_amd.graph_trainer import GraphTrainer
    scene, gains, n = rs.make_scene(), (0.7, 1.0, 1.3), 150
    on, off = Lead(GraphTrainer, scene, gains), Lead(GraphTrainer, scene, gains, exposure=False)
    on.run(n)
    off.run(n)
    diag = [float(on.term.table[k, :, :3].diagonal().mean()) for k in range(3)]
    l1_on, l1_off = on.train_l1(), off.train_l1()
    print(f"exposure effect after {n} iterations: mean diagonals {diag}, train L1 with {l1_on:.6f} without {l1_off:.6f}")
    assert diag[0] < diag[1] < diag[2], diag
    assert l1_on < l1_off, (l1_on, l1_off)


def test_evaluate_fit_exposure_recovers_a_known_gain(tmp_path, monkeypatch):
    """`evaluate --fit_exposure` on a model trained for 30 iterations on the golden LLFF folder.  Every test photo is scaled
    by the gain 0.5 (a power of two: the scaling itself is exact).  PSNR_exposure > PSNR; the least-squares map is linear in
    the photo, so the fitted diagonal is the gain times the diagonal fitted against the unscaled photo, within the CPU test's
    lstsq bound 64 cond(S) 2^-53 |A|; without the flag results.json has exactly today's keys."""
    import shutil
    from binocular3dgs_amd import evaluate, scene as scene_mod, train
    from binocular3dgs_amd.exposure import fit_exposure
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    src = shutil.copytree(os.path.join(gold, "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "model"
    args = train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "30",
                                      "--save_iterations", "30", "--quiet", "--seed", "7", "--step", "graph", "--exposure"])
    res = train.run(args)
    saved = json.load(open(out / "point_cloud" / "iteration_30" / "exposure.json"))
    assert sorted(saved) == sorted(res["exposure"].names) and all(np.asarray(v).shape == (3, 4) for v in saved.values())
    del res
    gain = {"value": 1.0}
    orig = scene_mod.Scene.from_dataset.__func__

    def scaled(cls, *a, **k):
        sc = orig(cls, *a, **k)
        for cam in sc.getTestCameras():
            cam.original_image = (cam.original_image * gain["value"]).contiguous()
        scaled.cams = sc.getTestCameras()
        return sc
    monkeypatch.setattr(scene_mod.Scene, "from_dataset", classmethod(scaled))
    unscaled = evaluate.run(str(out), str(src), fit_exposure=True)
    gain["value"] = 0.5
    plain = evaluate.run(str(out), str(src))
    keys = json.load(open(out / "results.json"))["ours_30"]
    assert sorted(keys) == ["PSNR", "SSIM"], keys
    assert sorted(json.load(open(out / "per_view.json"))["ours_30"]) == ["PSNR", "SSIM"]
    fitted = evaluate.run(str(out), str(src), fit_exposure=True)
    full = json.load(open(out / "results.json"))["ours_30"]
    per = json.load(open(out / "per_view.json"))["ours_30"]
    assert sorted(full) == ["PSNR", "PSNR_exposure", "SSIM", "SSIM_exposure"], full
    assert full["PSNR"] == keys["PSNR"] and full["SSIM"] == keys["SSIM"]
    print(f"PSNR {full['PSNR']:.4f} -> PSNR_exposure {full['PSNR_exposure']:.4f}")
    assert full["PSNR_exposure"] > full["PSNR"] and fitted["exposure"]["PSNR"] > plain["PSNR"]
    assert sorted(per["exposure"]) == sorted(per["PSNR"])
    cams = scaled.cams
    from binocular3dgs_amd.gaussian_model import GaussianModel
    model = GaussianModel(1)
    model.load_ply(str(out / "point_cloud" / "iteration_30" / "point_cloud.ply"))
    renders = evaluate.render_views(model, cams, torch.zeros(3, device=DEV))
    sums = fit_exposure([r.contiguous() for r in renders], [c.original_image.contiguous() for c in cams], return_sums=True)
    for k, (v0, v1) in enumerate(zip(unscaled["exposure"]["per_view"], fitted["exposure"]["per_view"])):
        A0, A1 = np.asarray(v0["exposure"]), np.asarray(v1["exposure"])
        S, _ = ref.matrix_of_sums(sums[k][2].cpu().numpy())
        bound = 64.0 * np.linalg.cond(S) * 2.0 ** -53 * np.linalg.norm(A1)
        err = np.abs(np.diag(A1[:, :3]) - 0.5 * np.diag(A0[:, :3])).max()
        print(f"view {k}: diagonal {np.diag(A1[:, :3])}, |diag - gain * unscaled diag| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
