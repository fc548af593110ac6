"""GPU: graph_trainer.GraphTrainer -- the reference's iteration (schedule.IterationSchedule) on the fused step, one HIP-graph
replay per iteration -- and `train --step graph`.

  * lockstep against the oracle-backed CPU trainer (tests/ref_schedule.py::Trainer) with the bars of
    test_reference_schedule_lockstep_fused_step_vs_oracle_backed_cpu, unchanged;
  * a replay is a replay: the capture counter stands still between densifications, and run_iteration passes torch's
    synchronisation check set to "error";
  * the CLI end to end on the golden LLFF and DTU folders, resume across the modes;
  * the two modes from one seed, before the schedule's chaos sets in;
  * recovery from a binning capacity that is too small (a capacity event: lists are truncated, nothing faults)."""
import os
import shutil
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ITERS = 500
KW = dict(densify_grad_threshold=0.001, densification_interval=50)     # as tests/test_gpu_reference_schedule.py


class GraphLead:
    """GraphTrainer behind the step() / get_state() / mean_psnr() surface of tests/ref_schedule.py's trainers."""

    def __init__(self, scene, iterations=300, densify_from_iter=60, densification_interval=40, densify_grad_threshold=0.0002,
                 shift_cam_start=100, sh_interval=100, cam_trans_dist=0.4, opacity_decay=0.995, seed=5, **extra):
        import ref_schedule as rs
        from binocular3dgs_amd import synth
        from binocular3dgs_amd.gaussian_model import GaussianModel
        from binocular3dgs_amd.graph_trainer import GraphTrainer
        from binocular3dgs_amd.render import PipelineParams
        from binocular3dgs_amd.scene import Scene
        LR = rs.LR
        i0 = scene["init"]
        self.iterations, self.device = iterations, "cuda"
        m = self.model = GaussianModel.from_tensors(i0["xyz"], i0["features_dc"], i0["features_rest"], i0["scaling"],
                                                    i0["rotation"], i0["opacity"], sh_degree=1, active_sh_degree=0, device="cuda")
        self.cams = synth.synth_cameras(scene["W"], scene["H"], yaws=synth.YAWS_6, device="cuda")[:3]
        self.gts = [g.cuda() for g in scene["gts"]]
        for cam, gt in zip(self.cams, self.gts):
            cam.original_image, cam.gt_alpha_mask = gt, None
        self.bg, self.extent, self.pipe = scene["bg"].cuda(), scene["extent"], PipelineParams()
        m.spatial_lr_scale = self.extent
        m.training_setup(types.SimpleNamespace(
            percent_dense=0.01, position_lr_init=LR["position_lr_init"], position_lr_final=LR["position_lr_final"],
            position_lr_delay_mult=LR["position_lr_delay_mult"], position_lr_max_steps=iterations, feature_lr=LR["feature_lr"],
            opacity_lr=LR["opacity_lr"], scaling_lr=LR["scaling_lr"], rotation_lr=LR["rotation_lr"]))

        def shared_split_noise(it):       # (both lock-step trainers split with the same noise)
            P = m.get_xyz.shape[0]
            m.split_noise = torch.randn(2, P, 3, generator=torch.Generator().manual_seed(1000 + it)).cuda()

        self.events = []
        self.tr = GraphTrainer(m, Scene(self.cams, m, cameras_extent=self.extent), self.pipe, self.bg, iterations=iterations,
                               shift_cam_start=shift_cam_start, binocular=True, opacity_decay_factor=opacity_decay or None,
                               lambda_dssim=0.2, densify_from_iter=densify_from_iter, densify_until_iter=iterations + 1,
                               densification_interval=densification_interval, densify_grad_threshold=densify_grad_threshold,
                               sh_interval=sh_interval, before_densify=shared_split_noise, events=self.events, **extra)
        self.opt = self.tr.backend.opt
        rng = np.random.default_rng(seed)                     # trans_dist sequence shared by all runs
        self.shifts = (rng.random(iterations + 1) * cam_trans_dist) * rng.choice([-1.0, 1.0], iterations + 1)
        self.last_newP = None

    def step(self, it):
        self.tr.densify_until_iter = self.iterations + 1      # (statistics in every iteration, as Trainer.step keeps them)
        loss = self.tr.run_iteration(it, (it - 1) % len(self.cams), float(self.shifts[it]))
        self.last_newP = self.model.get_xyz.shape[0] if self.tr.densified else None
        return float(loss)

    def get_state(self):
        import ref_schedule as rs
        return rs.FusedTrainer.get_state(self)

    def flat_params(self):
        import ref_schedule as rs
        return rs.FusedTrainer.flat_params(self)

    def mean_psnr(self):
        import ref_schedule as rs
        return rs.FusedTrainer.mean_psnr(self)


def test_graph_trainer_lockstep_vs_oracle_backed_cpu():
    """GraphTrainer LEADS, the oracle-backed CPU trainer -- the reference loop statement by statement -- is handed its full
    state before every iteration and both step.  The bars of the fused step's own lockstep test, unchanged: loss 1e-5
    relative (+1e-7), identical Gaussian count after every densification, updated parameters 1e-3 relative L2, PSNR within
    0.01 dB every 20 iterations.  210 iterations: the decay start (60), the binocular start and the SH raise (100), three
    densifications (100, 150, 200).  The state hand-over reads the device between iterations; the iterations themselves are
    replays (the counter is checked)."""
    import ref_schedule as rs
    torch.set_num_threads(8)
    scene = rs.make_scene()
    n = 210
    hip = GraphLead(scene, iterations=ITERS, **KW)
    cpu = rs.Trainer(scene, "cpu", iterations=ITERS, **KW)
    worst_rel, worst_psnr, worst_loss, densified = 0.0, 0.0, 0.0, []
    for it in range(1, n + 1):
        cpu.set_state(hip.get_state())
        lh, lc = hip.step(it), cpu.step(it)
        worst_loss = max(worst_loss, abs(lh - lc) / abs(lc))
        assert abs(lh - lc) <= 1e-5 * abs(lc) + 1e-7, (it, lh, lc)
        assert (hip.last_newP is None) == (cpu.last_newP is None)
        if hip.last_newP is not None:
            assert int(hip.last_newP) == int(cpu.last_newP), (it, hip.last_newP, cpu.last_newP)
            densified.append((it, int(hip.last_newP)))
        a, b = hip.flat_params(), torch.cat([g["params"][0].detach().reshape(-1).cpu() for g in cpu.opt.param_groups])
        assert a.shape == b.shape
        rel = float((a - b).norm() / b.norm())
        worst_rel = max(worst_rel, rel)
        assert rel <= 1e-3, (it, rel)
        if it % 20 == 0:
            d = abs(hip.mean_psnr() - cpu.mean_psnr())
            worst_psnr = max(worst_psnr, d)
            assert d < 0.01, (it, d)
    print(f"lockstep graph trainer: worst loss rel {worst_loss:.2e}, worst rel-L2 {worst_rel:.2e}, worst |dPSNR| "
          f"{worst_psnr:.2e} dB, P after densifications {densified}, captures {hip.tr.captures}")
    assert [i for i, _ in densified] == [100, 150, 200] and densified[-1][1] > densified[0][1]
    assert hip.model.active_sh_degree == 1
    caps = [(e["it"], e["why"]) for e in hip.events if e["event"] == "capture"]
    # single (1), decay on (61), [100: SH raise + densification, eager], pair after it (101), after 150 and 200
    assert caps == [(1, "first use"), (61, "first use"), (101, "densification"), (151, "densification"),
                    (201, "densification")], caps
    assert hip.tr.grown == 0


def test_replay_means_replay_and_reads_nothing():
    """Between densifications the capture counter stands still.  No host read inside an iteration: the device work of an
    iteration IS a captured graph (the technique of test_growth_in_one_graph_reads_nothing: a read-back during the capture
    would have failed it), and what run_iteration does around the replay -- staging the draw into static storage -- runs
    here with torch's synchronisation check set to "error"."""
    import ref_schedule as rs
    scene = rs.make_scene()
    hip = GraphLead(scene, iterations=ITERS, check_every=0x7fffffff, **KW)
    for it in range(1, 100):
        hip.step(it)
    c0 = hip.tr.captures
    hip.step(101)                         # (the schedule's iteration numbers decide the shape: past 100 the pair)
    c1 = hip.tr.captures
    assert c0 == 2 and c1 == 3, (c0, c1)                      # 1..99: single, decay on at 61; 101: the pair, once
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in hip.model.parameters()]
    n0 = len(hip.events)
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(102, 150):
            hip.tr.run_iteration(it, (it - 1) % 3, float(hip.shifts[it]))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert hip.tr.captures == c1
    assert [e["event"] for e in hip.events[n0:]] == ["replay"] * 48
    assert any(not torch.equal(p, q) for p, q in zip(hip.model.parameters(), before))
    assert hip.tr.backend.steps() == 99 + 1 + 48
    hip.tr.settle()
    assert hip.tr.grown == 0


def _train_args(src, out, extra=()):
    from binocular3dgs_amd import train
    return train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "60",
                                      "--shift_cam_start", "20", "--densify_from_iter", "10", "--densification_interval", "10",
                                      "--test_iterations", "40", "--save_iterations", "40", "--checkpoint_iterations", "40",
                                      "--quiet", *extra])


FILES = ("cfg_args", "input.ply", "cameras.json", "point_cloud/iteration_40/point_cloud.ply",
         "point_cloud/iteration_60/point_cloud.ply", "chkpnt40.pth")


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_cli_graph_step_end_to_end_and_resume_across_modes(tmp_path):
    from binocular3dgs_amd import spiral, train
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    out_s, out_g = tmp_path / "out_s", tmp_path / "out_g"
    res_s = train.run(_train_args(src, out_s))
    res_g = train.run(_train_args(src, out_g, ("--step", "graph")))
    assert _tree(out_g) == _tree(out_s) and all(os.path.exists(out_g / f) for f in FILES)          # the same files written
    assert res_g["first_iteration"] == 1 and res_g["iterations"] == 60 and np.isfinite(res_g["loss"]) and res_g["points"] > 0
    assert set(res_g["reports"]) == {40} and set(res_g["reports"][40]) == {"test", "train"}
    assert all(np.isfinite(v) for pair in res_g["reports"][40].values() for v in pair)
    assert res_g["captures"] >= 3 and res_s["captures"] == 0
    assert spiral.read_cfg_args(str(out_g))["step"] == "graph" and spiral.read_cfg_args(str(out_s))["step"] == "schedule"
    # resume graph -> schedule and schedule -> graph
    r1 = train.run(_train_args(src, tmp_path / "g2s", ("--start_checkpoint", str(out_g / "chkpnt40.pth"))))
    r2 = train.run(_train_args(src, tmp_path / "s2g", ("--start_checkpoint", str(out_s / "chkpnt40.pth"), "--step", "graph")))
    for r, folder in ((r1, "g2s"), (r2, "s2g")):
        assert r["first_iteration"] == 41 and np.isfinite(r["loss"]) and r["points"] > 0
        assert os.path.exists(tmp_path / folder / "point_cloud/iteration_60/point_cloud.ply")
        assert not os.path.exists(tmp_path / folder / "point_cloud/iteration_40")
    # the moments travelled: the resumed graph run starts from the checkpoint's step count
    from binocular3dgs_amd import checkpoint
    tup, it = checkpoint.load(str(out_s / "chkpnt40.pth"))
    steps = {int(float(s["step"])) for s in tup[10]["state"].values()}
    assert it == 40 and len(steps) == 1
    assert r2["trainer"].backend.steps() > steps.pop()


def test_cli_graph_step_on_dtu_drives_the_background_mask(tmp_path):
    from binocular3dgs_amd import train
    from binocular3dgs_amd.graph_trainer import Draw
    src = shutil.copytree(os.path.join(GOLD, "scene_dtu", "scan5"), tmp_path / "scan5")
    res = train.run(_train_args(src, tmp_path / "out", ("--dataset_name", "DTU", "-r", "1", "--step", "graph")))
    assert np.isfinite(res["loss"]) and set(res["reports"]) == {40}
    assert all(os.path.exists(tmp_path / "out" / f) for f in FILES)
    tr, scene = res["trainer"], res["scene"]
    cam = scene.getTrainCameras()[0]
    assert cam.bg_mask is not None and cam.gt_alpha_mask is None and cam.bg_mask.sum() > 0
    assert all(k[3] == "bg" for k in tr._graphs)
    # the coverage part of the fused loss on the trainer's own static storage == mean(|alpha| * bg_mask) by torch on the
    # same render; and its gradient reaches the alpha channel exactly where the mask is set
    from binocular3dgs_amd.fused_loss import binocular_loss_fused
    b = tr.backend
    key = (False, 0.0, True, "bg")
    b.stage(Draw(60, 0, None, tr.background, 1e-5, key, False))
    assert torch.equal(b.mask, cam.bg_mask) and torch.equal(b.gt, cam.original_image)
    b._configure(key)
    pkg = b.st._render_views()[0]
    alpha = pkg["rendered_alpha"].detach().clone().requires_grad_(True)
    total, parts = binocular_loss_fused(pkg["render"].detach(), pkg["rendered_depth"].detach(), alpha, b.gt, bg_mask=b.mask,
                                        slot=3, return_parts=True)
    none, parts0 = binocular_loss_fused(pkg["render"].detach(), pkg["rendered_depth"].detach(), alpha.detach(), b.gt, slot=4,
                                        return_parts=True)      # (its own gradient buffers: slot 3's wait for backward)
    want = (alpha.detach().abs() * cam.bg_mask).mean()
    print("coverage part", float(parts[5]), "torch", float(want), "without the mask", float(parts0[5]))
    # (a float32 sum of H*W = 48 terms: at most 48 * 2^-24 = 2.9e-6 relative)
    assert float(want) > 0 and abs(float(parts[5]) - float(want)) <= 3e-6 * float(want) and float(parts0[5]) == 0.0
    assert abs(float(total) - float(none) - float(want)) <= 1e-5 * abs(float(total))
    total.backward()
    g1 = alpha.grad.clone()
    alpha.grad = None
    a2 = alpha.detach().clone().requires_grad_(True)
    binocular_loss_fused(pkg["render"].detach(), pkg["rendered_depth"].detach(), a2, b.gt, slot=4).backward()
    diff = g1 - a2.grad
    assert (diff[cam.bg_mask > 0] != 0).any() and (diff[cam.bg_mask == 0] == 0).all()


def _params(model):
    return torch.cat([p.detach().reshape(-1).cpu() for p in model.parameters()])


def _cross_args(src, out, iters, extra=()):
    from binocular3dgs_amd import train
    return train.parser().parse_args(["-s", str(src), "-m", str(out), "--eval", "--init_points", "sparse", "--iterations", "1000",
                                      "--shift_cam_start", "3", "--densify_from_iter", "500", "--test_iterations", "1000",
                                      "--save_iterations", "1000", "--quiet", "--seed", "7", *extra]), iters


def test_the_two_modes_agree_from_one_seed_before_chaos_sets_in(tmp_path, monkeypatch):
    """--step schedule (the yardstick: the parent's loop) and --step graph from the same seed, densification beyond the run:
    after six iterations, three of them pair iterations, the drawn views and shifts are identical and the parameters agree
    within the 1e-3 relative L2 per step the lockstep tests grant the fused step (six steps: the bound is applied to the
    whole run, i.e. stricter than per step)."""
    from binocular3dgs_amd import graph_trainer, schedule, train
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    n = 6
    draws = {"schedule": [], "graph": []}

    class Stop(Exception):
        pass

    def spy(cls, tag):
        orig = cls.run_iteration

        def run_iteration(self, it, view_index, shift=None):
            if it > n:
                keep["trainer"] = self
                raise Stop()
            draws[tag].append((it, view_index, shift))
            return orig(self, it, view_index, shift)
        monkeypatch.setattr(cls, "run_iteration", run_iteration)

    spy(schedule.IterationSchedule, "schedule")
    spy(graph_trainer.GraphTrainer, "graph")
    got = {}
    for tag in ("schedule", "graph"):
        keep = {}
        args, _ = _cross_args(src, tmp_path / tag, n, ("--step", tag))
        with pytest.raises(Stop):
            train.run(args)
        tr = keep["trainer"]
        if tag == "graph":
            tr.settle()
            assert tr.grown == 0
        torch.cuda.synchronize()
        got[tag] = _params(tr.model)
    assert draws["schedule"] == draws["graph"] and len(draws["graph"]) == n
    assert [d[2] is not None for d in draws["graph"]] == [False] * 3 + [True] * 3
    rel = float((got["graph"] - got["schedule"]).norm() / got["schedule"].norm())
    print(f"cross-mode agreement after {n} iterations: rel L2 {rel:.3e}")
    assert rel <= 1e-3, rel


def test_overflow_recovery_grows_repeats_and_matches_a_roomy_run():
    """The rasterizer's instance capacity is cut to 1000 after construction (as test_step_detects_binning_overflow_and_grows
    does): lists are truncated, the word rises, the steps drop on the device.  The trainer grows, re-captures and repeats;
    the result matches a run that had room, within the lockstep bound."""
    import ref_schedule as rs
    scene = rs.make_scene()
    n = 45

    def run(cut_at):
        hip = GraphLead(scene, iterations=ITERS, check_every=8, **KW)
        for it in range(1, n + 1):
            if it == cut_at:
                fr = hip.tr.backend.fused
                fr.capacity = 1000                           # a scene that outgrew its buffers (a capacity event, no fault)
                for i in range(len(fr.slots)):
                    fr.slots[i] = fr._new_slot(fr.slots[i].stream, i)
                hip.tr._invalidate("test: new slots")        # (the graphs hold the old slots' addresses)
            hip.step(it)
        hip.tr.settle()
        torch.cuda.synchronize()
        return hip

    roomy, tight = run(None), run(20)
    assert roomy.tr.grown == 0 and tight.tr.grown >= 1 and tight.tr.repeated >= 1
    assert tight.tr.backend.fused.capacity > 1000 and tight.tr.backend.check()[0] == 0
    assert tight.tr.backend.steps() == roomy.tr.backend.steps() == n
    over = [e for e in tight.events if e["event"] == "overflow"]
    assert over and over[0]["repeat"][0] == 20 and over[0]["needed"] > 1000
    a, b = tight.flat_params(), roomy.flat_params()
    rel = float((a - b).norm() / b.norm())
    print(f"overflow recovery: grown {tight.tr.grown}, repeated {tight.tr.repeated}, rel L2 vs roomy run {rel:.3e}")
    assert rel <= 1e-3, rel
    # no iteration was counted twice: a Gaussian seen in every iteration has been counted n times in both runs
    assert float(tight.model.denom.max()) == float(roomy.model.denom.max()) == n


def test_a_dropped_cli_trainer_takes_its_graphs_along_without_the_collector(tmp_path):
    """train.run's trainer sits in no reference cycle: with the cyclic collector off, its kept graphs are destroyed when the
    last reference to the result goes.  (torch destroys a captured graph with a device synchronisation, which a capture in
    progress forbids: a trainer left to the collector could take the process down from inside somebody's later capture.)"""
    import gc
    import weakref
    from binocular3dgs_amd import train
    src = shutil.copytree(os.path.join(GOLD, "scene_llff"), tmp_path / "scene_llff")
    gc.collect()
    gc.disable()
    try:
        res = train.run(_train_args(src, tmp_path / "out", ("--step", "graph", "--iterations", "25")))
        graphs = [weakref.ref(c.graph) for c in res["trainer"]._graphs.values()]
        trainer = weakref.ref(res["trainer"])
        assert res["captures"] >= 2 and len(graphs) >= 1 and all(g() is not None for g in graphs)
        del res
        assert trainer() is None and all(g() is None for g in graphs)
    finally:
        gc.enable()
