"""GraphTrainer's POLICY without a device: stand-ins for the step / graph / model record what runs.  The same shortened
schedule is driven through schedule.IterationSchedule with recording stand-ins for everything it calls; per iteration both
must do the same things (which views are rendered, report, save point, decay, statistics, densification, optimiser step), in
the reference's order where the order is observable (report and save before anything moves the parameters, the checkpoint
after).  Captures happen at the first use of a shape, after a densification, after an SH raise and after a changed
seg1_fraction / capacity -- never otherwise; an injected overflow word repeats exactly the dropped draws."""
import random
import types

import pytest
import torch

from binocular3dgs_amd.graph_trainer import GraphTrainer
from binocular3dgs_amd.schedule import IterationSchedule

H, W = 6, 8
CFG = dict(iterations=48, shift_cam_start=14, binocular=True, opacity_decay_factor=0.995, lambda_dssim=0.2, densify_from_iter=8,
           densify_until_iter=30, densification_interval=10, densify_grad_threshold=0.0002, sh_interval=25)
TEST_ITERS, SAVE_ITERS, CKPT_ITERS = (20, 33), (20, 48), (33,)


class _Cam:
    def __init__(self, uid, mask=None):
        self.uid, self.image_height, self.image_width = uid, H, W
        self.original_image = torch.full((3, H, W), 0.3)
        self.gt_alpha_mask, self.bg_mask = None, mask

    def get_focal(self):
        return 50.0, 50.0


class _Scene:
    cameras_extent = 2.0

    def __init__(self, cams):
        self.cams = cams

    def getTrainCameras(self):
        return self.cams

    def getShiftedCamera(self, cam, shift):
        return _Cam(("shifted", cam.uid))


class _Model:
    """What both drivers call on `gaussians`; every state-changing method is an event."""

    def __init__(self, log, max_sh=1):
        self.log, self.active_sh_degree, self.max_sh_degree = log, 0, max_sh
        self.max_radii2D = torch.zeros(5)
        self.replaced = False       # densify_and_prune replaced the parameters: optimizer.step() finds no gradient
        self.optimizer = types.SimpleNamespace(step=lambda: None if self.replaced else log.append("adam"),
                                               zero_grad=lambda set_to_none=True: None)
        self.xyz_scheduler_args = lambda it: 1e-4 / it

    def update_learning_rate(self, it):
        self.replaced = False
        return self.xyz_scheduler_args(it)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    def opacity_decay(self, factor):
        self.log.append("decay")

    def add_densification_stats(self, pts, seen):
        self.log.append("stats")

    def densify_and_prune(self, *a):
        self.log.append("densify")
        self.replaced = True


def _schedule_run(draws, mask=False, cls=IterationSchedule, model_cls=_Model, seen=None, **extra):
    """IterationSchedule (or `cls`, a subclass, with its `extra` keywords) over recording stand-ins -> {it: [what happened,
    in order]}; `seen(it, sched, total)` is called after every iteration."""
    log = []
    cams = [_Cam(k, torch.ones(1, H, W) if mask else None) for k in range(3)]
    model = model_cls(log)

    def render(cam, m, pipe, bg):
        log.append("render:shifted" if isinstance(cam.uid, tuple) else f"render:{cam.uid}")
        leaf = lambda *s: torch.full(s, 0.5, requires_grad=True)   # noqa: E731
        return {"render": leaf(3, H, W), "rendered_depth": leaf(1, H, W), "rendered_alpha": leaf(1, H, W),
                "visibility_filter": torch.ones(5, dtype=torch.bool), "radii": torch.ones(5), "viewspace_points": leaf(5, 3)}

    class Smooth:
        def forward(self, disparity, image):
            return disparity.mean()

    ops = types.SimpleNamespace(render=render, l1_loss=lambda a, b, mask=None: (a - b).abs().mean(),
                                ssim=lambda a, b: (a * b).mean(), SmoothLoss=Smooth,
                                inverse_warp_images=lambda img, disp, r, c: img * 1.0 + disp.mean() * 0.0)
    sched = cls(model, _Scene(cams), None, torch.zeros(3), ops=ops, test_cameras=[], test_iterations=TEST_ITERS,
                report_fn=lambda *a: log.append("report") or {}, after_report=lambda it: log.append(
                    "save" if it in SAVE_ITERS else "after_report"), **CFG, **extra)
    out = {}
    for it, view, shift in draws:
        del log[:]
        total = sched.run_iteration(it, view, shift)
        if seen is not None:
            seen(it, sched, total)
        if it in CKPT_ITERS:
            log.append("checkpoint")
        out[it] = list(log)
    return out


class _Backend:
    """The device side as a recorder.  `raise_at`: iteration whose FIRST run raises the sticky capacity word (that step and
    all later ones are dropped until a check clears it); `frac_at`: a check at or after this iteration reports a changed
    seg1_fraction once."""

    def __init__(self, log, cams, raise_at=None, frac_at=None):
        self.log, self.cams, self.raise_at, self.frac_at = log, cams, raise_at, frac_at
        self.word, self.step_count, self.staged, self.last_it = 0, 0, None, 0
        self.applied = []            # (it, view, shift, lr, background) of every step that reached the parameters
        self.stats_applied = []

    def mask_kind(self, k):
        return "bg" if self.cams[k].bg_mask is not None else None

    def steps(self):
        return self.step_count

    def stage(self, d):
        self.staged, self.last_it = d, max(self.last_it, d.it)

    def _forward(self, key):
        d = self.staged
        if d.it == self.raise_at:
            self.word, self.raise_at = 1, None
        self.log.append(f"render:{d.view}")
        if key[0]:
            self.log.append("render:shifted")
        if not self.word and key[2]:
            self.stats_applied.append(d.it)
            self.log.append("stats")

    def capture(self, key):
        self.log.append(("capture", key))
        outer = self

        class G:
            def replay(self):
                outer._forward(key)
                if not outer.word:
                    if key[1]:
                        outer.log.append("decay")
                    outer.log.append("adam")
                    outer.step_count += 1
                    d = outer.staged
                    outer.applied.append((d.it, d.view, d.shift, d.lr, tuple(d.bg.tolist())))
        return G()

    def replayed(self, g):
        pass

    def grads_only(self, key):
        self._forward(key)

    def loss(self):
        return torch.tensor(1.0)

    def check(self):
        self.log.append("check")
        changed = self.frac_at is not None and self.last_it >= self.frac_at
        if changed:
            self.frac_at = None
        over, self.word = self.word, 0
        return (1234 if over else 0), (self.step_count if over else None), changed

    def decay(self, f):
        self.log.append("decay")

    def densify(self, *a):
        self.log.append("densify")


def _graph_run(draws, mask=False, **bk):
    log = []
    cams = [_Cam(k, torch.ones(1, H, W) if mask else None) for k in range(3)]
    model = _Model(log)
    backend = _Backend(log, cams, **bk)
    events = []
    tr = GraphTrainer(model, _Scene(cams), None, torch.zeros(3), backend=backend, events=events, test_cameras=[],
                      test_iterations=TEST_ITERS, report_fn=lambda *a: log.append("report") or {},
                      after_report=lambda it: log.append("save" if it in SAVE_ITERS else "after_report"),
                      save_iterations=SAVE_ITERS, checkpoint_iterations=CKPT_ITERS, check_every=32, **CFG)
    out = {}
    for it, view, shift in draws:
        del log[:]
        tr.background = torch.full((3,), it / 64.0)          # (--random_background: a new colour every iteration)
        tr.run_iteration(it, view, shift)
        if it in CKPT_ITERS:
            log.append("checkpoint")
        out[it] = list(log)
    tr.settle()
    return tr, backend, events, out


def _draws():
    rng = random.Random(4)
    return [(it, rng.randrange(3), (rng.random() * 0.4 * rng.choice([-1.0, 1.0])) if it > CFG["shift_cam_start"] else None)
            for it in range(1, CFG["iterations"] + 1)]


def _semantic(ev):
    """what an iteration did, order-free, without the bookkeeping of either driver"""
    return sorted(e for e in ev if isinstance(e, str) and e not in ("check", "after_report"))


@pytest.mark.parametrize("mask", [False, True])
def test_every_iteration_does_what_the_schedule_does(mask):
    draws = _draws()
    want = _schedule_run(draws, mask)
    tr, backend, events, got = _graph_run(draws, mask)
    for it, _, _ in draws:
        assert _semantic(got[it]) == _semantic(want[it]), (it, got[it], want[it])
        g = [e for e in got[it] if isinstance(e, str)]
        moved = [i for i, e in enumerate(g) if e in ("decay", "adam", "densify")]
        for point in ("report", "save"):                  # before anything moves the parameters: the reference's state
            if point in g:
                assert not moved or g.index(point) < moved[0], (it, g)
        if "checkpoint" in g:
            assert g[-1] == "checkpoint" and "adam" in g and g.index("adam") < g.index("checkpoint")
        w = want[it]                                       # the schedule itself: report / save sit before decay, as recorded
        if "report" in w and "decay" in w:
            assert w.index("report") < w.index("decay")
    # the windows of schedule.TrainerBase.plan were really crossed
    flat = [e for it in got for e in got[it]]
    assert flat.count("densify") == 4 and flat.count("report") == 2 and flat.count("save") == 2
    assert "adam" not in got[CFG["iterations"]] and "adam" not in got[10] and "decay" not in got[8] and "decay" in got[9]
    assert "render:shifted" in got[15] and "render:shifted" not in got[14]
    # a capacity check precedes every densification, report, save and checkpoint, and closes the run
    for it in (10, 20, 30, 40):
        assert got[it].index("check") < got[it].index("densify")
    for it in (20, 33):
        assert got[it].index("check") < got[it].index("report")
    assert got[33][-2] == "check" and got[48].index("check") < got[48].index("save")


def test_a_capture_happens_only_where_an_address_or_a_launch_shape_changes():
    draws = _draws()
    tr, backend, events, got = _graph_run(draws, frac_at=36)
    caps = [(e["it"], e["why"], e["key"]) for e in events if e["event"] == "capture"]
    # iterations 1-8 single/no decay; 9 decay switches on; 10 densifies (eager); 11 re-capture; 15 the pair's first use;
    # 20 densifies; 21; 25 raises the SH degree; 30 densifies; 31; the check of 40 (a densification) reports the changed
    # seg1_fraction AND densifies: one re-capture at 41; 48 is the last iteration (eager)
    assert [(it, why) for it, why, _ in caps] == [
        (1, "first use"), (9, "first use"), (11, "densification"), (15, "first use"), (21, "densification"), (25, "SH degree"),
        (31, "densification"), (41, "densification")]
    assert tr.captures == len(caps)
    assert caps[0][2] == (False, 0.0, True, None) and caps[1][2] == (False, 0.995, True, None) and caps[3][2][0] is True
    replays = [e["it"] for e in events if e["event"] == "replay"]
    assert replays == [it for it in range(1, 48) if it % 10 != 0]              # one replay for every Adam-carrying iteration
    assert [e["it"] for e in events if e["event"] == "grads"] == [10, 20, 30, 40, 48]
    # between two densifications the counter does not move unless one of the listed reasons occurs
    for a, b in ((12, 14), (16, 19), (26, 29), (42, 47)):
        assert not [c for c in caps if a <= c[0] <= b]


def test_a_changed_seg1_fraction_alone_recaptures():
    draws = _draws()
    tr, backend, events, got = _graph_run(draws, frac_at=32)        # the check before the report of iteration 33
    caps = [(e["it"], e["why"]) for e in events if e["event"] == "capture"]
    assert (33, "launch arguments") in caps and tr.captures == 8 + 1


def test_an_overflow_word_repeats_exactly_the_dropped_draws():
    draws = _draws()
    clean, b0, _, _ = _graph_run(draws)
    tr, b1, events, got = _graph_run(draws, raise_at=17)
    over = [e for e in events if e["event"] == "overflow"]
    # the word rises in the forward of 17: 17, 18 and 19 are dropped; the check before the report / save of 20 finds it;
    # 11..16 (since the clean check of 10) were applied and are NOT repeated
    assert len(over) == 1 and over[0]["repeat"] == [17, 18, 19] and tr.grown == 1 and tr.repeated == 3
    assert b1.applied == b0.applied                      # every step reached the parameters once, with its own draws
    assert b1.stats_applied == b0.stats_applied
    caps = [(e["it"], e["why"]) for e in events if e["event"] == "capture"]
    assert (17, "capacity") in caps and tr.captures == clean.captures + 1
    # the repeated iterations ran before the report and the save of iteration 20
    g = got[20]
    assert g.index("check") < g.index("report") < g.index("save") and g.count("adam") == 3 and g.count("densify") == 1
    # a word raised in an eager iteration (the densification of 30) drops its statistics: it is repeated before densifying
    tr3, b3, ev3, got3 = _graph_run(draws, raise_at=30)
    assert [e["repeat"] for e in ev3 if e["event"] == "overflow"] == [[30]] and b3.stats_applied == b0.stats_applied
    assert got3[30].count("densify") == 1 and got3[30].index("stats") < got3[30].index("densify")
    # a word raised in the last iteration is settled before the run ends
    tr2, b2, ev2, _ = _graph_run(draws, raise_at=48)
    assert [e["repeat"] for e in ev2 if e["event"] == "overflow"] == [[48]] and b2.word == 0


class _McmcModel(_Model):
    """_Model with what McmcSchedule reads besides: P rows, their opacities and scales"""

    def __init__(self, log):
        super().__init__(log)
        self.get_xyz = torch.zeros(5, 3)
        self.get_opacity = torch.linspace(0.05, 0.9, 5)[:, None]
        self.get_scaling = torch.linspace(0.01, 0.7, 15).reshape(5, 3)


def test_mcmc_schedule_swaps_the_strategy_and_nothing_else(monkeypatch):
    """McmcSchedule over the stand-ins of IterationSchedule's run above, its three device calls replaced by recorders: per
    iteration the same renders, report and save points and decay as the schedule; relocate + grow inside
    (densify_from_iter, densify_until_iter) only -- the decay does not extend that window; no statistics; the noise right
    after every optimiser step with that iteration's position learning rate; the total is the schedule's plus the
    regulariser, added last."""
    from binocular3dgs_amd import mcmc
    draws = _draws()
    P, cap, seed, o_reg, s_reg = 5, 64, 9, 0.02, 0.03
    grown = {10: 6, 20: 5}                 # what grow() answers: P moved at 10, not at 20
    base, plain_totals, totals, densified, noise = {}, {}, {}, {}, {}

    def relocate(model, optimizer, *, iteration, seed, min_opacity, debug):
        model.log.append("relocate")
        return ("relocated", iteration) if debug else None

    def grow(model, optimizer, cap_max, *, iteration, seed, min_opacity):
        assert cap_max == cap
        model.log.append("grow")
        return grown[iteration]

    def inject_noise(model, lr_xyz, *, iteration, seed, noise_lr):
        model.log.append("noise")
        noise[iteration] = (lr_xyz, iteration, seed, noise_lr)

    monkeypatch.setattr(mcmc, "relocate", relocate)
    monkeypatch.setattr(mcmc, "grow", grow)
    monkeypatch.setattr(mcmc, "inject_noise", inject_noise)

    want = _schedule_run(draws, mask=True, seen=lambda it, s, total: plain_totals.__setitem__(it, total.detach()))

    def seen(it, sched, total):
        totals[it], densified[it] = total.detach(), sched.densified
        base.setdefault("sched", sched)
    got = _schedule_run(draws, mask=True, cls=mcmc.McmcSchedule, model_cls=_McmcModel, seen=seen, cap_max=cap, seed=seed,
                        noise_lr=123.0, opacity_reg=o_reg, scale_reg=s_reg, log_relocations=True)
    sched = base["sched"]
    last = CFG["iterations"]
    for it, _, _ in draws:
        g, w = got[it], want[it]
        assert ("relocate" in g, "grow" in g) == ((it in (10, 20)),) * 2, (it, g)
        if it in (10, 20):
            assert g.index("relocate") + 1 == g.index("grow")
        assert "densify" not in g and ("densify" in w) == (it in (10, 20, 30, 40)), (it, g, w)
        assert "stats" not in g, (it, g)
        assert ("decay" in g) == (it >= 9), (it, g)
        if it < last:
            assert g.count("adam") == 1 and g.count("noise") == 1 and g.index("adam") + 1 == g.index("noise"), (it, g)
            assert noise[it] == (1e-4 / it, it, seed, 123.0)
        else:
            assert "adam" not in g and "noise" not in g and it not in noise
        assert ("report" in g) == (it in TEST_ITERS) and ("save" in g) == (it in SAVE_ITERS), (it, g)
        for point in ("report", "save"):
            if point in g and "decay" in g:
                assert g.index(point) < g.index("decay"), (it, g)
        assert ("render:shifted" in g) == (it >= 15), (it, g)
        # everything the strategy does not own is the schedule's, in the schedule's order (the optimiser step: above)
        own = ("relocate", "grow", "noise", "densify", "stats", "adam")
        assert [e for e in g if e not in own] == [e for e in w if e not in own], (it, g, w)
        m = sched.model
        reg = o_reg * m.get_opacity.mean() + s_reg * m.get_scaling.mean()
        assert float(totals[it]) == float(plain_totals[it] + reg), (it, float(totals[it]), float(plain_totals[it] + reg))
        assert densified[it] == (it in grown and grown[it] != P), it
    # (on a densification iteration the schedule's optimiser step finds no gradient; MCMC's does step)
    for it in (10, 20):
        assert "adam" in got[it] and "adam" not in want[it]
    assert sorted(sched.relocation_log) == [10, 20] and sched.relocation_log[10] == ("relocated", 10)
    assert sched.seed == seed and sched.densify_until_iter == CFG["densify_until_iter"]
