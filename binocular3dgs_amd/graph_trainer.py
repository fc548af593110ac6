"""The training iteration of schedule.IterationSchedule (train.py:83-198) on the build's own step, ONE HIP-graph replay per
iteration: FusedRasterizer + ViewShardedStep + binocular_loss_fused + FusedAdam(decay_first=True).

`GraphTrainer` sits on schedule.TrainerBase as IterationSchedule does -- the same keyword surface, the same per-iteration
plan and report point -- and has its `run_iteration(it, view_index, shift)`, so train.run builds
either one and the caller's draws (random.choice, torch.rand(1), random.choice) are the ones the schedule mode consumes.

What a captured graph fixes, and where each per-iteration value therefore lives
    the input view / its shifted partner     camera.CameraPairSlots: 71 floats rewritten in place, one pinned upload
    the shift                                CameraPairSlots.trans_dist_dev (B3gsLossIO::trans_dist_dev)
    the ground-truth image, the mask         copied into static buffers (the mask: schedule.mask_kind -- gt_alpha_mask, else bg_mask)
    the background colour                    three floats of a static block (refreshed when the caller hands in another tensor)
    the depth prior, its validity, the       copied into static buffers next to the mask; the patch offsets: two int32 words
    patch offsets (depth_prior.PriorTerm)    (PriorTerm.offset_buffer) the kernels read, one pinned upload per draw
    the normal prior and its validity        copied into static buffers in the same way (normal_prior.NormalTerm draws nothing)
    the learning rates                       six floats of the same block (B3gsAdamSegment::lr_dev), one pinned upload
    the exposure row and its learning rate   two words of exposure.ExposureTerm's own block (the table, the moments, the step
    (exposure.ExposureTerm)                  counts are static too), one pinned upload; the kernels read the row on the device
No value is read back inside an iteration.

What cannot live in device memory is a SHAPE of the graph, captured at its first use and kept:
    (pair?, opacity decay factor of the Adam launch or 0, statistics on?, mask kind[, "prior"][, "exposure"][, "normal"])
-- single view while `it <= shift_cam_start` or `binocular` is off, the (input, shifted) pair with one depth sort afterwards;
the fifth entry is there while the depth-prior term is active (all training views carry a prior, or none: a mixed set is
refused) and ABSENT otherwise, so a run without priors has the keys, the events and the launches it always had; a trailing
"exposure" is there, in the same way, only while the exposure term is active: the replay then applies the drawn view's row to
the render (and the shifted partner's) in one launch, and runs the row's Adam behind the fused step under the same capacity word;
a trailing "normal", likewise, only while the normal-prior term is active (all training views carry one, or none);
the decay switches on once (`it > densify_from_iter`), the statistics switch off once (`it >= densify_until_iter`, only with
the decay off: with it on, densification runs to the end).  These windows are schedule.TrainerBase.plan, the one place
that decides them for both trainers; "the replay carries Adam" is its `step and not densify`.  Every kept graph is dropped, and captured
again at its next use, exactly when an address or a launch argument changed: after densify_and_prune (P), after
oneupSHdegree raised the degree, after a capacity check changed `seg1_fraction` / the depth-key width or grew the buffers.
`captures` counts them.

Two iterations do not run Adam and are issued eagerly (compute_grads only), as tests/ref_schedule.py::FusedTrainer does:
the densification iteration (the reference replaces every parameter before optimizer.step(), which then finds no gradient:
train.py:180-198) and the last one (train.py:196).  A re-capture follows the first anyway.

ORDER OF THE REFERENCE'S POINTS.  In train.py:100-198 an iteration renders and back-propagates (no state changes), reports
and saves (:166-169), THEN decays the opacities (:171-173), accumulates the statistics, densifies and steps Adam.  The
parameters at the report / save of iteration `it` are therefore the ones iteration `it - 1` left behind, and nothing the
replay of `it` computes is needed for them: training_report and `after_report(it)` run BEFORE the replay of `it` and see the
reference's state; the replay then does decay + statistics + Adam in one go.  A checkpoint (train.py:200-202) follows the
optimiser step: it is written after the replay (train.run does, behind `run_iteration`).

OVERFLOW.  The binning kernels raise a sticky device word when a view needed more tile instances than the
buffers hold.  Read from the code: csrc/binning.hip sets it in the forward of the overflowing step; the chain-rule pass
(csrc/preprocess.hip, B3gsDensifyStats::skip_if_nonzero) and the Adam launch with its step counter (csrc/optim.hip:
adam_kernel, bump_step) return at once while it is set.  So a raised word drops the statistics, the decay, the update and the
step count of the OVERFLOWING iteration AND OF EVERY LATER ONE until the word is cleared; everything before it was applied in
full.  The device step counter says how many that is.  `settle()` -- every `check_every` (32) iterations, before every
densification, report, save and checkpoint, and at the end -- reads the word; when it is raised the buffers are grown, the
graphs dropped, and exactly the dropped iterations are repeated from the remembered draws (view, shift, background,
learning rate).  A run never ends on an overflow it could grow out of.

The model stays a GaussianModel; `model.optimizer` becomes the step's FusedAdam, which checkpoint.capture writes as the
reference's tuple: a checkpoint of either mode resumes in the other.
"""
from __future__ import annotations

import collections
import gc

import torch

from .schedule import TrainerBase, mask_kind

Draw = collections.namedtuple("Draw", "it view shift bg lr key full offset", defaults=(None,))


class _Captured:
    def __init__(self, graph, loss, params):
        self.graph, self.loss, self.params = graph, loss, params

    def replay(self):
        from .step import _bump_versions
        self.graph.replay()
        _bump_versions(self.params)      # (the replay wrote the parameters: render()'s depth-order hint keys on the version)


class FusedBackend:
    """The device side of GraphTrainer: static storage, the step objects, capture and the capacity word."""

    def __init__(self, model, views, background, lambda_dssim=0.2, smooth_weight=0.05, binning_capacity=None, depth_prior=None,
                 exposure=None, normal_prior=None):
        from . import _lib, checkpoint
        from .camera import CameraPairSlots, _PinnedRing
        from .fused import FusedRasterizer
        from .step import FusedAdam, ViewShardedStep
        self.model, self.views = model, list(views)
        self.lam, self.smooth_weight = float(lambda_dssim), float(smooth_weight)
        v0 = self.views[0]
        W, H = v0.image_width, v0.image_height
        for v in self.views:
            if (v.image_width, v.image_height, v.FoVx, v.FoVy) != (W, H, v0.FoVx, v0.FoVy):
                raise _lib.B3gsError("GraphTrainer: the training views must share one image size and field of view (the "
                                     "captured launches carry them); use the schedule step for mixed cameras")
        dev = model.get_xyz.device
        old = model.optimizer
        if isinstance(old, FusedAdam):
            self.opt = old
        else:       # the reference-shaped optimiser of training_setup() / restore(): same state, flat
            g0 = old.param_groups[0]
            by = {g["name"]: float(g["lr"]) for g in old.param_groups}
            self.opt = FusedAdam(model.parameters(), [by[n] for n in checkpoint.MODEL_ORDER], betas=tuple(g0["betas"]),
                                 eps=float(g0["eps"]), opacity_decay=0.0, opacity_index=5, decay_first=True)
            m, v, step, _ = checkpoint._moments_from_state_dict(model, checkpoint.optimizer_state_dict(model, old))
            self.opt.exp_avg.copy_(m)
            self.opt.exp_avg_sq.copy_(v)
            self.opt.step_count.fill_(step)
            model.optimizer = self.opt
        self.block = torch.zeros(16, dtype=torch.float32, device=dev)          # [learning rates (6) | - | background (3) | -]
        self.lr_dev, self.bg = self.block[:6], self.block[8:11]
        self.lr_dev.copy_(torch.tensor(self.opt.lrs, dtype=torch.float32))
        self.bg.copy_(background)
        self._bg_src = background
        self.opt.lr_device = self.lr_dev
        self._ring = _PinnedRing(64, 6)
        self.slots = CameraPairSlots(v0, 0.1)
        self.gt = v0.original_image.to(dev, torch.float32).clone()
        self.mask = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
        # depth_prior.PriorTerm: static prior plane, validity and offset words; every training view carries a prior, or none
        self.prior_term = depth_prior if (depth_prior is not None and depth_prior.enabled) else None
        self.has_prior = False
        if self.prior_term is not None:
            from .depth_prior import check_prior_set
            self.has_prior = check_prior_set(self.views)
        if self.has_prior:
            self.prior = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
            self.prior_mask = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
            self.offset_dev = self.prior_term.offset_buffer(dev)
        self._prior = False
        # exposure.ExposureTerm: its table, moments, row word and learning rate are static device memory of its own
        self.exposure_term = exposure
        self.has_exposure = exposure is not None
        self._exposure = False
        # normal_prior.NormalTerm: static target plane and validity, copied per view like the depth prior; all views or none
        self.normal_term = normal_prior if (normal_prior is not None and normal_prior.enabled) else None
        self.has_normal = False
        if self.normal_term is not None:
            from .normal_prior import check_prior_set as check_normal_set
            self.has_normal = check_normal_set(self.views)
        if self.has_normal:
            self.normal = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
            self.normal_mask = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
        self._normal = False
        self.fused = FusedRasterizer(model, W, H, num_slots=2, want_means2D=False, binning_capacity=binning_capacity)
        self.st = ViewShardedStep(model, [(self.slots.cam, self.slots.shifted, 0.1)], self.bg, optimizer=self.opt,
                                  fused=self.fused, overflow_check_every=0)
        self._both = list(self.st.views)
        self._pair, self._kind = True, None
        self._loss = None
        self.focal_x = v0.get_focal()[0]

    # ---- what the policy asks ------------------------------------------------------------------------------------------
    def steps(self) -> int:
        return int(self.opt.step_count.item())

    def stage(self, d: Draw):
        """The draw into static device storage: uploads and device copies only."""
        cam = self.views[d.view]
        self.slots.set(cam, 0.0 if d.shift is None else float(d.shift))
        self.gt.copy_(cam.original_image, non_blocking=True)
        kind = d.key[3]
        if kind is not None:
            self.mask.copy_(cam.gt_alpha_mask if kind == "alpha" else cam.bg_mask, non_blocking=True)
        if "prior" in d.key[4:]:
            self.prior.copy_(cam.depth_prior, non_blocking=True)
            self.prior_mask.copy_(cam.depth_prior_mask, non_blocking=True)
            self.prior_term.upload_offset(d.offset, self.offset_dev.device)
        if "exposure" in d.key[4:]:
            self.exposure_term.stage(d.view, d.it)
        if "normal" in d.key[4:]:
            self.normal.copy_(cam.normal_prior, non_blocking=True)
            self.normal_mask.copy_(cam.normal_prior_mask, non_blocking=True)
        if d.bg is not self._bg_src:
            self.bg.copy_(d.bg, non_blocking=True)
            self._bg_src = d.bg
        self.opt.lrs[0] = float(d.lr)
        k, row = self._ring.take()
        buf = row.numpy()
        buf[:] = self.opt.lrs
        self.lr_dev.copy_(row, non_blocking=True)
        self._ring.uploaded(k, self.lr_dev.device)

    def _configure(self, key):
        pair, decay, stats, kind = key[:4]
        self._prior, self._exposure, self._normal = "prior" in key[4:], "exposure" in key[4:], "normal" in key[4:]
        v0, v1 = self._both
        self.st.views = [v0, v1] if pair else [v0]
        v0.mate = 1 if pair else None
        self.st.densify_stats = bool(stats)
        self.opt.opacity_decay = float(decay)
        self._pair, self._kind = bool(pair), kind

    def _loss_fn(self, i, cam, pkg, spkg, t):
        from .fused_loss import binocular_loss_fused
        pair, kind = self._pair, self._kind
        image, shifted = pkg["render"], spkg["render"] if pair else None
        if self._exposure:      # the staged row, one apply launch (and one backward launch) for the pair
            if pair:
                image, shifted = self.exposure_term.apply(None, image, shifted)
            else:
                image = self.exposure_term.apply(None, image)
        total = binocular_loss_fused(image, pkg["rendered_depth"], pkg["rendered_alpha"], self.gt,
                                     lambda_dssim=self.lam, shifted_image=shifted,
                                     focal_x=self.focal_x, trans_dist=0.0 if pair else None,
                                     trans_dist_dev=self.slots.trans_dist_dev if pair else None,
                                     gt_alpha_mask=self.mask if kind == "alpha" else None,
                                     bg_mask=self.mask if kind == "bg" else None, lambda_smooth=self.smooth_weight,
                                     slot=0, unit_grad=True)
        if self._prior:
            total = total + self.prior_term.loss(cam, pkg, offset_dev=self.offset_dev, prior=self.prior, mask=self.prior_mask)
        if self._normal:      # (the views share one field of view: the first one's serves the static slot)
            total = total + self.normal_term.loss(self.views[0], pkg, target=self.normal, mask=self.normal_mask)
        self._loss = total.detach()
        return total

    def _state(self):
        m, o = self.model, self.opt
        own = self.exposure_term.state() if self.has_exposure else []
        return list(m.parameters()) + [o.exp_avg, o.exp_avg_sq, o._step_words, m.xyz_gradient_accum, m.denom, m.max_radii2D] + own

    def _step(self):
        """One full step: the fused step, then (while the term is active) the exposure row's Adam under the same capacity
        word -- an overflowing iteration drops both, and settle() repeats both."""
        self.st.step(loss_fn=self._loss_fn)
        if self._exposure:
            self.exposure_term.adam(self.fused.overflow_flag)

    def capture(self, key) -> _Captured:
        """Warm-up steps (they settle every allocation; the last one on a side stream, as a capture wants it), the capture,
        and the state the warm-up moved put back: capturing an iteration does not train."""
        self._configure(key)
        dev = self.model.get_xyz.device
        with torch.no_grad():
            snap = [t.detach().clone() for t in self._state()]
        self._step()
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        # The cyclic collector runs before the capture and stays out of it: a finaliser it ran there could make a call a
        # capture forbids.  The destructor of a torch CUDAGraph is one (on ROCm it synchronises the device, and its check
        # throws from the destructor: the process aborts), so a dropped trainer that sat in a reference cycle with its kept
        # graphs would end this one's capture wherever the collector happened to start.
        gc.collect()
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                self._step()
        finally:
            if collecting:
                gc.enable()
        with torch.no_grad():
            for t, s in zip(self._state(), snap):
                t.copy_(s)
        return _Captured(graph, self._loss, list(self.model.parameters()))

    def replayed(self, captured: _Captured):
        self._loss = captured.loss

    def grads_only(self, key):
        """Forward, loss, backward and the chain-rule pass with the statistics, launched eagerly; no decay, no Adam."""
        self._configure(key)
        self.st.compute_grads(loss_fn=self._loss_fn)

    def loss(self):
        return self._loss

    def check(self):
        """-> (0 | the instances a view needed, the device step counter when the word was raised, did a launch argument
        change).  The only host reads of the trainer."""
        f = self.fused
        before = (f.seg1_fraction, f.depth_key_bits)
        over = f.check_overflow()
        return over, (self.steps() if over else None), before != (f.seg1_fraction, f.depth_key_bits)

    def decay(self, factor):
        self.model.opacity_decay(factor=factor)

    def densify(self, max_grad, min_opacity, extent, noise=None) -> int:
        self.st.views = list(self._both)      # (the buffers are fitted to both views of the pair)
        self._both[0].mate = 1
        return self.st.densify_and_prune(max_grad, min_opacity, extent, None, percent_dense=self.model.percent_dense or 0.01,
                                         noise=noise)


class GraphTrainer(TrainerBase):
    """IterationSchedule's surface (model, scene, pipe, background + the keywords of schedule.TrainerBase) on the
    graph-replayed fused step.  Keywords of its own: `save_iterations` / `checkpoint_iterations` (where `after_report` / the
    caller write files: the capacity word is settled first), `check_every`, `binning_capacity`, `backend` (tests), `events`
    (a list that receives what ran)."""

    def __init__(self, model, scene, pipe, background, *, ops=None, log_item=False, save_iterations=(),
                 checkpoint_iterations=(), check_every=32, binning_capacity=None, backend=None, events=None, **kw):
        if ops is not None or log_item:
            raise ValueError("GraphTrainer runs the fused step: `ops` and `log_item` belong to IterationSchedule")
        super().__init__(model, scene, pipe, background, **kw)
        self.save_iterations, self.checkpoint_iterations = frozenset(save_iterations), frozenset(checkpoint_iterations)
        self.check_every = int(check_every)
        self.backend = backend if backend is not None else FusedBackend(model, self.views, background, self.lam,
                                                                        self.smooth_weight, binning_capacity, self.depth_prior,
                                                                        self.exposure, self.normal_prior)
        self.events = events
        self.captures = 0        # graphs captured so far: a replay does not move it
        self.grown = 0           # capacity events settled
        self.repeated = 0        # iterations repeated after them
        self._graphs = {}
        self._why = "first use"
        self._pending = []       # the draws since the last clean capacity check
        self._mark = self.backend.steps()     # the device step counter at that check

    # ---- bookkeeping ----------------------------------------------------------------------------------------------------
    def _ev(self, what, **kw):
        if self.events is not None:
            self.events.append(dict(kw, event=what))

    def _invalidate(self, why):
        self._graphs.clear()
        self._why = why

    def _run(self, d: Draw):
        b = self.backend
        b.stage(d)
        if d.full:
            g = self._graphs.get(d.key)
            if g is None:
                g = self._graphs[d.key] = b.capture(d.key)
                self.captures += 1
                self._ev("capture", it=d.it, key=d.key, why=self._why)
                self._why = "first use"
            g.replay()
            b.replayed(g)
            self._ev("replay", it=d.it, view=d.view, shift=d.shift, key=d.key)
        else:
            b.grads_only(d.key)
            self._ev("grads", it=d.it, view=d.view, shift=d.shift, key=d.key)
        self._pending.append(d)

    def settle(self):
        """The capacity protocol (module docstring): on a clean word forget the remembered draws; on a raised one grow,
        drop the graphs and repeat exactly the dropped iterations."""
        b = self.backend
        for _ in range(16):
            over, steps_now, changed = b.check()
            if changed:
                self._invalidate("launch arguments")
            if not over:
                self._mark += sum(1 for d in self._pending if d.full)
                self._pending = []
                return
            self._invalidate("capacity")
            applied = steps_now - self._mark          # every Adam-carrying draw before the overflowing one
            dropped, self._pending, self._mark = self._pending[applied:], [], steps_now
            self.grown += 1
            self.repeated += len(dropped)
            self._ev("overflow", needed=over, repeat=[d.it for d in dropped])
            for d in dropped:
                self._run(d)
        from . import _lib
        raise _lib.B3gsError("B3GS_ERR_CAPACITY: the binning buffers kept overflowing after 16 rounds of growing them")

    # ---- the iteration --------------------------------------------------------------------------------------------------
    def run_iteration(self, it: int, view_index: int, shift: float | None = None):
        """-> the total loss of the iteration (a device tensor; nothing is read back)."""
        m, b = self.model, self.backend
        lr = m.xyz_scheduler_args(it)                       # update_learning_rate's schedule; it reaches Adam through lr_dev
        if it % self.sh_interval == 0:
            before = m.active_sh_degree
            m.oneupSHdegree()
            if m.active_sh_degree != before:
                self._invalidate("SH degree")
        plan = self.plan(it)
        adam = plan.step and not plan.densify               # the replay carries Adam; the other iterations run eagerly
        # train.py:166-169 -- before this iteration's replay: the parameters are the ones the reference reports and saves
        if plan.report or it in self.save_iterations:
            self.settle()
        self._report(it, plan)
        if plan.report:
            self._ev("report", it=it)
        if self.after_report is not None:
            self._ev("after_report", it=it)
        key = (plan.pair, float(self.decay) if (plan.decay and adam) else 0.0, plan.stats, mask_kind(self.views[view_index]))
        offset = None
        if getattr(b, "has_prior", False) and self.depth_prior.active(it):
            key, offset = key + ("prior",), self.depth_prior.draw_offset()      # (the term's own generator; kept for a repeat)
        if getattr(b, "has_exposure", False) and self.exposure.active(it):
            key = key + ("exposure",)
        if getattr(b, "has_normal", False) and self.normal_prior.active(it):
            key = key + ("normal",)
        self._run(Draw(it, view_index, float(shift) if plan.pair else None, self.background, lr, key, adam, offset))
        self.densified = False
        if not adam:
            self.settle()                                   # before a densification; and no run ends on a raised word
            if plan.decay:
                b.decay(self.decay)
                self._ev("decay", it=it)
            if plan.densify:
                if self.before_densify is not None:
                    self.before_densify(it)
                noise, m.split_noise = getattr(m, "split_noise", None), None
                self._invalidate("densification")
                b.densify(self.grad_threshold, self.min_opacity, self.scene.cameras_extent, noise)
                self.densified = True
                self._ev("densify", it=it)
        elif len(self._pending) >= self.check_every or it in self.checkpoint_iterations:
            self.settle()
        return b.loss()
