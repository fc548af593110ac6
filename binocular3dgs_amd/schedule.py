"""One training iteration of a Binocular3DGS-style trainer as a sequence of CALLS into pluggable callables.

What is pinned is the contract, not anybody's text: golden G11 (tests/golden/train_trace.json, recorded from the
reference's loop train.py:65-202 with stand-ins for everything it calls) holds, per iteration, the ordered calls, their
argument shapes / constants, which earlier output feeds which later input, and the weights the loss terms carry into
backward().  `IterationSchedule.run_iteration` drives that sequence; tests/test_schedule_trace.py asserts that it produces
G11 event for event when handed the same stand-ins.  With the default `ops` it drives this build's modules (render,
loss_utils, graphics_utils -- each one HIP launch behind the reference's signature), which is what the "unchanged" surface
of bench_ref_schedule.py and the lock-step trainer of tests/ref_schedule.py run.

The DTU background mask (train.py:110-120, 139-143) is driven from the camera: a view that carries a `bg_mask` (computed
once per camera by ground_truth.prepare_ground_truth, not 49 launches per iteration) and no alpha mask adds
mean(|alpha| * bg_mask) to the loss; cameras without the attribute behave as before.  Branches that are configuration, not
call sequence, and are NOT driven here: random backgrounds (the caller hands in `background`), the network GUI, saving
(binocular3dgs_amd/train.py does).  The test-view report of
train.py:226-261 is optional (`test_iterations`, default none): evaluate.training_report at the reference's point of the
iteration, after backward() and before the opacity decay, the densification statistics and optimizer.step().

What an iteration does -- the shifted partner, the report, the decay, the statistics, the densification, the optimiser step
-- is decided in ONE place, `TrainerBase.plan(it)`, for this loop, for mcmc.McmcSchedule (a strategy swapped in through three
hooks) and for graph_trainer.GraphTrainer (the same iteration as one graph replay).
"""
from __future__ import annotations

import collections
import types

import torch


def default_ops():
    """The build's own callables behind the five names the loop uses."""
    from .graphics_utils import inverse_warp_images
    from .loss_utils import SmoothLoss, l1_loss, ssim
    from .render import render
    return types.SimpleNamespace(render=render, l1_loss=l1_loss, ssim=ssim, SmoothLoss=SmoothLoss,
                                 inverse_warp_images=inverse_warp_images)


Plan = collections.namedtuple("Plan", "pair report decay stats densify step")


def mask_kind(cam):
    """Which mask weighs a view's coverage term: "alpha" (its gt_alpha_mask), else "bg" (its DTU bg_mask), else None."""
    if getattr(cam, "gt_alpha_mask", None) is not None:
        return "alpha"
    return "bg" if getattr(cam, "bg_mask", None) is not None else None


class TrainerBase:
    """What IterationSchedule and graph_trainer.GraphTrainer share: the keyword surface and its attributes, `views`,
    `reports`, `densified`, the per-iteration `plan` and the report point.  A densification strategy states two facts."""
    keeps_stats = True                      # the densification statistics are accumulated inside the densification window
    decay_extends_densification = True      # with the opacity decay on, densification runs to the last iteration
    captures = 0                            # HIP graphs captured (GraphTrainer counts them)

    def __init__(self, model, scene, pipe, background, *, iterations=30_000, shift_cam_start=20_000, binocular=True,
                 opacity_decay_factor=0.995, lambda_dssim=0.2, densify_from_iter=500, densify_until_iter=15_000,
                 densification_interval=100, densify_grad_threshold=0.0002, min_opacity=0.005, sh_interval=1000,
                 smooth_weight=0.05, before_densify=None, test_cameras=None, test_iterations=(), report_fn=None,
                 after_report=None, depth_prior=None, exposure=None, normal_prior=None):
        self.model, self.scene, self.pipe, self.background = model, scene, pipe, background
        self.iterations, self.shift_cam_start, self.binocular = iterations, shift_cam_start, binocular
        self.decay, self.lam, self.smooth_weight = opacity_decay_factor, lambda_dssim, smooth_weight
        self.densify_from_iter, self.densify_until_iter = densify_from_iter, densify_until_iter
        self.densification_interval, self.grad_threshold, self.min_opacity = densification_interval, densify_grad_threshold, \
            min_opacity
        self.sh_interval, self.before_densify = sh_interval, before_densify
        # train.py:166 training_report: {iteration: {"test": (l1, psnr), "train": (l1, psnr)}} for every iteration listed
        self.test_cameras, self.test_iterations = list(test_cameras or []), frozenset(test_iterations)
        self.report_fn, self.reports = report_fn, {}
        # depth_prior.PriorTerm or None: a view that carries a `depth_prior` adds the Pearson depth term to the total
        self.depth_prior = depth_prior
        # normal_prior.NormalTerm or None: a view that carries a `normal_prior` adds the loss between the normals of its rendered
        # depth map and the prior (gradients in the rendered depth and alpha); None leaves every call and launch as it was
        self.normal_prior = normal_prior
        # exposure.ExposureTerm or None: the drawn view's render (and its shifted partner's) goes through the view's learned
        # 3x4 colour transform before the loss; None leaves every call, event and launch as it was
        self.exposure = exposure
        self.after_report = after_report    # called with the iteration at train.py:166-169 (the point where it saves)
        self.views = list(scene.getTrainCameras())
        self.densified = False      # did the iteration just run change the Gaussian set?

    def plan(self, it: int) -> Plan:
        """What iteration `it` does.  `densify_until_iter` is read at every call (callers assign it between iterations)
        and, once the decay is on, moved to the last iteration for good."""
        decay = self.decay is not None and it > self.densify_from_iter
        if decay and self.decay_extends_densification:
            self.densify_until_iter = self.iterations
        window = it < self.densify_until_iter
        return Plan(pair=bool(self.binocular and it > self.shift_cam_start), report=it in self.test_iterations, decay=decay,
                    stats=window and self.keeps_stats,
                    densify=window and it > self.densify_from_iter and it % self.densification_interval == 0,
                    step=it < self.iterations)

    def _report(self, it, plan):
        """train.py:166-169: the test-view report of a listed iteration, then the caller's save point."""
        if plan.report:
            if self.report_fn is None:
                from .evaluate import training_report
                self.report_fn = training_report
            self.reports[it] = self.report_fn(self.model, self.test_cameras, self.views, self.background)
        if self.after_report is not None:
            self.after_report(it)

    def settle(self):
        """Nothing is pending between iterations (GraphTrainer: the capacity protocol)."""


class IterationSchedule(TrainerBase):
    """model: update_learning_rate / oneupSHdegree / opacity_decay / add_densification_stats / densify_and_prune /
    optimizer / max_radii2D (the reference's GaussianModel surface); scene: getTrainCameras / getShiftedCamera /
    cameras_extent.  `opacity_decay_factor=None` and `binocular=False` switch the two optional phases off.
    A strategy other than clone / split / prune overrides `_add_loss_terms`, `_densify` and `_after_step` (mcmc.py)."""

    def __init__(self, model, scene, pipe, background, *, ops=None, log_item=False, **kw):
        super().__init__(model, scene, pipe, background, **kw)
        self.ops = ops if ops is not None else default_ops()
        self.log_item = log_item
        H, W = self.views[0].image_height, self.views[0].image_width
        dev = background.device
        # pixel-coordinate grids and the all-ones image whose warp says which pixels the shifted view reaches
        ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
        self.rows, self.cols = ys.contiguous(), xs.contiguous()
        self.ones = torch.ones((1, H, W), dtype=torch.float32, device=dev)
        self.smooth = self.ops.SmoothLoss()
        self.ema = 0.0

    # ---- the terms of the loss --------------------------------------------------------------------------------------
    def _stereo_term(self, cam, first, target, shift, expose=None):
        """Render the partner `shift` along the camera's x axis, warp it back with the primary's depth, compare.
        `expose`: (first render, partner render) -> the two through the view's exposure row (both are compared with the same
        photo); the first is then left in `self._exposed` for the photometric terms."""
        ops = self.ops
        partner = self.scene.getShiftedCamera(cam, shift)
        second = ops.render(partner, self.model, self.pipe, self.background)
        if expose is not None:
            self._exposed, shifted = expose(first["render"], second["render"])
            second = dict(second, render=shifted)
        fx = cam.get_focal()[0]
        disp = (fx * -shift) / (first["rendered_depth"] + 1e-5)
        disp4, target4 = disp[None], target[None]
        warped = ops.inverse_warp_images(second["render"][None], disp4, self.rows, self.cols)
        reach = ops.inverse_warp_images(self.ones[None], disp4, self.rows, self.cols)
        return ops.l1_loss(warped, target4, mask=reach) + self.smooth_weight * self.smooth.forward(disparity=disp * reach,
                                                                                                   image=target4)

    def _add_loss_terms(self, total):
        """-> the reconstruction + stereo + coverage sum with the strategy's own terms added (none here)"""
        return total

    def run_iteration(self, it: int, view_index: int, shift: float | None = None):
        """-> the total loss (attached).  `view_index` / `shift`: the caller's draws (an input view; the signed baseline)."""
        m, ops = self.model, self.ops
        lr_xyz = m.update_learning_rate(it)
        if it % self.sh_interval == 0:
            m.oneupSHdegree()
        plan = self.plan(it)
        cam = self.views[view_index]
        first = ops.render(cam, m, self.pipe, self.background)
        target = cam.original_image.to(self.background.device)
        stereo = 0.0
        # the exposure term (active from its `from_iter`): ONE apply for the render and its shifted partner, whose gradient
        # sums for the view's matrix meet in fp64
        expo = self.exposure if (self.exposure is not None and self.exposure.active(it)) else None
        image = first["render"]
        if plan.pair and expo is not None:
            stereo = self._stereo_term(cam, first, target, float(shift), lambda a, b: expo.apply(view_index, a, b))
            image = self._exposed
        elif plan.pair:
            stereo = self._stereo_term(cam, first, target, float(shift))
        elif expo is not None:
            image = expo.apply(view_index, image)
        coverage = 0.0
        kind = mask_kind(cam)
        if kind is not None:
            coverage = (first["rendered_alpha"].abs() * ((1 - cam.gt_alpha_mask) if kind == "alpha" else cam.bg_mask)).mean()
        photo = ops.l1_loss(image, target)
        recon = (1.0 - self.lam) * photo + self.lam * (1.0 - ops.ssim(image, target))
        total = self._add_loss_terms(recon + stereo + coverage)
        if self.depth_prior is not None:
            total = self.depth_prior.add(total, it, cam, first)
        if self.normal_prior is not None:
            total = self.normal_prior.add(total, it, cam, first)
        total.backward()
        self.densified = False
        with torch.no_grad():
            if self.log_item:
                self.ema = 0.4 * recon.item() + 0.6 * self.ema
            self._after_backward(it, first, plan, lr_xyz)
        return total

    def _after_backward(self, it, first, plan=None, lr_xyz=None):
        """Report, decay, statistics, densification, optimiser step -- in the reference's order.  `lr_xyz`: the position
        learning rate update_learning_rate(it) returned, for `_after_step`."""
        m = self.model
        if plan is None:
            plan = self.plan(it)
        self._report(it, plan)
        if plan.decay:
            m.opacity_decay(factor=self.decay)
        if plan.stats:
            seen = first["visibility_filter"]
            widest = m.max_radii2D
            widest[seen] = torch.max(widest[seen], first["radii"][seen])
            m.add_densification_stats(first["viewspace_points"], seen)
        if plan.densify:
            if self.before_densify is not None:
                self.before_densify(it)
            self._densify(it)
        if plan.step:
            opt = m.optimizer
            opt.step()
            opt.zero_grad(set_to_none=True)
            self._after_step(it, lr_xyz)
            # the exposure row's own Adam, on the iterations whose optimiser step carries gradients (graph_trainer: the
            # replayed ones): not on a densification iteration, not on the last one
            if self.exposure is not None and self.exposure.active(it) and not plan.densify:
                self.exposure.step(it)

    def _densify(self, it):
        self.model.densify_and_prune(self.grad_threshold, self.min_opacity, self.scene.cameras_extent, None)
        self.densified = True

    def _after_step(self, it, lr_xyz):
        pass
