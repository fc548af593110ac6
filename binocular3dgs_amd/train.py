"""python -m binocular3dgs_amd.train -s SOURCE_PATH -m MODEL_PATH [--eval --n_views 3 --dataset_name LLFF ...]

The reference's train.py: a COLMAP / Blender dataset folder in, a trained model out.

    Scene.from_dataset     readers on the host, ground truth (and the DTU background mask) prepared on the device
    IterationSchedule      the iteration of train.py:65-202, every statement a HIP launch of this build (--step schedule)
    GraphTrainer           the same iteration on the fused step, one HIP-graph replay per iteration (--step graph); the draws,
                           reports, saves and checkpoints are the same, a checkpoint of one mode resumes in the other
    per iteration          random.choice(views); past --shift_cam_start: torch.rand(1) * cam_trans_dist and a random sign
                           (train.py:92,125-126, the same draws from the same generators)
    --test_iterations      evaluate.training_report's "[ITER n] Evaluating test|train: L1 .. PSNR .." lines
    --save_iterations      <model_path>/point_cloud/iteration_<n>/point_cloud.ply (before the optimiser step, as there)
    --checkpoint_iterations / --start_checkpoint   <model_path>/chkpnt<n>.pth (checkpoint.py: the reference's tuple)
    --depth_priors DIR     <image_name>.npy depth (or inverse-depth) priors of the training views: the Pearson depth loss of
                           depth_prior.py (both --step modes; --depth_prior_mode depth|disparity, --depth_prior_weight, --depth_prior_local with
                           --depth_prior_patch, --depth_prior_from / --depth_prior_until, --depth_prior_alpha_min)
    --normal_priors DIR    <image_name>.npy | .png normal priors of the training views (any monocular normal network): the loss of
                           normal_prior.py between the normals of the rendered depth map and the prior (both --step modes, both
                           --densify strategies; --normal_prior_frame opencv|opengl|world, --normal_prior_cos, --normal_prior_l1,
                           --normal_prior_from / --normal_prior_until, --normal_prior_alpha_min)
    --exposure             a learned 3x4 affine colour transform per training image (exposure.ExposureTerm: upstream 3DGS's
                           exposure compensation), applied to the render before the loss; --exposure_lr_init / --exposure_lr_final,
                           --exposure_from IT; exposure.json next to every saved point cloud, chkpnt<n>.exposure.pth next to
                           every checkpoint (the reference's checkpoint tuple is untouched)
    --densify adc|mcmc     adc (default): the reference's clone / split / prune; mcmc: mcmc.McmcSchedule -- relocation, growth to
                           --cap_max and position noise (--noise_lr, --opacity_reg, --scale_reg); --step schedule only

<model_path>/cfg_args holds the Namespace(...) line the reference writes; `python -m binocular3dgs_amd.spiral -m MODEL_PATH`
and evaluate.write_results read the result without further arguments.  No progress bar, no tensorboard, no network GUI.
`run(args)` is the importable form: `run(parser().parse_args([...]))`.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import uuid

import numpy as np
import torch


def parser() -> argparse.ArgumentParser:
    """The flags of the reference's train.py that mean something here, with its defaults (arguments/__init__.py,
    train.py:264-281)."""
    p = argparse.ArgumentParser(description="train a Binocular3DGS model from a dataset folder")
    g = p.add_argument_group("loading")
    g.add_argument("--sh_degree", type=int, default=1)
    g.add_argument("--source_path", "-s", type=str, default="")
    g.add_argument("--model_path", "-m", type=str, default="")
    g.add_argument("--images", "-i", type=str, default="images")
    g.add_argument("--resolution", "-r", type=int, default=-1)
    g.add_argument("--white_background", "-w", action="store_true", default=False)
    g.add_argument("--data_device", type=str, default="cuda")
    g.add_argument("--eval", action="store_true", default=False)
    g.add_argument("--init_points", type=str, default="matcher",
                   help='"matcher" (the dense matcher\'s cloud, the reference\'s rule), "sparse" (COLMAP points3D) or a PLY path')
    g = p.add_argument_group("optimisation")
    g.add_argument("--iterations", type=int, default=30_000)
    g.add_argument("--position_lr_init", type=float, default=0.00016)
    g.add_argument("--position_lr_final", type=float, default=0.0000016)
    g.add_argument("--position_lr_delay_mult", type=float, default=0.01)
    g.add_argument("--position_lr_max_steps", type=int, default=30_000)
    g.add_argument("--feature_lr", type=float, default=0.0025)
    g.add_argument("--opacity_lr", type=float, default=0.05)
    g.add_argument("--scaling_lr", type=float, default=0.005)
    g.add_argument("--rotation_lr", type=float, default=0.001)
    g.add_argument("--percent_dense", type=float, default=0.01)
    g.add_argument("--lambda_dssim", type=float, default=0.2)
    g.add_argument("--densification_interval", type=int, default=100)
    g.add_argument("--opacity_reset_interval", type=int, default=3000)
    g.add_argument("--densify_from_iter", type=int, default=500)
    g.add_argument("--densify_until_iter", type=int, default=15_000)
    g.add_argument("--densify_grad_threshold", type=float, default=0.0002)
    g.add_argument("--random_background", action="store_true", default=False)
    p.add_argument("--test_iterations", nargs="+", type=int, default=[30_000])
    p.add_argument("--save_iterations", nargs="+", type=int, default=[30_000])
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[])
    p.add_argument("--start_checkpoint", type=str, default=None)
    p.add_argument("--opacity_decay", action="store_true", default=True)
    p.add_argument("--opacity_decay_factor", type=float, default=0.995)
    p.add_argument("--cam_trans_dist", type=float, default=0.4)
    p.add_argument("--binocular_consistency", action="store_true", default=True)
    p.add_argument("--shift_cam_start", type=int, default=20000)
    p.add_argument("--dataset_name", type=str, default="LLFF")
    p.add_argument("--n_views", type=int, default=3)
    p.add_argument("--suffix", type=str, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--step", choices=("schedule", "graph"), default="schedule",
                   help='"schedule": the reference-shaped loop, one launch per statement (schedule.IterationSchedule); "graph": '
                        'the same iteration on the fused step, one HIP-graph replay per iteration (graph_trainer.GraphTrainer)')
    p.add_argument("--densify", choices=("adc", "mcmc"), default="adc",
                   help='"adc": clone / split / prune by the gradient threshold (the reference\'s rule); "mcmc": relocation, growth '
                        'to --cap_max and position noise (mcmc.McmcSchedule)')
    p.add_argument("--cap_max", type=int, default=None, help="--densify mcmc: the final number of Gaussians")
    p.add_argument("--noise_lr", type=float, default=5e5)
    p.add_argument("--opacity_reg", type=float, default=0.01)
    p.add_argument("--scale_reg", type=float, default=0.01)
    p.add_argument("--depth_priors", default=None, help="folder of <image_name>.npy priors (float32 / float64 [H,W], any size; "
                                                        "<image_name>_mask.png optional) for the training views")
    p.add_argument("--depth_prior_mode", choices=("depth", "disparity"), default="depth",
                   help='"disparity": the prior is an inverse depth (MiDaS / DepthAnything output)')
    p.add_argument("--depth_prior_weight", type=float, default=0.0, help="weight of 1 - rho over the whole image")
    p.add_argument("--depth_prior_local", type=float, default=0.0, help="weight of the mean of 1 - rho over the patches")
    p.add_argument("--depth_prior_patch", type=int, default=64, help="patch size of the local term, 8 .. 256")
    p.add_argument("--depth_prior_from", type=int, default=0)
    p.add_argument("--depth_prior_until", type=int, default=None)
    p.add_argument("--depth_prior_alpha_min", type=float, default=0.0, help="pixels with rendered alpha below this are not used")
    p.add_argument("--normal_priors", default=None, help="folder of <image_name>.npy (float32 / float64 [H,W,3] or [3,H,W], any size) or "
                                                         "<image_name>.png (8-bit RGB, n = 2 c / 255 - 1) normal priors for the "
                                                         "training views; <image_name>_mask.png optional")
    p.add_argument("--normal_prior_frame", choices=("opencv", "opengl", "world"), default="opencv",
                   help='the frame the files hold: "opencv" x right, y down, z forward; "opengl" x right, y up, z backward; "world"')
    p.add_argument("--normal_prior_cos", type=float, default=0.0, help="weight of the mean of 1 - n.t")
    p.add_argument("--normal_prior_l1", type=float, default=0.0, help="weight of the mean of |n - t|_1")
    p.add_argument("--normal_prior_from", type=int, default=0)
    p.add_argument("--normal_prior_until", type=int, default=None)
    p.add_argument("--normal_prior_alpha_min", type=float, default=0.5,
                   help="pixels with rendered alpha below this (or next to one) carry no normal; > 0")
    p.add_argument("--exposure", action="store_true", help="learn a 3x4 affine colour transform per training image")
    p.add_argument("--exposure_lr_init", type=float, default=0.01)
    p.add_argument("--exposure_lr_final", type=float, default=0.001)
    p.add_argument("--exposure_from", type=int, default=0, metavar="IT", help="the first iteration the transform is applied in")
    return p


def exposure_sidecar(checkpoint_path: str) -> str:
    """chkpnt<n>.pth -> chkpnt<n>.exposure.pth"""
    root, ext = os.path.splitext(checkpoint_path)
    return root + ".exposure" + (ext or ".pth")


def check_args(args) -> None:
    """The rules between the flags; ValueError with the reason."""
    wg, wl = getattr(args, "depth_prior_weight", 0.0) or 0.0, getattr(args, "depth_prior_local", 0.0) or 0.0
    if (wg != 0.0 or wl != 0.0) and not getattr(args, "depth_priors", None):
        raise ValueError("--depth_prior_weight / --depth_prior_local need --depth_priors DIR, the folder of the priors")
    if wl != 0.0 and not 8 <= getattr(args, "depth_prior_patch", 64) <= 256:
        raise ValueError("--depth_prior_local needs --depth_prior_patch in 8 .. 256")
    nc, nl = getattr(args, "normal_prior_cos", 0.0) or 0.0, getattr(args, "normal_prior_l1", 0.0) or 0.0
    if (nc != 0.0 or nl != 0.0) and not getattr(args, "normal_priors", None):
        raise ValueError("--normal_prior_cos / --normal_prior_l1 need --normal_priors DIR, the folder of the priors")
    if not getattr(args, "normal_prior_alpha_min", 0.5) > 0.0:
        raise ValueError("--normal_prior_alpha_min is > 0 (the normal comes from depth / alpha)")
    if getattr(args, "exposure", False):
        if not (getattr(args, "exposure_lr_init", 0.01) > 0.0 and getattr(args, "exposure_lr_final", 0.001) > 0.0):
            raise ValueError("--exposure_lr_init and --exposure_lr_final are > 0 (the schedule is log-linear)")
        if getattr(args, "exposure_from", 0) < 0:
            raise ValueError("--exposure_from IT needs IT >= 0")
    elif any(getattr(args, k, d) != d for k, d in (("exposure_lr_init", 0.01), ("exposure_lr_final", 0.001), ("exposure_from", 0))):
        raise ValueError("--exposure_lr_init / --exposure_lr_final / --exposure_from need --exposure")
    if getattr(args, "densify", "adc") != "mcmc":
        return
    if getattr(args, "cap_max", None) is None or args.cap_max < 1:
        raise ValueError("--densify mcmc requires --cap_max N, the final number of Gaussians (N >= 1)")
    if getattr(args, "step", "schedule") == "graph":
        raise ValueError("--densify mcmc --step graph is not supported: the noise launch and the regulariser are not part of "
                         "the captured step yet; use --step schedule")


def cfg_args_text(args) -> str:
    """The line the reference writes to <model_path>/cfg_args (spiral.read_cfg_args parses it)"""
    return str(argparse.Namespace(**vars(args)))


def run(args) -> dict:
    """Trains; -> {"model_path", "first_iteration", "iterations", "loss" (the last total loss), "points", "reports",
    "captures" (graphs captured by --step graph; 0 in schedule mode)}."""
    from . import checkpoint
    from .gaussian_model import GaussianModel
    from .render import PipelineParams
    from .scene import Scene
    from .schedule import IterationSchedule
    args = argparse.Namespace(**vars(args))
    check_args(args)
    say = (lambda *a, **k: None) if args.quiet else print
    args.source_path = os.path.abspath(args.source_path)
    args.save_iterations = list(args.save_iterations) + [args.iterations]
    if not args.model_path:
        args.model_path = os.path.join("./output/", str(uuid.uuid4())[0:10])
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    say("Output folder: {}".format(args.model_path))
    os.makedirs(args.model_path, exist_ok=True)
    with open(os.path.join(args.model_path, "cfg_args"), "w") as fp:
        fp.write(cfg_args_text(args))

    dev = torch.device("cuda")
    model = GaussianModel(args.sh_degree)
    scene = Scene.from_dataset(args.source_path, model, images=args.images, eval=args.eval, n_views=args.n_views,
                               dataset_name=args.dataset_name, suffix=args.suffix, resolution=args.resolution,
                               white_background=args.white_background, init_points=args.init_points,
                               model_path=args.model_path, device=dev, depth_priors=getattr(args, "depth_priors", None),
                               normal_priors=getattr(args, "normal_priors", None),
                               normal_prior_frame=getattr(args, "normal_prior_frame", "opencv"))
    model.training_setup(args)
    first_iter = 0
    if args.start_checkpoint:
        model_params, first_iter = checkpoint.load(args.start_checkpoint)
        model.restore(model_params, args)
    background = torch.tensor([1, 1, 1] if args.white_background else [0, 0, 0], dtype=torch.float32, device=dev)
    exposure = None
    if getattr(args, "exposure", False):
        from .exposure import ExposureTerm
        exposure = ExposureTerm([c.image_name for c in scene.getTrainCameras()], device=dev, lr_init=args.exposure_lr_init,
                                lr_final=args.exposure_lr_final, iterations=args.iterations, from_iter=args.exposure_from)
        # (a checkpoint written without --exposure has no sidecar: the term then starts from the identity)
        if args.start_checkpoint and os.path.isfile(exposure_sidecar(args.start_checkpoint)):
            exposure.load_state_dict(torch.load(exposure_sidecar(args.start_checkpoint), map_location="cpu"))

    def after_report(it):
        # (`reports`, not the trainer: a closure that named its trainer would tie the two into a reference cycle, and the
        # trainer's kept graphs would then be destroyed wherever the cyclic collector ran, e.g. inside a later capture)
        for name, (l1, psnr) in reports.get(it, {}).items():
            say("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(it, name, l1, psnr))
        if it in args.save_iterations:
            say("\n[ITER {}] Saving Gaussians".format(it))
            scene.save(it)
            if exposure is not None:
                from .exposure import write_matrices
                write_matrices(os.path.join(args.model_path, "point_cloud", "iteration_{}".format(it), "exposure.json"),
                               exposure.matrices())

    kw = dict(iterations=args.iterations, shift_cam_start=args.shift_cam_start, binocular=args.binocular_consistency,
              opacity_decay_factor=args.opacity_decay_factor if args.opacity_decay else None,
              lambda_dssim=args.lambda_dssim, densify_from_iter=args.densify_from_iter,
              densify_until_iter=args.densify_until_iter, densification_interval=args.densification_interval,
              densify_grad_threshold=args.densify_grad_threshold, test_cameras=scene.getTestCameras(),
              test_iterations=args.test_iterations, after_report=after_report)
    if getattr(args, "depth_priors", None):
        from .depth_prior import PriorTerm
        # (its own generator: the view and shift draws below do not move when the term is switched on)
        kw["depth_prior"] = PriorTerm(mode=args.depth_prior_mode, weight=args.depth_prior_weight, local=args.depth_prior_local,
                                      patch=args.depth_prior_patch, from_iter=args.depth_prior_from, until_iter=args.depth_prior_until,
                                      alpha_min=args.depth_prior_alpha_min, seed=args.seed)
    if getattr(args, "normal_priors", None):
        from .normal_prior import NormalTerm
        kw["normal_prior"] = NormalTerm(cos=args.normal_prior_cos, l1=args.normal_prior_l1, from_iter=args.normal_prior_from,
                                        until_iter=args.normal_prior_until, alpha_min=args.normal_prior_alpha_min)
    if exposure is not None:
        kw["exposure"] = exposure
    if getattr(args, "step", "schedule") == "graph":
        from .graph_trainer import GraphTrainer
        sched = GraphTrainer(model, scene, PipelineParams(), background, save_iterations=args.save_iterations,
                             checkpoint_iterations=args.checkpoint_iterations, **kw)
    elif getattr(args, "densify", "adc") == "mcmc":
        from .mcmc import McmcSchedule
        sched = McmcSchedule(model, scene, PipelineParams(), background, cap_max=args.cap_max, seed=args.seed, noise_lr=args.noise_lr,
                             opacity_reg=args.opacity_reg, scale_reg=args.scale_reg, **kw)
    else:
        sched = IterationSchedule(model, scene, PipelineParams(), background, **kw)
    reports = sched.reports
    views = sched.views
    loss = None
    for it in range(first_iter + 1, args.iterations + 1):
        cam = random.choice(views)
        sched.background = torch.rand((3), device=dev) if args.random_background else background
        shift = None
        if args.binocular_consistency and it > args.shift_cam_start:
            shift = torch.rand(1) * args.cam_trans_dist
            shift = (shift * random.choice([-1.0, 1.0])).item()
        loss = sched.run_iteration(it, views.index(cam), shift)
        if it in args.checkpoint_iterations:
            say("\n[ITER {}] Saving Checkpoint".format(it))
            checkpoint.save(args.model_path + "/chkpnt" + str(it) + ".pth", model, model.optimizer, it)
            if exposure is not None:
                torch.save(exposure.state_dict(), exposure_sidecar(args.model_path + "/chkpnt" + str(it) + ".pth"))
    sched.settle()
    say("\nTraining complete.")
    return {"model_path": args.model_path, "first_iteration": first_iter + 1, "iterations": args.iterations,
            "loss": None if loss is None else float(loss.detach()), "points": int(model.get_xyz.shape[0]), "reports": dict(sched.reports),
            "scene": scene, "model": model, "captures": sched.captures, "trainer": sched, "exposure": exposure}


def main(argv=None) -> int:
    p = parser()
    args = p.parse_args(argv)
    try:
        check_args(args)
    except ValueError as e:
        p.error(str(e))
    say = (lambda *a: None) if args.quiet else print
    say("Optimizing " + args.model_path)
    run(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
