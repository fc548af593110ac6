"""Held-out view evaluation: batched renders and on-device metrics.

The reference does two things with a trained scene besides training it:

    train.py:226-261      training_report   test views + 5 train views at --test_iterations: mean L1 and PSNR
    render.py:24-49 +     renders to PNG, then SSIM / PSNR / LPIPS per view (DTU object masks), results.json +
    metrics.py:37-124     per_view.json

Here both run on the device without a round trip through files:
  * render_views() renders up to 8 views per b3gs_forward_raw_batch launch through a FusedRasterizer that evaluation owns
    (its own slots, binning buffers, overflow / high-water words and open-tile prediction: the training rasterizer is never
    touched), without gradients, one-round binning and the full 32-bit depth sort;
  * the metric sums of every view of a launch come from ONE b3gs_image_metrics_batch (csrc/metrics.hip: clamp or 8-bit
    round trip, mask composite, fp64 sums, fixed-order fold), the SSIM of all of them from one b3gs_ssim_forward.
The host reads the device once per render batch (the overflow word) and once at the end (the sums).

Two numbers that are easy to confuse:
  * training_report's PSNR (mode "report") is image_utils.psnr on a 3-D [3,H,W] tensor: the MEAN OF THE THREE
    PER-CHANNEL PSNRs, of images clamped to [0,1];
  * metrics.py's PSNR (mode "png") takes the masked branch of image_utils.psnr: one MSE over every element whose mask is
    exactly 1, of images that went through the 8-bit PNG round trip and the mask composite.  An empty mask gives NaN,
    identical images +inf (as in the reference).
LPIPS (VGG) is the third number of metrics.py: with `lpips_weights` (lpips.load_weights of the two weight FILES the reference
downloads; nothing is fetched here) it is computed on the device from the same composited pair that SSIM takes
(csrc/lpips.hip).  Without weights the results are what they were.

python -m binocular3dgs_amd.evaluate -m MODEL_PATH [-s SOURCE] [--iteration N] [--mode png|report]
                                     [--lpips_vgg F --lpips_lin F | --lpips_npz F] [--align_poses N [--align_scales 4 2 1]]
evaluates the test cameras of the dataset folder and writes results.json / per_view.json under method ours_<iteration>.
--align_poses N: every held-out camera is first aligned to the model by N photometric steps on its pose against its own ground
truth (pose.refine_pose: a model trained on three views lives in a frame slightly off the held-out poses); the files gain
SSIM_aligned / PSNR_aligned / LPIPS_aligned beside the unaligned keys, per_view.json each view's twist.
"""
from __future__ import annotations

import json
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

MAX_BATCH = 8          # views per forward launch (B3GS_MAX_FUSED_VIEWS)
CLAMP, QUANTIZE = 1, 2  # B3GS_METRIC_CLAMP / B3GS_METRIC_QUANTIZE of include/b3gs_raster.h
MODES = {"report": CLAMP, "png": QUANTIZE}


# ---- batched renders ---------------------------------------------------------------------------------------------------
def _renderer(model, W: int, H: int, first_views: Sequence, bg: torch.Tensor, batch: int, capacity: Optional[int]):
    """The evaluation-owned FusedRasterizer of (model, W, H): cached on the model, rebuilt when P changed (densification)."""
    from .fused import FusedRasterizer
    cache = model.__dict__.setdefault("_b3gs_eval_renderers", {})
    fr = cache.get((W, H))
    if fr is None or fr.P != model.get_xyz.shape[0] or len(fr.slots) < batch or capacity is not None:
        fr = FusedRasterizer(model, W, H, num_slots=batch, binning_capacity=capacity, want_means2D=False,
                             schedule="batched", seg1_fraction=0.0)
        if capacity is None:
            fr.fit_capacity([(c, k) for k, c in enumerate(first_views[:batch])], bg)
        cache[(W, H)] = fr
    return fr


def _render_checked(fr, cams: Sequence, bg: torch.Tensor) -> List[dict]:
    """One launch for `cams`; one read of the overflow word; grow + render again when a tile list did not fit."""
    views = [(c, k) for k, c in enumerate(cams)]
    for _ in range(3):
        outs = fr.render_batch(views, bg)
        flag = int(fr.overflow_flag.item())
        if flag:
            fr.overflow_flag.zero_()
        if flag & 8:
            from ._lib import B3gsError
            raise B3gsError("a view was rendered from the depth order of the camera it names as `same_depth_as`, but their "
                            "depth keys differ")
        if not flag & 1:
            return outs
        fr.grow(need=int(fr.high_water.max().item()))
    raise RuntimeError("evaluation render: the binning capacity still overflowed after growing twice")


def _batches(model, cameras: Sequence, bg: torch.Tensor, batch: int, capacity: Optional[int] = None, full: bool = False):
    """Yields (indices into `cameras`, [3,H,W] images) per launch, views of one W x H together; with `full`, the per-view
    output dicts of the render ("render", "rendered_depth", "rendered_alpha", ...) instead of the images.  Both are the
    renderer's slot buffers: valid until the next item is drawn."""
    batch = max(1, min(int(batch), MAX_BATCH))
    groups: Dict[tuple, List[int]] = {}
    for i, cam in enumerate(cameras):
        groups.setdefault((int(cam.image_width), int(cam.image_height)), []).append(i)
    with torch.no_grad():
        for (W, H), idx in groups.items():
            cams = [cameras[i] for i in idx]
            fr = _renderer(model, W, H, cams, bg, batch, capacity)
            for c0 in range(0, len(cams), batch):
                outs = _render_checked(fr, cams[c0:c0 + batch], bg)
                yield idx[c0:c0 + batch], (outs if full else [o["render"] for o in outs])


def _walk_batches(model, cameras: Sequence, bg: torch.Tensor, batch: int, capacity: Optional[int] = None):
    """_batches(full=True) for the calls that walk the forward's tile lists a second time (importance, pixel_maps, segment):
    yields (indices into `cameras`, per-view output dicts, W, H, slots) per launch -- slots[k] holds the state buffers
    (geom, binning, img) the forward of camera idx[k] left (_render_checked renders camera k of a launch into slot k)."""
    for idx, outs in _batches(model, cameras, bg, batch, capacity, full=True):
        cam0 = cameras[idx[0]]
        W, H = int(cam0.image_width), int(cam0.image_height)
        yield idx, outs, W, H, model.__dict__["_b3gs_eval_renderers"][(W, H)].slots[:len(idx)]


def render_views(model, cameras: Sequence, bg: torch.Tensor, *, batch: int = MAX_BATCH,
                 capacity: Optional[int] = None) -> List[torch.Tensor]:
    """render(cam, model, pipe, bg)["render"] under no_grad for every camera, up to `batch` (<= 8) views of the same
    W x H per launch.  `capacity`: the starting binning capacity of a fresh renderer (default: fit_capacity() on the
    first batch)."""
    out: List[Optional[torch.Tensor]] = [None] * len(cameras)
    for idx, imgs in _batches(model, cameras, bg, batch, capacity):
        for i, img in zip(idx, imgs):
            out[i] = img.clone()
    return out


# ---- metrics -----------------------------------------------------------------------------------------------------------
def image_metrics(images: Sequence[torch.Tensor], gts: Sequence[torch.Tensor], masks=None, mode: int = CLAMP,
                  prepared: bool = False):
    """Device sums of b3gs_image_metrics_batch for [C,H,W] pairs of one shape: float64 [n, 2C + 2] (sum |d| per channel,
    sum d^2 per channel, sum d^2 where mask == 1, that count) and, with `prepared`, the composited pair ([n,C,H,W] each)."""
    from . import _C
    n = len(images)
    C, H, W = images[0].shape
    dev = images[0].device
    out = torch.empty((n, 2 * C + 2), dtype=torch.float64, device=dev)
    pi = pg = None
    if prepared:
        pi = torch.empty((n, C, H, W), dtype=torch.float32, device=dev)
        pg = torch.empty_like(pi)
    _C.image_metrics(list(images), list(gts), None if masks is None else list(masks), int(mode), out, pi, pg)
    return out, pi, pg


def _psnr(mse):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 20.0 * np.log10(1.0 / np.sqrt(mse))


def _fit_views(imgs, gts, mk):
    """Every render through the best affine colour map onto its ground truth (exposure.fit_exposure over the pixels of the
    view's mask; a degenerate view keeps the identity) -> (the fitted renders, the matrices).  No host read."""
    from .exposure import apply_exposure_batch, fit_exposure
    planes = None if mk is None else [None if m is None else (m[0] != 0).to(torch.uint8) for m in mk]
    fits = fit_exposure([x.contiguous() for x in imgs], [g.to(imgs[0].device, torch.float32).contiguous() for g in gts], planes)
    with torch.no_grad():
        out = apply_exposure_batch([x.contiguous() for x in imgs], [A for A, _ in fits])
    return out, [A for A, _ in fits]


def _device_sums(model, cameras, bg, masks, mode_bits: int, want_ssim: bool, batch: int, capacity=None, lpips_weights=None,
                 fitted=None):
    """-> (sums [N, 2C+2] float64, ssim [N] or None, H*W per view, lpips [N] or None), one read-back at the end.
    `fitted`: a list that receives (view index, its fitted 3x4 on the device); the renders are then scored after _fit_views."""
    from . import _C
    parts = []
    lp = []
    for idx, imgs in _batches(model, cameras, bg, batch, capacity):
        gts = [cameras[i].original_image for i in idx]
        mk = None if masks is None else [masks[i] for i in idx]
        if fitted is not None:
            imgs, mats = _fit_views(imgs, gts, mk)
            fitted.extend(zip(idx, mats))
        sums, pi, pg = image_metrics(imgs, gts, mk, mode_bits, prepared=want_ssim)
        ss = _C.ssim(pi, pg, 11, False) if want_ssim else None
        if lpips_weights is not None:        # metrics.py:105 on the pair of metrics.py:95-96
            from .lpips import lpips
            lp.append(lpips(pi, pg, lpips_weights))
        parts.append((idx, sums, ss))
    order = [i for idx, _, _ in parts for i in idx]
    sums = torch.cat([s for _, s, _ in parts]).cpu().numpy()
    ssim = torch.cat([s for _, _, s in parts]).double().cpu().numpy() if want_ssim else None
    inv = np.empty(len(order), dtype=np.int64)
    inv[np.asarray(order, dtype=np.int64)] = np.arange(len(order))
    hw = np.array([float(cameras[i].image_width * cameras[i].image_height) for i in range(len(cameras))])
    return sums[inv], (None if ssim is None else ssim[inv]), hw, (torch.cat(lp).cpu().numpy()[inv] if lp else None)


def evaluate_views(model, cameras: Sequence, bg: torch.Tensor, *, masks=None, mode: str = "report",
                   batch: int = MAX_BATCH, lpips_weights=None, fit_exposure: bool = False) -> dict:
    """SSIM / PSNR / L1 of every camera's render against its `original_image`.

    mode "report": both images clamped to [0,1]; PSNR = mean of the per-channel PSNRs (train.py:226-261).
    mode "png":    both images through the 8-bit PNG round trip, composited with `masks` (per camera None, [1,H,W] or
                   [3,H,W]; None = LLFF's all-ones mask), PSNR over the elements whose mask is exactly 1 (metrics.py).
    SSIM is ssim() of the composited pair, L1 the mean |difference| of the same pair.
    `lpips_weights` (lpips.LpipsWeights): every per-view dict also gets "LPIPS" = lpips(net_type='vgg') of that same pair
    (metrics.py:105) and the result its fp32 mean; SSIM, PSNR and L1 keep their bits.
    `fit_exposure`: every render is first mapped onto its ground truth by the best 3x4 affine colour map (the colour-corrected
    metrics of RawNeRF / Zip-NeRF: exposure.fit_exposure, over the view's mask where it has one); every per-view dict gains
    "exposure", the fitted matrix.
    -> {"per_view": [{"SSIM", "PSNR", "L1"}, ...], "SSIM", "PSNR", "L1": fp32 means of the per-view values}."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    if not cameras:
        return {"per_view": [], "SSIM": math.nan, "PSNR": math.nan, "L1": math.nan}
    fitted = [] if fit_exposure else None
    sums, ssim, hw, lp = _device_sums(model, cameras, bg, masks, MODES[mode], True, batch, lpips_weights=lpips_weights, fitted=fitted)
    C = (sums.shape[1] - 2) // 2
    l1 = sums[:, :C].sum(1) / (C * hw)
    if mode == "report":
        psnr = _psnr(sums[:, C:2 * C] / hw[:, None]).mean(1)
    else:
        psnr = _psnr(sums[:, 2 * C] / sums[:, 2 * C + 1])
    per_view = [{"SSIM": float(s), "PSNR": float(p), "L1": float(a)} for s, p, a in zip(ssim, psnr, l1)]
    if lp is not None:
        for v, x in zip(per_view, lp):
            v["LPIPS"] = float(x)
    if fitted:
        mats = torch.stack([A for _, A in fitted]).cpu().tolist()
        for (i, _), A in zip(fitted, mats):
            per_view[i]["exposure"] = A
    res = {"per_view": per_view}
    for key in ("SSIM", "PSNR", "L1") + (("LPIPS",) if lp is not None else ()):     # metrics.py:108-110: torch.tensor(values).mean() -- fp32
        res[key] = float(torch.tensor([v[key] for v in per_view]).mean())
    return res


# ---- training_report (train.py:226-261) --------------------------------------------------------------------------------
def report_configs(test_cameras, train_cameras):
    """train.py:235-236: the test cameras, and train cameras 5, 10, .., 25 modulo their count (3 views: 2,1,0,2,1)."""
    train = list(train_cameras or [])
    return [("test", list(test_cameras or [])),
            ("train", [train[i % len(train)] for i in range(5, 30, 5)] if train else [])]


def training_report(model, test_cameras, train_cameras, bg: torch.Tensor, *, batch: int = MAX_BATCH,
                    render_fn: Optional[Callable] = None, view_metrics: Optional[Callable] = None) -> dict:
    """train.py:238-252 -> {"test": (l1, psnr), "train": (l1, psnr)}; a config without cameras is left out.
    Per view: clamp(render, 0, 1) against clamp(original_image, 0, 1), L1 and the mean of the per-channel PSNRs, summed in
    float64 in view order and divided by the camera count.

    Default: render_views + b3gs_image_metrics_batch (fp64 sums).  `render_fn(cameras) -> [3,H,W] images` and
    `view_metrics(image, gt) -> (l1, psnr)` replace the two halves (the reference's statements, on the CPU)."""
    res = {}
    for name, cams in report_configs(test_cameras, train_cameras):
        if not cams:
            continue
        if view_metrics is None:
            sums, _, hw, _ = _device_sums(model, cams, bg, None, CLAMP, False, batch)
            C = (sums.shape[1] - 2) // 2
            vals = zip(sums[:, :C].sum(1) / (C * hw), _psnr(sums[:, C:2 * C] / hw[:, None]).mean(1))
        else:
            images = render_fn(cams) if render_fn is not None else render_views(model, cams, bg, batch=batch)
            vals = [view_metrics(torch.clamp(img, 0.0, 1.0), torch.clamp(cam.original_image, 0.0, 1.0))
                    for img, cam in zip(images, cams)]
        l1_sum, psnr_sum = 0.0, 0.0
        for l1, psnr in vals:
            l1_sum += float(l1)
            psnr_sum += float(psnr)
        res[name] = (l1_sum / len(cams), psnr_sum / len(cams))
    return res


def depth_pearson(model, cameras: Sequence, bg: torch.Tensor, priors_dir: str, mode: str = "depth") -> List[float]:
    """rho_image of depth_prior.depth_prior_loss between every camera's rendered depth and <priors_dir>/<image_name>.npy
    (resized to the camera's size; every valid pixel is used).  One host read per view, behind the loop."""
    from .depth_prior import depth_prior_loss, load_priors
    from .render import PipelineParams, render
    priors = load_priors(priors_dir, cameras, device=bg.device)
    rhos = []
    with torch.no_grad():
        for k, (cam, (prior, mask)) in enumerate(zip(cameras, priors)):
            pkg = render(cam, model, PipelineParams(), bg)
            _, parts = depth_prior_loss(pkg["rendered_depth"], pkg["rendered_alpha"], prior, mask, mode=mode, return_parts=True)
            rhos.append(parts[5])
    return [float(x) for x in torch.stack(rhos).cpu()] if rhos else []


def normal_cos(model, cameras: Sequence, bg: torch.Tensor, priors_dir: str, frame: str = "opencv", alpha_min: float = 0.5) -> List[float]:
    """Per camera the mean n.t over the valid pixels between the normals of its rendered depth map and
    <priors_dir>/<image_name>.npy | .png (normal_prior.load_normal_priors: resized to the camera's size, `frame` converted to
    the camera frame); a view without a valid pixel scores 0.  One host read, behind the loop."""
    from .normal_prior import load_normal_priors, normal_prior_loss
    from .render import PipelineParams, render
    priors = load_normal_priors(priors_dir, cameras, frame=frame, device=bg.device)
    dots = []
    with torch.no_grad():
        for k, (cam, (target, mask)) in enumerate(zip(cameras, priors)):
            pkg = render(cam, model, PipelineParams(), bg)
            _, parts = normal_prior_loss(pkg["rendered_depth"], pkg["rendered_alpha"], target, mask, cam, alpha_min=alpha_min,
                                         return_parts=True)
            dots.append(parts[4])
    return [float(x) for x in torch.stack(dots).cpu()] if dots else []


# ---- results.json / per_view.json (metrics.py:105-122) ----------------------------------------------------------------
def write_results(model_path: str, method: str, per_view: Sequence[dict], names: Sequence[str], aligned: Optional[Sequence[dict]] = None,
                  twists=None, exposure: Optional[Sequence[dict]] = None) -> dict:
    """Writes <model_path>/results.json {method: {"SSIM", "PSNR"}} and per_view.json {method: {"SSIM": {name: v}, "PSNR":
    {name: v}}} in the reference's layout (json.dump, indent=True); the "LPIPS" key is written in both files, as
    metrics.py:112-117 does, when EVERY per-view entry carries it, and left out otherwise; so are "DepthPearson" (depth_pearson) and "NormalCos" (normal_cos).  Means are fp32, as
    torch.tensor(values).mean() is there.  `aligned` (the per-view metrics after pose alignment) adds the same keys with the
    suffix _aligned behind them, `twists` ([n,6]) adds per_view.json's "twist": {name: [omega, t]}; without them the files are
    what they were.  `exposure` (the per-view metrics after evaluate_views(fit_exposure=True)) adds the keys with the suffix
    _exposure in the same way and per_view.json's "exposure": {name: 3x4}.  Returns the two dicts."""
    if len(per_view) != len(names) or any(x is not None and len(x) != len(names) for x in (aligned, exposure)):
        raise ValueError("one name per view")
    keys = ("SSIM", "PSNR") + tuple(k for k in ("LPIPS", "DepthPearson", "NormalCos") if per_view and all(k in v for v in per_view))
    vals = {k: torch.tensor([float(v[k]) for v in per_view]) for k in keys}
    if aligned is not None:
        vals.update({k + "_aligned": torch.tensor([float(v[k]) for v in aligned]) for k in keys if all(k in v for v in aligned)})
    if exposure is not None:
        vals.update({k + "_exposure": torch.tensor([float(v[k]) for v in exposure]) for k in keys if all(k in v for v in exposure)})
    full = {method: {k: vals[k].mean().item() for k in vals}}
    per = {method: {k: {name: x for x, name in zip(vals[k].tolist(), names)} for k in vals}}
    if exposure is not None:
        per[method]["exposure"] = {name: v["exposure"] for v, name in zip(exposure, names)}
    if twists is not None:
        per[method]["twist"] = {name: [float(x) for x in t] for t, name in zip(twists, names)}
    os.makedirs(model_path, exist_ok=True)
    with open(os.path.join(model_path, "results.json"), "w") as fp:
        json.dump(full, fp, indent=True)
    with open(os.path.join(model_path, "per_view.json"), "w") as fp:
        json.dump(per, fp, indent=True)
    return {"results": full, "per_view": per}


# ---- command line: metrics.py over the test cameras of a trained model ------------------------------------------------
def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, mode: str = "png", lpips_weights=None,
        masks=None, align_poses: int = 0, align_scales: Sequence[int] = (4, 2, 1), depth_priors: Optional[str] = None,
        depth_prior_mode: Optional[str] = None, fit_exposure: bool = False, normal_priors: Optional[str] = None,
        normal_prior_frame: Optional[str] = None) -> dict:
    """Loads <model_path>/point_cloud/iteration_<it> and the dataset's test cameras (cfg_args gives the defaults, as in
    spiral.py), evaluates them, prints the means in metrics.py:107-109's format and writes results.json / per_view.json under
    method ours_<it>.  `masks`: DTU IDR object masks per test camera (the command line does not read them).
    align_poses = N > 0: the cameras are refined for N iterations each (pose.refine_poses, coarse to fine over align_scales)
    and evaluated again; the result gains "aligned" (evaluate_views of the refined cameras) and "twists".
    depth_priors = DIR: "DepthPearson", the mean rho_image against <DIR>/<image_name>.npy of the test views (depth_pearson;
    depth_prior_mode defaults to the run's own in cfg_args), in results.json and per view in per_view.json.
    normal_priors = DIR: "NormalCos", the mean over the test views of the per-view mean n.t over the valid pixels (normal_cos;
    normal_prior_frame and alpha_min default to the run's own in cfg_args), in results.json and per view in per_view.json.
    fit_exposure: the views are scored a second time after the best affine colour map onto their ground truth (a held-out
    view has no learned exposure); the result gains "exposure" and the files SSIM_exposure / PSNR_exposure / LPIPS_exposure
    and each view's matrix."""
    from .gaussian_model import GaussianModel
    from .scene import Scene
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    source_path = source_path or cfg.get("source_path")
    if not source_path:
        raise ValueError("no source path: pass -s or keep cfg_args next to the model")
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it), "point_cloud.ply"))
    white = bool(cfg.get("white_background", False))
    scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                               dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                               resolution=cfg.get("resolution", -1), white_background=white,
                               init_points=cfg.get("init_points", "matcher"), shuffle=False)
    cams = scene.getTestCameras()
    if not cams:
        raise ValueError(f"{source_path}: no test cameras")
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    res = evaluate_views(model, cams, bg, masks=masks, mode=mode, lpips_weights=lpips_weights)
    print("  SSIM : {:>12.7f}".format(res["SSIM"]))
    print("  PSNR : {:>12.7f}".format(res["PSNR"]))
    if "LPIPS" in res:
        print("  LPIPS: {:>12.7f}".format(res["LPIPS"]))
    if depth_priors:
        rhos = depth_pearson(model, cams, bg, depth_priors, depth_prior_mode or cfg.get("depth_prior_mode", "depth") or "depth")
        for v, r in zip(res["per_view"], rhos):
            v["DepthPearson"] = r
        res["DepthPearson"] = float(torch.tensor(rhos).mean())
        print("  DepthPearson: {:>12.7f}".format(res["DepthPearson"]))
    if normal_priors:
        dots = normal_cos(model, cams, bg, normal_priors, normal_prior_frame or cfg.get("normal_prior_frame", "opencv") or "opencv",
                          float(cfg.get("normal_prior_alpha_min", 0.5) or 0.5))
        for v, r in zip(res["per_view"], dots):
            v["NormalCos"] = r
        res["NormalCos"] = float(torch.tensor(dots).mean())
        print("  NormalCos: {:>12.7f}".format(res["NormalCos"]))
    print("")
    names = ["{0:05d}.png".format(i) for i in range(len(cams))]      # render.py:34: the file names metrics.py lists
    fit = None
    if fit_exposure:
        res["exposure"] = evaluate_views(model, cams, bg, masks=masks, mode=mode, lpips_weights=lpips_weights, fit_exposure=True)
        fit = res["exposure"]["per_view"]
        print("  SSIM (exposure): {:>12.7f}".format(res["exposure"]["SSIM"]))
        print("  PSNR (exposure): {:>12.7f}".format(res["exposure"]["PSNR"]))
        if "LPIPS" in res["exposure"]:
            print("  LPIPS (exposure): {:>12.7f}".format(res["exposure"]["LPIPS"]))
        print("")
    if align_poses > 0:
        from .pose import refine_poses
        refined, twists, _ = refine_poses(model, cams, masks=masks, iters=int(align_poses), scales=tuple(align_scales), bg=bg)
        res["aligned"] = evaluate_views(model, refined, bg, masks=masks, mode=mode, lpips_weights=lpips_weights)
        res["twists"] = twists
        print("  SSIM (aligned): {:>12.7f}".format(res["aligned"]["SSIM"]))
        print("  PSNR (aligned): {:>12.7f}".format(res["aligned"]["PSNR"]))
        if "LPIPS" in res["aligned"]:
            print("  LPIPS (aligned): {:>12.7f}".format(res["aligned"]["LPIPS"]))
        print("")
        write_results(model_path, "ours_{}".format(it), res["per_view"], names, res["aligned"]["per_view"], twists, exposure=fit)
        return res
    write_results(model_path, "ours_{}".format(it), res["per_view"], names, exposure=fit)
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.evaluate", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--mode", choices=sorted(MODES), default="png")
    p.add_argument("--lpips_vgg", default=None, help="torchvision's vgg16-397923af.pth (a file; nothing is fetched)")
    p.add_argument("--lpips_lin", default=None, help="the LPIPS package's weights/v0.1/vgg.pth")
    p.add_argument("--lpips_npz", default=None, help="the two files converted once by lpips.save_weights")
    p.add_argument("--align_poses", type=int, default=0, metavar="N",
                   help="align every held-out camera to the model by N photometric pose steps before scoring it again")
    p.add_argument("--align_scales", type=int, nargs="+", default=[4, 2, 1], help="the coarse-to-fine pyramid of the alignment")
    p.add_argument("--depth_priors", default=None, metavar="DIR",
                   help="<image_name>.npy priors of the test views: adds DepthPearson (mean rho_image) to results.json / per_view.json")
    p.add_argument("--depth_prior_mode", choices=("depth", "disparity"), default=None, help="default: the training run's")
    p.add_argument("--normal_priors", default=None, metavar="DIR",
                   help="<image_name>.npy | .png normal priors of the test views: adds NormalCos (mean n.t) to results.json / per_view.json")
    p.add_argument("--normal_prior_frame", choices=("opencv", "opengl", "world"), default=None, help="default: the training run's")
    p.add_argument("--fit_exposure", action="store_true",
                   help="score every view again after the best 3x4 affine colour map onto its ground truth: SSIM_exposure / "
                        "PSNR_exposure / LPIPS_exposure in results.json, each view's matrix in per_view.json")
    a = p.parse_args(argv)
    w = None
    if a.lpips_npz:
        if a.lpips_vgg or a.lpips_lin:
            p.error("--lpips_npz replaces --lpips_vgg / --lpips_lin")
        from .lpips import load_weights
        w = load_weights(a.lpips_npz)
    elif a.lpips_vgg or a.lpips_lin:
        if not (a.lpips_vgg and a.lpips_lin):
            p.error("--lpips_vgg and --lpips_lin go together")
        from .lpips import load_weights
        w = load_weights(a.lpips_vgg, a.lpips_lin)
    run(a.model_path, a.source_path, a.iteration, a.mode, w, align_poses=a.align_poses, align_scales=a.align_scales,
        depth_priors=a.depth_priors, depth_prior_mode=a.depth_prior_mode, fit_exposure=a.fit_exposure,
        normal_priors=a.normal_priors, normal_prior_frame=a.normal_prior_frame)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
