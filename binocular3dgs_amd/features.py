"""Feature fields: a C-channel float field per Gaussian, rendered into [C,H,W] maps and lifted back from such maps.

render_features() renders the cameras as evaluate.py, importance.py and segment.py do (up to 8 views of one W x H per
b3gs_forward_raw_batch launch on the evaluation-owned FusedRasterizer, no gradients to the geometry) and, after every launch,
walks the tile lists that forward left on the device a second time (b3gs_feature_render_batch, csrc/features.hip): every
blended (pixel, Gaussian) has the weight w = alpha * T, and

    out[c, pixel] = sum of w f[g, c] over the pixel's blended Gaussians          (float32, in list order, no background term)

-- what the forward does with its three colours, for any C <= 256 and without projecting, binning and sorting once per three
channels.  lift_features() is the adjoint (b3gs_feature_lift_batch):

    sums[g, c] = sum of w F[c, pixel] over the pixels of all cameras Gaussian g was blended into,    weight[g] = sum of w

so that <render(f), F> = <f, lift(F)>.  The device sums integers (rint(w F / scale[c] 2^32), 64-bit adds): the same bits
whatever the batch size or the camera order.  `scale` must bound |F| per channel (default: the largest |F| over all maps); a
larger |F| is clamped.  mean_features(sums, weight) is the learning-free uplift of 2D feature maps (DINO / CLIP / SAM
embeddings): every Gaussian takes the blend-weighted mean of the features of the pixels it paints.

FeatureRender / feature_field() tie the pair into torch.autograd: forward = render, backward = lift of the incoming gradient,
gradients to the features only (the geometry is frozen), so per-Gaussian features can be fitted to 2D targets with any torch
loss and optimizer.  The backward renders its cameras again (a later forward may have reused the state buffers).

gaussian_normals() / render_normals(): the shortest axis of every Gaussian, flipped towards the camera per view, blended and
normalised -- world-space normal maps.  similar() / feature_under(): click-to-select by cosine similarity.

python -m binocular3dgs_amd.features -m MODEL_PATH [-s SOURCE] [--iteration N] [--pruned] COMMAND ...
    lift    --maps DIR [--views train|test|all] [--out F.npy]     DIR/<image_name>.npy float32 [C,h,w] per camera (a camera
                                                                  without a file is skipped), nearest-neighbour to the view's
                                                                  size; writes the mean features, float32 [P, C]
    render  --features F.npy --views test|all --out DIR [--channels a b c]
                                                                  feature_%05d.npy [C,H,W] and feature_%05d.png: three
                                                                  channels, min-max scaled over the view
    normals --views test|all --out DIR [--source depth]           normal_%05d.png of (n + 1) / 2 (--source depth: depth_normal_%05d.png,
                                                                  the normals of the rendered depth map, normal_prior.depth_normals)
    select  --features F.npy --view NAME --pixel X Y --threshold T --model_out NEW
                                                                  the Gaussians whose feature is similar to the one rendered
                                                                  at the pixel, as NEW/point_cloud/iteration_<n>/point_cloud.ply
"""
from __future__ import annotations

import json
import os
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_CHANNELS = 256       # B3GS_MAX_FEATURE_CHANNELS
Q32 = 4294967296.0


def _check_features(model, features: torch.Tensor) -> torch.Tensor:
    P = model.get_xyz.shape[0]
    f = torch.as_tensor(features)
    if f.dim() != 2 or f.shape[0] != P or not 1 <= f.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"features is [P, C] = [{P}, 1 .. {MAX_CHANNELS}], not {tuple(f.shape)}")
    return f.detach().to(device=model.get_xyz.device, dtype=torch.float32).contiguous()


def _black(model) -> torch.Tensor:
    return torch.zeros(3, dtype=torch.float32, device=model.get_xyz.device)


def _render_batches(model, cameras: Sequence, bg: torch.Tensor, f: torch.Tensor, batch: int, capacity: Optional[int]):
    """Per launch: (camera indices, forward output dicts, the [C,H,W] planes of every view)."""
    from . import _C
    from .evaluate import _walk_batches
    dev = f.device
    P, C = f.shape
    for idx, outs, W, H, slots in _walk_batches(model, cameras, bg, batch, capacity):
        # (the launch writes every pixel; without Gaussians there is no launch)
        planes = [torch.empty((C, H, W), dtype=torch.float32, device=dev) if P else torch.zeros((C, H, W), device=dev) for _ in slots]
        if P:
            _C.feature_render([(s.geom, s.binning, s.img, W, H, o) for s, o in zip(slots, planes)], f)
        yield idx, outs, planes


def render_features(model, cameras: Sequence, features: torch.Tensor, *, batch: int = 8,
                    capacity: Optional[int] = None) -> Iterator[Tuple[int, torch.Tensor]]:
    """Yields (camera index, float32 [C,H,W]) for every camera, launch by launch (cameras of one size together, otherwise in
    order): per pixel and channel the blend-weighted sum of the Gaussians' features.  The tensors are the caller's to keep."""
    f = _check_features(model, features)
    for idx, _outs, planes in _render_batches(model, cameras, _black(model), f, batch, capacity):
        for i, p in zip(idx, planes):
            yield i, p


def _as_maps(maps: Sequence, cameras: Sequence, dev) -> Tuple[list, int]:
    if len(maps) != len(cameras):
        raise ValueError("one [C,H,W] map (or None) per camera")
    out, C = [], None
    for m, cam in zip(maps, cameras):
        if m is None:
            out.append(None)
            continue
        m = torch.as_tensor(m)
        H, W = int(cam.image_height), int(cam.image_width)
        if m.dim() != 3 or tuple(m.shape[1:]) != (H, W) or (C is not None and m.shape[0] != C):
            raise ValueError(f"a map is [C,H,W] = [C,{H},{W}] with one C for all cameras, not {tuple(m.shape)}")
        C = int(m.shape[0])
        out.append(m.detach().to(device=dev, dtype=torch.float32).contiguous())
    if C is None:
        raise ValueError("no camera has a map")
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"1 .. {MAX_CHANNELS} channels, not {C}")
    return out, C


def default_scale(maps: Sequence) -> torch.Tensor:
    """float32 [C] on the maps' device: the largest |F| of every channel over all maps, 1 where that is 0."""
    amax = None
    for m in maps:
        if m is not None:
            a = m.abs().amax(dim=(1, 2))
            amax = a if amax is None else torch.maximum(amax, a)
    return torch.where(amax > 0, amax, torch.ones_like(amax))


def lift_features_q32(model, cameras: Sequence, bg: torch.Tensor, maps: Sequence, *, masks=None, scale=None, batch: int = 8,
                      capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The device integers of lift_features(): (sums_q32 int64 [P,C], weight_q32 int64 [P], scale float32 [C]);
    sums = scale * sums_q32 / 2^32, weight = weight_q32 / 2^32."""
    from . import _C
    from .evaluate import _walk_batches
    dev = model.get_xyz.device
    P = model.get_xyz.shape[0]
    maps, C = _as_maps(maps, cameras, dev)
    if masks is not None and len(masks) != len(cameras):
        raise ValueError("one mask (or None) per camera")
    used = [i for i, m in enumerate(maps) if m is not None]
    finite = torch.stack([torch.isfinite(maps[i]).all() for i in used]).all()
    if scale is None:
        scale = default_scale(maps)
    scale = torch.as_tensor(scale, dtype=torch.float32).reshape(-1)
    if scale.shape[0] != C:
        raise ValueError("one scale per channel")
    host_scale = scale.cpu()                       # (the one wait of the call: the library takes the table from host memory)
    if not bool(finite):
        raise ValueError("the maps hold values that are not finite")
    if not bool((torch.isfinite(host_scale) & (host_scale > 0)).all()):
        raise ValueError("every scale is a finite number > 0")
    sums = torch.zeros((P, C), dtype=torch.int64, device=dev)
    wq = torch.zeros(P, dtype=torch.int64, device=dev)
    if P:
        cams = [cameras[i] for i in used]
        for idx, _outs, W, H, slots in _walk_batches(model, cams, bg, batch, capacity):
            views = []
            for i, s in zip(idx, slots):
                m = None if masks is None or masks[used[i]] is None else \
                    (torch.as_tensor(masks[used[i]]).reshape(H, W) != 0).to(device=dev, dtype=torch.uint8)
                views.append((s.geom, s.binning, s.img, W, H, maps[used[i]], m))
            _C.feature_lift(views, host_scale, sums, wq)
    return sums, wq, scale.to(dev)


def lift_features(model, cameras: Sequence, bg: torch.Tensor, maps: Sequence, *, masks=None, scale=None, batch: int = 8,
                  capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(sums float32 [P,C], weight float32 [P]): sums[g,c] = sum of w maps[c,pixel], weight[g] = sum of w over the pixels of all
    cameras that blended Gaussian g.  maps: per camera None (skipped) or [C,H,W]; masks: None, or per camera None or an [H,W]
    tensor (nonzero = count the pixel); scale: [C], every |F| above it is clamped (default: default_scale(maps))."""
    sums, wq, scale = lift_features_q32(model, cameras, bg, maps, masks=masks, scale=scale, batch=batch, capacity=capacity)
    s = (sums.to(torch.float64) * (scale.to(torch.float64) / Q32)).to(torch.float32)
    # (the weight words are unsigned: below 2^63 for any camera set that fits a lifetime)
    return s, (wq.to(torch.float64) / Q32).to(torch.float32)


def mean_features(sums: torch.Tensor, weight: torch.Tensor, min_weight: float = 0.0) -> torch.Tensor:
    """[P,C]: sums / weight where weight > min_weight, 0 elsewhere.  Pure torch."""
    ok = weight > min_weight
    w = torch.where(ok, weight, torch.ones_like(weight)).unsqueeze(1)
    return torch.where(ok.unsqueeze(1), sums / w, torch.zeros_like(sums))


class FeatureRender(torch.autograd.Function):
    """features [P,C] -> the stacked [n,C,H,W] renders of n cameras of one size.  backward: the lift of the incoming gradient
    (scale = its largest magnitude per channel, so nothing is clamped and the quantisation step is 2^-32 of that).  The
    geometry is frozen: no gradient reaches the model."""

    @staticmethod
    def forward(ctx, features, model, cameras, batch):
        cameras = list(cameras)
        if len({(int(c.image_width), int(c.image_height)) for c in cameras}) != 1:
            raise ValueError("the cameras of one feature_field() call share their size")
        ctx.model, ctx.cameras, ctx.batch = model, cameras, batch
        out = [None] * len(cameras)
        for i, p in render_features(model, cameras, features, batch=batch):
            out[i] = p
        return torch.stack(out)

    @staticmethod
    def backward(ctx, grad):
        cams = ctx.cameras
        g = grad.detach().to(torch.float32)
        sums, _w = lift_features(ctx.model, cams, _black(ctx.model), [g[i] for i in range(len(cams))], batch=ctx.batch)
        return sums.to(grad.dtype), None, None, None


def feature_field(model, camera_batch: Sequence, *, batch: int = 8):
    """-> a function features [P,C] -> [n,C,H,W] that torch.autograd differentiates with respect to the features."""
    cams = list(camera_batch)
    return lambda features: FeatureRender.apply(features, model, cams, batch)


# ---- normals ---------------------------------------------------------------------------------------------------------------
def gaussian_normals(model) -> torch.Tensor:
    """float32 [P,3]: the unit axis of every Gaussian's rotation that belongs to its smallest scale (sign as the rotation has it)."""
    from .gaussian_model import build_rotation
    with torch.no_grad():
        R = build_rotation(model._rotation.detach())                 # columns = axes
        k = model.get_scaling.detach().argmin(dim=1)
        return R.gather(2, k.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(2).contiguous()


def render_normals(model, cameras: Sequence, *, capacity: Optional[int] = None) -> Iterator[Tuple[int, torch.Tensor, torch.Tensor]]:
    """Yields (camera index, normals float32 [3,H,W], valid bool [H,W]): every Gaussian's shortest axis, flipped towards the
    camera, blended; divided by its norm where the pixel's weight sum is > 0 (and the blended vector is not 0): world-space
    unit normals, 0 where not valid.  One launch per camera: the flip belongs to the view."""
    n = gaussian_normals(model)
    xyz = model.get_xyz.detach()
    bg = _black(model)
    for i, cam in enumerate(cameras):
        to_cam = cam.camera_center.to(xyz.device).unsqueeze(0) - xyz
        f = torch.where(((n * to_cam).sum(1, keepdim=True) < 0), -n, n).contiguous()
        for _idx, outs, planes in _render_batches(model, [cam], bg, f, 1, capacity):
            v = planes[0]
            norm = torch.sqrt((v * v).sum(0))
            valid = (outs[0]["rendered_alpha"].reshape(norm.shape) > 0) & (norm > 0)
            yield i, torch.where(valid.unsqueeze(0), v / torch.where(valid, norm, torch.ones_like(norm)).unsqueeze(0), torch.zeros_like(v)), valid


# ---- selection by similarity -------------------------------------------------------------------------------------------------
def similar(features: torch.Tensor, query: torch.Tensor, threshold: float) -> torch.Tensor:
    """bool [P]: cosine similarity of every row of features [P,C] with query [C] is >= threshold (a zero row is similar to
    nothing).  Pure torch."""
    f = torch.as_tensor(features, dtype=torch.float32)
    q = torch.as_tensor(query, dtype=torch.float32, device=f.device).reshape(-1)
    fn, qn = torch.sqrt((f * f).sum(1)), torch.sqrt((q * q).sum())
    ok = (fn > 0) & (qn > 0)
    cos = (f @ q) / torch.where(ok, fn * qn, torch.ones_like(fn))
    return ok & (cos >= threshold)


def feature_under(model, camera, features: torch.Tensor, x: int, y: int) -> torch.Tensor:
    """float32 [C]: the feature rendered at pixel (x, y) of `camera`, divided by its norm (0 where nothing was blended)."""
    if not (0 <= int(x) < int(camera.image_width) and 0 <= int(y) < int(camera.image_height)):
        raise ValueError("the pixel lies outside the view")
    (_i, planes), = list(render_features(model, [camera], features, batch=1))
    v = planes[:, int(y), int(x)]
    nrm = torch.sqrt((v * v).sum())
    return v / nrm if float(nrm) > 0 else torch.zeros_like(v)


# ---- command line ------------------------------------------------------------------------------------------------------------
def _load(model_path: str, source_path: Optional[str], iteration: int, pruned: bool):
    from .gaussian_model import GaussianModel
    from .scene import Scene
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    source_path = source_path or cfg.get("source_path")
    if not source_path:
        raise ValueError("no source path: pass -s or keep cfg_args next to the model")
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it) + ("_pruned" if pruned else ""), "point_cloud.ply"))
    white = bool(cfg.get("white_background", False))
    scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                               dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                               resolution=cfg.get("resolution", -1), white_background=white,
                               init_points=cfg.get("init_points", "matcher"), shuffle=False)
    train, test = list(scene.getTrainCameras()), list(scene.getTestCameras())
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    return model, {"train": train, "test": test, "all": train + test}, bg, it


def _read_map(directory: str, cam) -> Optional[torch.Tensor]:
    """DIR/<image_name>.npy (the name as it is, or without its extension): float32 [C,h,w], nearest-neighbour to the view's size."""
    name = str(cam.image_name)
    for stem in (name, os.path.splitext(name)[0]):
        path = os.path.join(directory, stem + ".npy")
        if os.path.exists(path):
            a = np.load(path)
            if a.ndim != 3 or a.dtype.kind != "f":
                raise ValueError(f"{path}: a feature map is a float [C,h,w] array")
            m = torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))
            H, W = int(cam.image_height), int(cam.image_width)
            if tuple(m.shape[1:]) != (H, W):
                ys = (torch.arange(H) * m.shape[1]) // H
                xs = (torch.arange(W) * m.shape[2]) // W
                m = m[:, ys][:, :, xs]
            return m.contiguous()
    return None


def _picture(planes: torch.Tensor) -> torch.Tensor:
    """[3,H,W] float -> uint8 [H,W,3] (CPU), min-max scaled over the whole picture."""
    lo, hi = planes.min(), planes.max()
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return ((planes - lo) / span * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu()


def run_lift(model, cams, bg, maps_dir: str, out: str) -> dict:
    maps = [_read_map(maps_dir, c) for c in cams]
    if all(m is None for m in maps):
        raise ValueError(f"no camera has a feature map in {maps_dir}")
    sums, weight = lift_features(model, cams, bg, maps)
    np.save(out, mean_features(sums, weight).cpu().numpy())
    return {"features": out, "P": int(sums.shape[0]), "C": int(sums.shape[1]), "views": sum(m is not None for m in maps),
            "seen": int((weight > 0).sum())}


def run_render(model, cams, features_path: str, out: str, channels=None) -> dict:
    from . import frames
    f = torch.from_numpy(np.load(features_path))
    C = int(f.shape[1])
    ch = list(channels) if channels else [min(k, C - 1) for k in range(3)]
    if len(ch) != 3 or any(not 0 <= c < C for c in ch):
        raise ValueError(f"--channels names three channels below {C}")
    os.makedirs(out, exist_ok=True)
    for i, planes in render_features(model, cams, f):
        np.save(os.path.join(out, "feature_%05d.npy" % i), planes.cpu().numpy())
        frames.write_png(os.path.join(out, "feature_%05d.png" % i), _picture(planes[ch]))
    return {"rendered": len(cams), "C": C, "channels": ch, "out": out}


def depth_normal_maps(model, cameras: Sequence, *, alpha_min: float = 0.5, background=None):
    """Yields (camera index, normals float32 [3,H,W], valid bool [H,W]): the normal of every camera's rendered depth map
    (normal_prior.depth_normals: central differences of the back-projected points), camera frame, 0 where not valid."""
    from .normal_prior import depth_normals
    from .render import PipelineParams, render
    bg = torch.zeros(3, device=model.get_xyz.device) if background is None else background
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            pkg = render(cam, model, PipelineParams(), bg)
            n, valid = depth_normals(pkg["rendered_depth"], pkg["rendered_alpha"], cam, alpha_min=alpha_min)
            yield i, n, valid[0] != 0


def run_normals(model, cams, out: str, source: str = "gaussians", alpha_min: float = 0.5) -> dict:
    """source "gaussians": normal_%05d.png of the blended shortest axes; "depth": depth_normal_%05d.png of the depth-derived
    normals, next to them.  Both as (n + 1) / 2, black where not valid."""
    from . import frames
    os.makedirs(out, exist_ok=True)
    if source == "depth":
        for i, n, valid in depth_normal_maps(model, cams, alpha_min=alpha_min):
            pic = torch.where(valid.unsqueeze(0), (n + 1.0) * 0.5, torch.zeros_like(n))
            frames.write_png(os.path.join(out, "depth_normal_%05d.png" % i),
                             (pic * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu())
        return {"rendered": len(cams), "out": out, "source": source}
    for i, n, valid in render_normals(model, cams):
        pic = torch.where(valid.unsqueeze(0), (n + 1.0) * 0.5, torch.zeros_like(n))
        frames.write_png(os.path.join(out, "normal_%05d.png" % i), (pic * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu())
    return {"rendered": len(cams), "out": out}


def run_select(model, cams, features_path: str, view: str, pixel, threshold: float, model_out: str, it: int, model_path: str) -> dict:
    import shutil
    from . import segment
    f = torch.from_numpy(np.load(features_path)).to(model.get_xyz.device)
    named = [c for c in cams if str(c.image_name) == view or os.path.splitext(str(c.image_name))[0] == view]
    if not named:
        raise ValueError(f"no camera is called {view}")
    q = feature_under(model, named[0], f, int(pixel[0]), int(pixel[1]))
    mask = similar(f, q, threshold)
    part = segment.extract(model, mask.to(torch.uint8), keep=[1])
    out_dir = os.path.join(model_out, "point_cloud", "iteration_" + str(it))
    os.makedirs(out_dir, exist_ok=True)
    part.save_ply(os.path.join(out_dir, "point_cloud.ply"))
    if os.path.exists(os.path.join(model_path, "cfg_args")):
        shutil.copyfile(os.path.join(model_path, "cfg_args"), os.path.join(model_out, "cfg_args"))
    return {"P_before": int(f.shape[0]), "P_after": int(mask.sum()), "ply": os.path.join(out_dir, "point_cloud.ply")}


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.features", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--pruned", action="store_true", help="start from iteration_<n>_pruned")
    sub = p.add_subparsers(dest="command", required=True)
    s = sub.add_parser("lift")
    s.add_argument("--maps", required=True, metavar="DIR")
    s.add_argument("--views", choices=("train", "test", "all"), default="train")
    s.add_argument("--out", default=None, metavar="F.npy")
    s = sub.add_parser("render")
    s.add_argument("--features", required=True, metavar="F.npy")
    s.add_argument("--views", choices=("test", "all"), default="test")
    s.add_argument("--out", required=True, metavar="DIR")
    s.add_argument("--channels", type=int, nargs=3, default=None)
    s = sub.add_parser("normals")
    s.add_argument("--views", choices=("test", "all"), default="test")
    s.add_argument("--out", required=True, metavar="DIR")
    s.add_argument("--source", choices=("gaussians", "depth"), default="gaussians",
                   help='"depth": the normals of the rendered depth map (depth_normal_%%05d.png) in place of the Gaussians\' axes')
    s.add_argument("--alpha_min", type=float, default=0.5, help="--source depth: pixels below this alpha carry no normal")
    s = sub.add_parser("select")
    s.add_argument("--features", required=True, metavar="F.npy")
    s.add_argument("--view", required=True, metavar="NAME")
    s.add_argument("--pixel", type=int, nargs=2, required=True, metavar=("X", "Y"))
    s.add_argument("--threshold", type=float, required=True)
    s.add_argument("--model_out", required=True, metavar="NEW")
    a = p.parse_args(argv)
    model, cams, bg, it = _load(a.model_path, a.source_path, a.iteration, a.pruned)
    if a.command == "lift":
        out = a.out or os.path.join(a.model_path, "point_cloud", "iteration_" + str(it) + ("_pruned" if a.pruned else ""), "features.npy")
        res = run_lift(model, cams[a.views], bg, a.maps, out)
    elif a.command == "render":
        res = run_render(model, cams[a.views], a.features, a.out, a.channels)
    elif a.command == "normals":
        res = run_normals(model, cams[a.views], a.out, a.source, a.alpha_min)
    else:
        res = run_select(model, cams["all"], a.features, a.view, a.pixel, a.threshold, a.model_out, it, a.model_path)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
