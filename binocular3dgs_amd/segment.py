"""Segment a trained model from 2D label planes, and render per-Gaussian labels back into label maps.

label_votes() renders the cameras as evaluate.py and importance.py do (up to 8 views of one W x H per b3gs_forward_raw_batch
launch on the evaluation-owned FusedRasterizer, no gradients) and, after every launch, walks the tile lists that forward left
on the device a second time (b3gs_label_votes_batch, csrc/segment.hip).  Every blended (pixel, Gaussian) has the weight
w = alpha * T, the share of the pixel the Gaussian paints; the pixel gives that weight to the label it carries:

    votes[g, l]  sum of w over the pixels of label l that Gaussian g was blended into   (int64: the device sums rint(w 2^32))

A Gaussian then takes the label with the largest vote (assign_labels) -- the closed-form optimum of FlashSplat (Shen et al.,
"FlashSplat: 2D to 3D Gaussian Splatting Segmentation Solved Optimally", ECCV 2024); `gain` is its background bias.  One walk
serves every label; importance.contributions(masks=(labels == l)) gives the same integers with one walk per label.

render_labels() goes the other way (b3gs_label_render_batch): per pixel and label the sum S_l of w over the blended Gaussians
of label l; the pixel shows the label of the largest sum.  Labels drawn on a few training views thus reach held-out views and
spiral paths, and label_iou() scores an assignment against the planes it came from.

Labels are bytes 0 .. n_labels - 1, n_labels <= 16; a byte >= n_labels (255 by convention) is "no label".  The votes are
integer sums on the device: the same bits whatever the batch size or the camera order.  The label maps are per-pixel: the same
bits whatever the batch.  The caveat of importance.py holds: the entry that saturates a pixel stops it WITHOUT being blended.

python -m binocular3dgs_amd.segment -m MODEL_PATH [-s SOURCE] [--iteration N] (--labels DIR | --dtu_masks) [--n_labels L]
      [--views train|test|all] [--gain G0 G1 ..] [--min_share X] (--keep L.. | --remove L..) [--pruned]
      [--render test|all --out DIR] [--stats FILE.npz]

--labels DIR reads DIR/<image stem>.png or .npy per camera (a camera without a file does not vote); --dtu_masks uses the
cameras' gt_alpha_mask (object = 1, background = 0, two labels).  Writes point_cloud/iteration_<n>_segmented/point_cloud.ply
(the Gaussians whose label is kept) and, next to it, labels.npy (the label of every Gaussian of the source model); --render
also writes label_%05d.png (label_colours).  Prints one JSON line: Gaussians per label, the unassigned count, per-label IoU of
the re-rendered labels against the given planes over the voting views, P_before and P_after.
"""
from __future__ import annotations

import json
import os
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_LABELS = 16          # B3GS_MAX_LABELS
NO_LABEL = 255
# label_colours: sixteen well separated colours (the tab10 hues and six lighter ones)
PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189), (140, 86, 75), (227, 119, 194),
           (127, 127, 127), (188, 189, 34), (23, 190, 207), (174, 199, 232), (255, 187, 120), (152, 223, 138), (255, 152, 150),
           (197, 176, 213), (196, 156, 148))


def _check_n(n_labels: int) -> int:
    n = int(n_labels)
    if not 1 <= n <= MAX_LABELS:
        raise ValueError(f"n_labels is 1 .. {MAX_LABELS}, not {n_labels}")
    return n


def label_votes(model, cameras: Sequence, bg: torch.Tensor, labels: Sequence, n_labels: int, *, batch: int = 8,
                capacity: Optional[int] = None) -> torch.Tensor:
    """int64 [P, n_labels] on the device: votes[g, l] = sum of rint(w 2^32) over the pixels labelled l of all cameras;
    votes.double() / 2**32 is the weight.  labels: per camera None (the camera is skipped) or a uint8 [H,W] tensor."""
    from . import _C
    from .evaluate import _walk_batches
    L = _check_n(n_labels)
    if len(labels) != len(cameras):
        raise ValueError("one label plane (or None) per camera")
    dev = model.get_xyz.device
    P = model.get_xyz.shape[0]
    votes = torch.zeros((P, L), dtype=torch.int64, device=dev)
    used = [i for i in range(len(cameras)) if labels[i] is not None]
    if not used or P == 0:
        return votes
    cams = [cameras[i] for i in used]
    for idx, _outs, W, H, slots in _walk_batches(model, cams, bg, batch, capacity):
        views = []
        for i, s in zip(idx, slots):
            plane = labels[used[i]]
            if plane.dtype != torch.uint8 or plane.numel() != H * W:
                raise ValueError(f"camera {used[i]}: a label plane is uint8 [H,W] = [{H},{W}]")
            views.append((s.geom, s.binning, s.img, W, H, plane.reshape(H, W).to(dev).contiguous()))
        _C.label_votes(views, L, votes)
    return votes


def assign_labels(votes: torch.Tensor, *, gain=None, min_weight: float = 0.0, min_share: float = 0.0) -> torch.Tensor:
    """uint8 [P]: the label l with the largest gain[l] * votes[:, l] (float64; gain defaults to ones -- FlashSplat's background
    bias is a gain above 1 on the background label), ties to the LOWEST label; 255 where the total weight sum_l votes / 2^32 is
    <= min_weight or the winner's share of the total is < min_share.  Pure torch, any device."""
    if votes.dim() != 2 or not 1 <= votes.shape[1] <= MAX_LABELS:
        raise ValueError(f"votes is [P, L] with L <= {MAX_LABELS}")
    P, L = votes.shape
    v = votes.to(torch.float64) / 4294967296.0
    if gain is None:
        scored = v
    else:
        g = torch.as_tensor(gain, dtype=torch.float64, device=votes.device).reshape(-1)
        if g.shape[0] != L:
            raise ValueError("one gain per label")
        scored = v * g
    best = scored.max(dim=1, keepdim=True).values
    # the first (lowest) label that reaches the maximum: torch.argmax does not promise which of several equal maxima it returns
    ramp = torch.arange(L, device=votes.device).expand(P, L)
    winner = torch.where(scored == best, ramp, torch.full_like(ramp, L)).min(dim=1).values.clamp(max=L - 1)
    total = v.sum(dim=1)
    share = v.gather(1, winner.unsqueeze(1)).squeeze(1) / torch.where(total > 0, total, torch.ones_like(total))
    none = (total <= min_weight) | (share < min_share)
    return torch.where(none, torch.full_like(winner, NO_LABEL), winner).to(torch.uint8)


def render_labels(model, cameras: Sequence, bg: torch.Tensor, gaussian_labels: torch.Tensor, n_labels: int, *, batch: int = 8,
                  capacity: Optional[int] = None) -> Iterator[Tuple[int, dict]]:
    """Yields (camera index, {"label": uint8 [H,W], "weight": float32 [H,W], "rendered_alpha": [1,H,W]}) for every camera,
    launch by launch (cameras of one size together, otherwise in order): per pixel the label whose Gaussians hold the largest
    sum of blend weights (255: none) and that sum.  All tensors are the caller's to keep."""
    from . import _C
    from .evaluate import _walk_batches
    L = _check_n(n_labels)
    dev = model.get_xyz.device
    P = model.get_xyz.shape[0]
    gl = torch.as_tensor(gaussian_labels)
    if gl.dtype != torch.uint8 or gl.shape != (P,):
        raise ValueError("gaussian_labels is uint8 [P]")
    gl = gl.to(dev).contiguous()
    for idx, outs, W, H, slots in _walk_batches(model, cameras, bg, batch, capacity):
        views, res = [], []
        for s in slots:
            # (the launch writes every pixel; without Gaussians there is no launch)
            label = torch.empty((H, W), dtype=torch.uint8, device=dev) if P else torch.full((H, W), NO_LABEL, dtype=torch.uint8, device=dev)
            weight = torch.empty((H, W), dtype=torch.float32, device=dev) if P else torch.zeros((H, W), device=dev)
            views.append((s.geom, s.binning, s.img, W, H, label, weight))
            res.append({"label": label, "weight": weight})
        if P:
            _C.label_render(views, L, gl)
        for i, o, r in zip(idx, outs, res):
            r["rendered_alpha"] = o["rendered_alpha"].detach().clone()
            yield i, r


def label_iou(rendered: torch.Tensor, given: torch.Tensor, n_labels: int) -> torch.Tensor:
    """int64 [n_labels, 2]: per label the (intersection, union) pixel counts of `rendered == l` and `given == l` over the
    pixels whose `given` byte is < n_labels.  Sum it over views; IoU = [:, 0] / [:, 1].  Pure torch."""
    L = _check_n(n_labels)
    r, g = rendered.reshape(-1), given.reshape(-1).to(rendered.device)
    if r.shape != g.shape:
        raise ValueError("rendered and given hold the same pixels")
    valid = g < L
    r, g = r[valid].to(torch.int64), g[valid].to(torch.int64)
    out = torch.zeros((L, 2), dtype=torch.int64, device=rendered.device)
    for l in range(L):
        a, b = r == l, g == l
        out[l, 0], out[l, 1] = (a & b).sum(), (a | b).sum()
    return out


def extract(model, gaussian_labels: torch.Tensor, keep):
    """A new GaussianModel of the Gaussians whose label is in `keep` (importance.prune of that mask)."""
    from . import importance
    gl = torch.as_tensor(gaussian_labels)
    keep = torch.as_tensor(list(keep), dtype=gl.dtype, device=gl.device)
    return importance.prune(model, torch.isin(gl, keep))


def label_colours(label_map: torch.Tensor) -> torch.Tensor:
    """A label map as a picture: uint8 [H,W,3] on the map's device, PALETTE[l] for l < 16, black for 255 (and any other byte)."""
    pal = torch.tensor(PALETTE + ((0, 0, 0),), dtype=torch.uint8, device=label_map.device)
    return pal[label_map.to(torch.int64).clamp(max=MAX_LABELS)]


def _palette_as_gray(data: bytes) -> bytes:
    """The bytes of an 8-bit palette PNG with its IHDR rewritten to 8-bit gray: the samples ARE the palette indices, one byte
    per pixel in both layouts, so frames.read_png then returns the index plane.  (read_png itself refuses colour type 3.)"""
    import struct
    import zlib
    head = bytearray(data[16:29])            # the 13 IHDR bytes behind signature, length and tag
    head[9] = 0
    return data[:16] + bytes(head) + struct.pack(">I", zlib.crc32(b"IHDR" + bytes(head)) & 0xFFFFFFFF) + data[33:]


def read_labels(path: str) -> torch.Tensor:
    """uint8 [H,W] label plane (CPU) from a .npy file (an integer [H,W] array with values 0 .. 255) or an 8-bit gray or palette
    PNG (palette: the indices are the labels, the colours are not looked at)."""
    from . import frames
    if path.lower().endswith(".npy"):
        a = np.load(path)
        if a.ndim != 2 or a.dtype.kind not in "ui" or (a.size and (a.min() < 0 or a.max() > 255)):
            raise ValueError(f"{path}: a label plane is an integer [H,W] array of 0 .. 255")
        return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint8)))
    with open(path, "rb") as fp:
        data = fp.read()
    if data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[24] == 8 and data[25] == 3:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            gray = os.path.join(tmp, "indices.png")
            with open(gray, "wb") as fp:
                fp.write(_palette_as_gray(data))
            a = frames.read_png(gray)
    else:
        a = frames.read_png(path)
    if a.ndim != 2:
        raise ValueError(f"{path}: a label plane is an 8-bit gray or palette PNG, not {a.shape[2]} channels")
    return torch.from_numpy(np.ascontiguousarray(a))


def _find_labels(directory: str, cam) -> Optional[torch.Tensor]:
    stem = os.path.splitext(str(cam.image_name))[0]
    for ext in (".png", ".npy"):
        path = os.path.join(directory, stem + ext)
        if os.path.exists(path):
            plane = read_labels(path)
            if plane.shape != (int(cam.image_height), int(cam.image_width)):
                raise ValueError(f"{path}: {tuple(plane.shape)} labels for a {cam.image_height} x {cam.image_width} camera")
            return plane
    return None


def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, labels: Optional[str] = None, dtu_masks: bool = False,
        n_labels: Optional[int] = None, views: str = "train", gain=None, min_share: float = 0.0, keep=None, remove=None,
        pruned: bool = False, render: Optional[str] = None, out: Optional[str] = None, stats: Optional[str] = None) -> dict:
    from . import frames
    from .gaussian_model import GaussianModel
    from .scene import Scene
    from .spiral import max_iteration, read_cfg_args
    if (labels is None) == (not dtu_masks):
        raise ValueError("one of --labels DIR and --dtu_masks")
    if (keep is None) == (remove is None):
        raise ValueError("one of --keep and --remove")
    if render and not out:
        raise ValueError("--render needs --out DIR")
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
    cams = {"train": train, "test": test, "all": train + test}[views]
    if dtu_masks:
        L = 2
        planes = [None if getattr(c, "gt_alpha_mask", None) is None else (c.gt_alpha_mask.reshape(int(c.image_height), int(c.image_width)) > 0.5).to(torch.uint8)
                  for c in cams]
    else:
        planes = [_find_labels(labels, c) for c in cams]
        seen = [int(p[p != NO_LABEL].max()) for p in planes if p is not None and bool((p != NO_LABEL).any())]
        L = int(n_labels) if n_labels is not None else min(MAX_LABELS, max(seen, default=0) + 1)
    L = _check_n(L)
    if all(p is None for p in planes):
        raise ValueError(f"no {views} camera has a label plane")
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    votes = label_votes(model, cams, bg, planes, L)
    gl = assign_labels(votes, gain=gain, min_share=min_share)
    kept = sorted(set(int(l) for l in keep)) if keep is not None else [l for l in range(L) if l not in set(int(r) for r in remove)]
    part = extract(model, gl, kept)
    out_dir = os.path.join(model_path, "point_cloud", "iteration_" + str(it) + "_segmented")
    os.makedirs(out_dir, exist_ok=True)
    part.save_ply(os.path.join(out_dir, "point_cloud.ply"))
    np.save(os.path.join(out_dir, "labels.npy"), gl.cpu().numpy())
    # the assignment scored against its own inputs: the labels re-rendered over the voting views
    voting = [i for i, p in enumerate(planes) if p is not None]
    iou = torch.zeros((L, 2), dtype=torch.int64, device=gl.device)
    for j, r in render_labels(model, [cams[i] for i in voting], bg, gl, L):
        iou += label_iou(r["label"], planes[voting[j]].to(gl.device), L)
    iou = iou.cpu().numpy()
    counts = torch.bincount(gl.to(torch.int64), minlength=256).cpu().numpy()
    res = {"P_before": int(gl.shape[0]), "P_after": int(part._xyz.shape[0]), "n_labels": L, "kept": kept,
           "gaussians_per_label": [int(counts[l]) for l in range(L)], "unassigned": int(counts[L:].sum()),
           "iou": [float(a) / float(b) if b else None for a, b in iou.tolist()], "voting_views": len(voting), "iteration": it,
           "views": views, "ply": os.path.join(out_dir, "point_cloud.ply")}
    if render:
        os.makedirs(out, exist_ok=True)
        rcams = {"test": test, "all": train + test}[render]
        paths = [None] * len(rcams)
        for j, r in render_labels(model, rcams, bg, gl, L):
            paths[j] = frames.write_png(os.path.join(out, "label_%05d.png" % j), label_colours(r["label"]).cpu())
        res["rendered"] = len(paths)
    if stats:
        np.savez(stats, votes_q32=votes.cpu().numpy(), labels=gl.cpu().numpy(), iou=iou)
    print(json.dumps(res))
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.segment", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--labels", default=None, metavar="DIR", help="DIR/<image stem>.png or .npy per camera")
    g.add_argument("--dtu_masks", action="store_true", help="the cameras' gt_alpha_mask: object = 1, background = 0")
    p.add_argument("--n_labels", type=int, default=None)
    p.add_argument("--views", choices=("train", "test", "all"), default="train")
    p.add_argument("--gain", type=float, nargs="+", default=None, help="one factor per label on its votes")
    p.add_argument("--min_share", type=float, default=0.0)
    k = p.add_mutually_exclusive_group(required=True)
    k.add_argument("--keep", type=int, nargs="+", default=None)
    k.add_argument("--remove", type=int, nargs="+", default=None)
    p.add_argument("--pruned", action="store_true", help="start from iteration_<n>_pruned")
    p.add_argument("--render", choices=("test", "all"), default=None)
    p.add_argument("--out", default=None, metavar="DIR")
    p.add_argument("--stats", default=None, metavar="FILE.npz")
    a = p.parse_args(argv)
    run(a.model_path, a.source_path, a.iteration, a.labels, a.dtu_masks, a.n_labels, a.views, a.gain, a.min_share, a.keep, a.remove,
        a.pruned, a.render, a.out, a.stats)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
