"""Levels of detail of a trained model: the small Gaussians of one grid cell merged into the one that covers the same space.

python -m binocular3dgs_amd.lod -m MODEL_PATH [-s SOURCE] [--iteration N] [--pruned] [--ratios 0.5 0.25 .. | --cell C]
      [--views train|test|all | --uniform] [--evaluate] [--model_out NEW]

importance.prune drops Gaussians and compress quantises their rows; coarsen() replaces every cluster -- the Gaussians of one
cell of a grid of edge `cell` whose largest scale is at most `cell` -- by the Gaussian with the mass-weighted mean and
covariance of the cluster's mixture (mass = weight * opacity * s0 s1 s2), its eigen-decomposition as scales and rotation, the
opacity that preserves the summed mass, and the mass-weighted mean of the SH coefficients (they are in the world frame).  A
Gaussian larger than the cell passes through untouched: a background splat does not swallow its neighbours.  The rule is
stated in include/b3gs_raster.h and restated in tests/lod_ref.py, which the device code (csrc/lod.hip) matches bit for bit.

The kernel sees ACTIVATED values (the model's own accessors) and this module converts back with torch.log and the inverse
sigmoid; an output row with one member takes the raw parameter rows of its source instead, so what is not merged keeps its
bits.  One host read per coarsen(): the totals, between count and emit.

The command line writes <MODEL_PATH>/point_cloud/iteration_<n>_lod<k>/point_cloud.ply per level (k = 1, 2, ..) and lod.json
(cell, counts, mass) next to each, and prints one JSON line.  --views weights the members by importance.contributions(...)
.weight over those cameras (the default, train), --uniform by 1.  --evaluate adds PSNR / SSIM of every level on the test
cameras against the ground truth and against the full model's own renders.  --model_out NEW also writes the LAST level as
NEW/point_cloud/iteration_<n> with cfg_args: a -m folder for the other commands.
"""
from __future__ import annotations

import json
import os
from typing import Optional, Sequence

import torch

MAX_CELLS = 1024
TOTALS = ("clusters", "pass_through", "merged_members", "nonfinite_rows", "over_range_rows", "rows", "extent_bits")


def _activated(model):
    with torch.no_grad():
        return (model.get_xyz.detach().contiguous(), model.get_scaling.detach().contiguous(), model._rotation.detach().contiguous(),
                model.get_opacity.detach().reshape(-1).contiguous(), model._features_dc.detach().contiguous(),
                model._features_rest.detach().contiguous())


def _weights(weights, P, dev):
    if weights is None:
        return None
    w = torch.as_tensor(weights).to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
    if w.shape[0] != P:
        raise ValueError("coarsen: one weight per Gaussian")
    return w


def _count(acts, w, cell):
    """count and the ONE host read -> (workspace, totals list)"""
    from . import _C
    ws, totals = _C.gaussian_merge_count(*acts, w, float(cell))
    return ws, totals.tolist()                                            # the one host read


def merge_activated(positions, scales, quaternions, opacities, features_dc, features_rest, cell, weights=None):
    """The device rule on activated tensors -> (positions, scales, quaternions, opacities, features_dc, features_rest, cluster_of,
    members, totals dict).  Rows that are not finite, or beyond 1024 cells of an axis, raise B3gsError with their count (the
    message of b3gs_last_error; for the cells, with the smallest cell that would do)."""
    from . import _C
    from ._lib import B3gsError
    from .mesh_tools import _extent_of, smallest_cell
    acts = (positions, scales, quaternions, opacities, features_dc, features_rest)
    w = _weights(weights, positions.shape[0], positions.device)
    ws, t = _count(acts, w, cell)
    try:
        out = _C.gaussian_merge_emit(*acts, w, float(cell), ws, t[:5])
    except B3gsError as e:
        if t[4] and not t[3]:
            raise B3gsError(f"{e}: the smallest admissible cell is {smallest_cell(_extent_of(t[6]))!r}") from None
        raise
    return tuple(out) + (dict(zip(TOTALS, t)),)


def coarsen(model, cell: float, weights=None, return_stats: bool = False):
    """-> (GaussianModel, cluster_of int32 [P]: the output row of every input, members int32 [rows]: the member count of every
    row); with return_stats also level_stats-style totals.  SH degrees are carried over, no optimizer state is kept (as
    importance.prune).  weights: None or [P] >= 0 (importance.contributions(...).weight, say)."""
    from .gaussian_model import GaussianModel
    if not float(cell) > 0.0:
        raise ValueError("coarsen: the cell is positive")
    with torch.no_grad():
        acts = _activated(model)
        pos, sc, quat, al, dc, rest, cluster_of, members, t = merge_activated(*acts, cell, weights)
        raw_sc = model.scaling_inverse_activation(sc)
        raw_al = model.inverse_opacity_activation(al).reshape(-1, 1)
        # rows with one member: the raw parameter rows of their source (log(exp(x)) is not x)
        P = acts[0].shape[0]
        src = torch.zeros(pos.shape[0], dtype=torch.int64, device=pos.device)
        src[cluster_of.long()] = torch.arange(P, device=pos.device)
        one = members == 1
        raw_sc = torch.where(one[:, None], model._scaling.detach()[src], raw_sc)
        raw_al = torch.where(one[:, None], model._opacity.detach().reshape(-1, 1)[src], raw_al)
        new = GaussianModel.from_tensors(pos, dc, rest, raw_sc, quat, raw_al, sh_degree=model.max_sh_degree,
                                         active_sh_degree=model.active_sh_degree, requires_grad=model._xyz.requires_grad)
    if return_stats:
        return new, cluster_of, members, t
    return new, cluster_of, members


def _extent(model) -> float:
    xyz = model.get_xyz.detach()
    return float((xyz.amax(dim=0) - xyz.amin(dim=0)).max())


def coarsen_to(model, target: int, weights=None, steps: int = 24):
    """Geometric bisection of the cell, as mesh_tools.simplify_to: -> (the model with the largest count <= target that was found,
    cluster_of, members, the cell used).  Count-only trials (one host read each), then one coarsen().  ValueError when even a
    cell of the whole extent leaves more than `target` (Gaussians larger than the extent pass through)."""
    from .mesh_tools import smallest_cell
    P = int(model.get_xyz.shape[0])
    if target < 1:
        raise ValueError("coarsen_to: target is at least 1")
    if P == 0:
        raise ValueError("coarsen_to: the model is empty")
    extent = _extent(model)
    if not extent < float("inf"):
        raise ValueError("coarsen_to: the positions span no finite extent")
    with torch.no_grad():
        acts = _activated(model)
        w = _weights(weights, P, acts[0].device)
        # twice the larger of the extent and the largest scale: one cell, every Gaussian mergeable, one row
        hi = 2.0 * max(extent, float(acts[1].amax()))
        lo = min(smallest_cell(extent), hi) if extent > 0.0 else hi

        def rows(cell):
            return _count(acts, w, cell)[1][5]

        if rows(lo) <= target:
            hi = lo
        else:
            if rows(hi) > target:
                raise ValueError(f"coarsen_to: a cell of {hi:g} still leaves {rows(hi)} Gaussians")
            for _ in range(max(0, steps - 2)):
                mid = (lo * hi) ** 0.5
                if not lo < mid < hi:
                    break
                if rows(mid) <= target:
                    hi = mid
                else:
                    lo = mid
    return coarsen(model, hi, weights) + (hi,)


def build_levels(model, ratios: Sequence[float] = (0.5, 0.25, 0.125), weights=None, return_cells: bool = False):
    """One model per ratio (target = max(1, floor(ratio * P))), every level from the FULL model so that errors do not compound."""
    P = int(model.get_xyz.shape[0])
    levels, cells = [], []
    for r in ratios:
        if not 0.0 < r <= 1.0:
            raise ValueError("build_levels: a ratio is in (0, 1]")
        m, _, _, cell = coarsen_to(model, max(1, int(r * P)), weights)
        levels.append(m)
        cells.append(cell)
    return (levels, cells) if return_cells else levels


def _mass(model) -> float:
    with torch.no_grad():
        return float((model.get_opacity.double().reshape(-1) * torch.prod(model.get_scaling.double(), dim=1)).sum())


def level_stats(model, level, members=None) -> dict:
    """Counts, the share of the inputs that went into merged rows, and the total mass sum alpha_i s0 s1 s2 before and after."""
    P, Q = int(model.get_xyz.shape[0]), int(level.get_xyz.shape[0])
    res = {"P_before": P, "P_after": Q, "mass_before": _mass(model), "mass_after": _mass(level)}
    if members is not None:
        res["merged_share"] = float(members[members >= 2].sum()) / P if P else 0.0
    return res


# ---- the command line ------------------------------------------------------------------------------------------------------------
def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, pruned: bool = False, ratios=None,
        cell: Optional[float] = None, views: str = "train", uniform: bool = False, evaluate: bool = False,
        model_out: Optional[str] = None) -> dict:
    import copy
    from . import importance
    from .evaluate import evaluate_views, render_views
    from .gaussian_model import GaussianModel
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it) + ("_pruned" if pruned else ""), "point_cloud.ply"))
    white = bool(cfg.get("white_background", False))
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    train = test = None
    if not uniform or evaluate:
        from .scene import Scene
        source_path = source_path or cfg.get("source_path")
        if not source_path:
            raise ValueError("no source path: pass -s or keep cfg_args next to the model")
        scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                                   dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                                   resolution=cfg.get("resolution", -1), white_background=white,
                                   init_points=cfg.get("init_points", "matcher"), shuffle=False)
        train, test = list(scene.getTrainCameras()), list(scene.getTestCameras())
    weights = None
    if not uniform:
        cams = {"train": train, "test": test, "all": train + test}[views]
        if not cams:
            raise ValueError(f"{source_path}: no {views} cameras")
        weights = importance.contributions(model, cams, bg).weight
    if cell is not None:
        built = [coarsen(model, cell, weights) + (float(cell),)]
    else:
        P = int(model.get_xyz.shape[0])
        built = [coarsen_to(model, max(1, int(r * P)), weights) for r in (ratios or (0.5, 0.25, 0.125))]
    res = {"iteration": it, "weights": "uniform" if uniform else views, "levels": []}
    own = None
    if evaluate:
        if not test:
            raise ValueError(f"{source_path}: --evaluate needs test cameras")
        e = evaluate_views(model, test, bg, mode="report")
        res["full"] = {k: e[k] for k in ("PSNR", "SSIM")}
        own = []
        for c, img in zip(test, render_views(model, test, bg)):
            c2 = copy.copy(c)
            c2.original_image = img.detach().clone()
            own.append(c2)
    out_dir = None
    for k, (level, _, members, used) in enumerate(built, start=1):
        out_dir = os.path.join(model_path, "point_cloud", "iteration_" + str(it) + "_lod" + str(k))
        os.makedirs(out_dir, exist_ok=True)
        level.save_ply(os.path.join(out_dir, "point_cloud.ply"))
        info = dict(level_stats(model, level, members), cell=used, ply=os.path.join(out_dir, "point_cloud.ply"))
        if evaluate:
            e = evaluate_views(level, test, bg, mode="report")
            info["ground_truth"] = {k2: e[k2] for k2 in ("PSNR", "SSIM")}
            e = evaluate_views(level, own, bg, mode="report")
            info["full_model"] = {k2: e[k2] for k2 in ("PSNR", "SSIM")}
        with open(os.path.join(out_dir, "lod.json"), "w") as fp:
            json.dump(info, fp)
        res["levels"].append(info)
    if model_out and out_dir:
        import shutil
        new_dir = os.path.join(model_out, "point_cloud", "iteration_" + str(it))
        os.makedirs(new_dir, exist_ok=True)
        for f in ("point_cloud.ply", "lod.json"):
            shutil.copyfile(os.path.join(out_dir, f), os.path.join(new_dir, f))
        if os.path.exists(os.path.join(model_path, "cfg_args")):
            shutil.copyfile(os.path.join(model_path, "cfg_args"), os.path.join(model_out, "cfg_args"))
        res["model"] = os.path.abspath(model_out)
    print(json.dumps(res))
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.lod", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--pruned", action="store_true", help="start from iteration_<n>_pruned")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--ratios", type=float, nargs="+", default=None, help="one level per ratio of the Gaussian count (default 0.5 0.25 0.125)")
    g.add_argument("--cell", type=float, default=None, help="one level at this cell edge (world units)")
    w = p.add_mutually_exclusive_group()
    w.add_argument("--views", choices=("train", "test", "all"), default="train", help="weight by the render contribution over these cameras")
    w.add_argument("--uniform", action="store_true", help="weight every Gaussian by 1")
    p.add_argument("--evaluate", action="store_true")
    p.add_argument("--model_out", default=None, metavar="NEW_MODEL_PATH",
                   help="also write the last level as NEW_MODEL_PATH/point_cloud/iteration_<n>, with cfg_args")
    a = p.parse_args(argv)
    run(a.model_path, a.source_path, a.iteration, a.pruned, a.ratios, a.cell, a.views, a.uniform, a.evaluate, a.model_out)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
