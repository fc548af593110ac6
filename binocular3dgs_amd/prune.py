"""Cut a trained model to the Gaussians that carry its renders (importance.py over the cameras of the dataset folder).

python -m binocular3dgs_amd.prune -m MODEL_PATH [-s SOURCE] [--iteration N] [--views train|test|all]
      [--rule weight|significance] [--keep F | --min_score X] [--min_hits N] [--never_dominant] [--evaluate] [--stats FILE.npz]

Loads <MODEL_PATH>/point_cloud/iteration_<n>/point_cloud.ply and the cameras as evaluate.py does, computes the per-Gaussian
contribution over the chosen cameras, keeps the Gaussians the criteria select (ANDed) and writes
<MODEL_PATH>/point_cloud/iteration_<n>_pruned/point_cloud.ply.  --stats also writes the four arrays (weight, hits, dominant,
wmax) and the kept mask.  Prints one JSON line: P before and after, the share of Gaussians with zero hits, the share that is
never dominant, the share of the weight that was kept; with --evaluate the evaluate_views means (mode "report") of the test
cameras before and after.
"""
from __future__ import annotations

import json
import os
from typing import Optional

import numpy as np
import torch


def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, views: str = "train", rule: str = "weight",
        keep: Optional[float] = None, min_score: Optional[float] = None, min_hits: Optional[int] = None,
        never_dominant: bool = False, evaluate: bool = False, stats: Optional[str] = None) -> dict:
    from . import importance
    from .evaluate import evaluate_views
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
    train, test = list(scene.getTrainCameras()), list(scene.getTestCameras())
    cams = {"train": train, "test": test, "all": train + test}[views]
    if not cams:
        raise ValueError(f"{source_path}: no {views} cameras")
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    c = importance.contributions(model, cams, bg)
    sc = importance.score(c, model, rule)
    mask = importance.select(sc, keep=keep, min_score=min_score, min_hits=min_hits, never_dominant=never_dominant, contrib=c)
    pruned = importance.prune(model, mask)
    out_dir = os.path.join(model_path, "point_cloud", "iteration_" + str(it) + "_pruned")
    os.makedirs(out_dir, exist_ok=True)
    pruned.save_ply(os.path.join(out_dir, "point_cloud.ply"))
    P = int(mask.shape[0])
    total = float(c.weight.sum())
    res = {"P_before": P, "P_after": int(mask.sum()), "zero_hit_share": float((c.hits == 0).double().mean()) if P else 0.0,
           "never_dominant_share": float((c.dominant == 0).double().mean()) if P else 0.0,
           "weight_share_kept": float(c.weight[mask].sum()) / total if total > 0 else 0.0,
           "iteration": it, "views": views, "rule": rule, "ply": os.path.join(out_dir, "point_cloud.ply")}
    if stats:
        np.savez(stats, weight=c.weight.cpu().numpy(), hits=c.hits.cpu().numpy(), dominant=c.dominant.cpu().numpy(),
                 wmax=c.wmax.cpu().numpy(), kept=mask.cpu().numpy())
    if evaluate:
        if not test:
            raise ValueError(f"{source_path}: --evaluate needs test cameras")
        for tag, m in (("before", model), ("after", pruned)):
            e = evaluate_views(m, test, bg, mode="report")
            res[tag] = {k: e[k] for k in ("PSNR", "SSIM", "L1")}
    print(json.dumps(res))
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.prune", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--views", choices=("train", "test", "all"), default="train")
    p.add_argument("--rule", choices=("weight", "significance"), default="weight")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--keep", type=float, default=None, help="fraction of the Gaussians to keep, by score")
    g.add_argument("--min_score", type=float, default=None)
    p.add_argument("--min_hits", type=int, default=None)
    p.add_argument("--never_dominant", action="store_true", help="drop the Gaussians that are the largest weight of no pixel")
    p.add_argument("--evaluate", action="store_true")
    p.add_argument("--stats", default=None, metavar="FILE.npz")
    a = p.parse_args(argv)
    run(a.model_path, a.source_path, a.iteration, a.views, a.rule, a.keep, a.min_score, a.min_hits, a.never_dominant, a.evaluate,
        a.stats)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
