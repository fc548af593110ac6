"""Localise a photo in a trained model: photometric pose refinement from a pose guess (pose.refine_pose, INTEGRATION.md
section 24).

python -m binocular3dgs_amd.localize -m MODEL_PATH --image PHOTO.png (--init_view NAME | --init_matrix F.txt --fov DEG)
                                     [-s SOURCE] [--iteration N] [--iters N] [--scales 4 2 1] [--out pose.json]

--init_view NAME takes the pose, field of view and image size of the dataset camera whose image name is NAME (train or test);
--init_matrix F.txt a 4x4 world-to-camera matrix in COLMAP's convention (x_cam = R x + t) with --fov, the horizontal field of view
in degrees.  The photo is resized to the camera's image size (the bicubic resize of ground_truth).  Prints one JSON line: the
pose as COLMAP qvec (w, x, y, z; unit, w >= 0) / tvec, the final loss, the twist from the guess (about the mean of the model's
positions, world frame) and the iterations; --out also writes it to a file.
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch


def colmap_pose(cam):
    """(qvec (w, x, y, z) with w >= 0, tvec) of a camera: x_cam = R(q) x + t"""
    from .edit import Similarity, _camera_pose
    R, C = _camera_pose(cam)                     # camera-to-world rotation, centre
    return Similarity(R.T).quaternion(), -(R.T @ C)


def run(model_path: str, image: str, init_view: Optional[str] = None, init_matrix: Optional[str] = None, fov: Optional[float] = None,
        source_path: Optional[str] = None, iteration: int = -1, iters: int = 100, scales: Sequence[int] = (4, 2, 1),
        out: Optional[str] = None) -> dict:
    from .camera import Camera, focal2fov, fov2focal
    from .dataset_readers import read_image
    from .gaussian_model import GaussianModel
    from .ground_truth import prepare_ground_truth
    from .pose import refine_pose
    from .spiral import max_iteration, read_cfg_args
    if (init_view is None) == (init_matrix is None):
        raise ValueError("exactly one of --init_view and --init_matrix")
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it), "point_cloud.ply"))
    white = bool(cfg.get("white_background", False))
    photo = read_image(image)
    if init_view is not None:
        from .scene import Scene
        source_path = source_path or cfg.get("source_path")
        if not source_path:
            raise ValueError("no source path: pass -s or keep cfg_args next to the model")
        scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                                   dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                                   resolution=cfg.get("resolution", -1), white_background=white,
                                   init_points=cfg.get("init_points", "matcher"), shuffle=False)
        cams = list(scene.getTrainCameras()) + list(scene.getTestCameras())
        match = [c for c in cams if c.image_name == init_view or os.path.splitext(str(c.image_name))[0] == os.path.splitext(init_view)[0]]
        if not match:
            raise ValueError(f"--init_view {init_view}: no such camera among {sorted(str(c.image_name) for c in cams)}")
        guess = match[0]
    else:
        if fov is None:
            raise ValueError("--init_matrix needs --fov (the horizontal field of view in degrees)")
        M = np.loadtxt(init_matrix, dtype=np.float64)
        if M.shape != (4, 4) or not np.isfinite(M).all() or np.abs(M[:3, :3] @ M[:3, :3].T - np.eye(3)).max() > 1e-6:
            raise ValueError(f"{init_matrix}: a finite 4x4 world-to-camera matrix with an orthogonal rotation")
        Hp, Wp = photo.shape[:2]
        fovx = math.radians(fov)
        guess = Camera(M[:3, :3].T, M[:3, 3], fovx, focal2fov(fov2focal(fovx, Wp), Hp), Wp, Hp, device="cuda")
    W, H = int(guess.image_width), int(guess.image_height)
    target = prepare_ground_truth([photo], (W, H), white_background=white, device="cuda")[0][0]
    if target.shape[0] == 1:
        target = target.expand(3, H, W).contiguous()
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    cam, hist = refine_pose(model, guess, target, iters=int(iters), scales=tuple(scales), bg=bg)
    q, t = colmap_pose(cam)
    res = {"qvec": [float(v) for v in q], "tvec": [float(v) for v in t], "loss": hist["loss"][-1] if hist["loss"] else None,
           "initial_loss": hist["loss"][0] if hist["loss"] else None, "twist": hist["twist"], "pivot": hist["pivot"],
           "iterations": len(hist["loss"]), "width": W, "height": H, "iteration": it}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as fp:
            fp.write(line + "\n")
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.localize", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--image", required=True, metavar="PHOTO.png")
    p.add_argument("--init_view", default=None, metavar="NAME", help="start from the dataset camera of this image name")
    p.add_argument("--init_matrix", default=None, metavar="F.txt", help="start from this 4x4 world-to-camera matrix (needs --fov)")
    p.add_argument("--fov", type=float, default=None, help="horizontal field of view in degrees (with --init_matrix)")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--scales", type=int, nargs="+", default=[4, 2, 1])
    p.add_argument("--out", default=None, metavar="pose.json")
    a = p.parse_args(argv)
    if (a.init_view is None) == (a.init_matrix is None):
        p.error("exactly one of --init_view and --init_matrix")
    run(a.model_path, a.image, a.init_view, a.init_matrix, a.fov, a.source_path, a.iteration, a.iters, a.scales, a.out)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
