"""Novel-view spiral paths: the cameras the reference's spiral.py renders (scene/dataset_readers.py:314-399, CreateLLFFSpiral /
CreateDTUSpiral, with utils/pose_utils.py:425-538 and utils/camera_utils.py:69-95), as this project's camera.Camera objects.

From the [N, 17] rows of an LLFF / DTU `poses_bounds.npy` (a 3x5 [R | t | hwf] block and the near / far bounds per view):
  1. axes reordered by the fixed rotation [[0,-1,0,0], [1,0,0,0], [0,0,1,0], [0,0,0,1]] (float32) on the right;
  2. recentred on the average pose (mean position, mean z axis, mean y axis as up);
  3. the spiral, n_rots = 2 turns with zrate = 0.5, positions scaled by per-axis percentiles of the recentred positions:
     LLFF  90th percentile, every camera looks along position - lookat, lookat at the focus depth
           1 / (0.25 / (0.9 min bound) + 0.75 / (5 max bound)) on the average pose's z axis;
     DTU   positions normalised by their largest absolute coordinate first, 60th percentile, every camera looks away from
           the point nearest to all optical axes (least squares) and the scale is restored afterwards;
  4. moved back by the average pose, the reordering undone (the float32 inverse of the rotation), the first view's hwf column;
  5. converted to a world-to-camera R, T (the axes swapped to x = y', y = x', z = -z', then inverted), with FoVx / FoVy from
     the focal length of the hwf column and its height / width, which stay floats until the size rule of loadRenderCam:
     resolution in {1, 2, 4, 8}: round(orig / resolution); -1: widths above 6400 are scaled to 6400; otherwise the target
     width.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import numpy as np

from .camera import Camera, focal2fov

_AXES = np.array([[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)


def _unit(x: np.ndarray) -> np.ndarray:
    return x / np.linalg.norm(x)


def _look(z: np.ndarray, up: np.ndarray, position: np.ndarray) -> np.ndarray:
    """3x4 camera-to-world [x | y | z | position] with z along `z` and x = up x z."""
    z = _unit(z)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, position], axis=1)


def _homogeneous(p: np.ndarray) -> np.ndarray:
    """[..., 3, 4] -> [..., 4, 4] with the row [0, 0, 0, 1]."""
    row = np.broadcast_to([0, 0, 0, 1.0], p[..., :1, :4].shape)
    return np.concatenate([p[..., :3, :4], row], axis=-2)


def _mean_pose(poses: np.ndarray) -> np.ndarray:
    centre = poses[:, :3, 3].mean(0)
    return _look(poses[:, :3, 2].mean(0), poses[:, :3, 1].mean(0), centre)


def _to_frame(poses: np.ndarray, frame: np.ndarray) -> np.ndarray:
    return (np.linalg.inv(_homogeneous(frame)) @ _homogeneous(poses))[..., :3, :4]


def _from_frame(poses: np.ndarray, frame: np.ndarray) -> np.ndarray:
    return (_homogeneous(frame) @ _homogeneous(poses))[..., :3, :4]


def _angles(n_frames: int, n_rots: int) -> np.ndarray:
    return np.linspace(0.0, 2.0 * np.pi * n_rots, n_frames, endpoint=False)


def _orbit(c2w: np.ndarray, radii: np.ndarray, theta: float, zrate: float) -> np.ndarray:
    offset = radii * np.array([np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.0])
    return c2w @ offset


def _spiral_llff(poses: np.ndarray, bounds: np.ndarray, n_frames: int, n_rots: int = 2, zrate: float = 0.5) -> np.ndarray:
    near, far = bounds.min() * 0.9, bounds.max() * 5.0
    w = 0.75
    focus = 1 / ((1 - w) / near + w / far)
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), 90, 0), [1.0]])
    c2w = _mean_pose(poses)
    up = poses[:, :3, 1].mean(0)
    target = c2w @ np.array([0, 0, -focus, 1.0])
    out = []
    for theta in _angles(n_frames, n_rots):
        position = _orbit(c2w, radii, theta, zrate)
        out.append(_look(position - target, up, position))
    return np.stack(out, axis=0)


def _nearest_to_axes(poses: np.ndarray) -> np.ndarray:
    """Least-squares point nearest to every camera's optical axis (line through the position along the z axis)."""
    d, o = poses[:, :3, 2:3], poses[:, :3, 3:4]
    proj = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    normal = np.transpose(proj, [0, 2, 1]) @ proj
    return np.linalg.inv(normal.mean(0)) @ (normal @ o).mean(0)[:, 0]


def _spiral_dtu(poses: np.ndarray, n_frames: int, n_rots: int = 2, zrate: float = 0.5, perc: float = 60) -> np.ndarray:
    radii = np.concatenate([np.percentile(np.abs(poses[:, :3, 3]), perc, 0), [1.0]])
    c2w = _mean_pose(poses)
    up = poses[:, :3, 1].mean(0)
    focus = _nearest_to_axes(poses)
    out = []
    for theta in _angles(n_frames, n_rots):
        position = _orbit(c2w, radii, theta, zrate)
        out.append(_look(position - focus, up, position))
    return np.stack(out, axis=0)


def spiral_poses(poses_bounds: np.ndarray, *, dtu: bool, n_frames: int = 180) -> np.ndarray:
    """[n_frames, 3, 5] camera-to-world poses with the hwf column, in the layout of poses_bounds.npy."""
    arr = np.asarray(poses_bounds)
    if arr.ndim != 2 or arr.shape[1] != 17 or arr.shape[0] < 1:
        raise ValueError("poses_bounds must be an [N, 17] array")
    blocks = arr[:, :-2].reshape([-1, 3, 5])
    bounds = arr[:, -2:]
    undo = np.linalg.inv(_AXES)
    poses = blocks[:, :3, :4] @ _AXES
    centred = _to_frame(poses, _mean_pose(poses))
    if dtu:
        s = np.max(np.abs(centred[:, :3, -1]))
        centred[:, :3, -1] /= s
        path = _spiral_dtu(centred, n_frames)
        path[:, :3, -1] *= s
    else:
        path = _spiral_llff(centred, bounds, n_frames)
    path = _from_frame(path, _mean_pose(poses)) @ undo
    hwf = np.tile(blocks[:1, :3, 4:], (path.shape[0], 1, 1))
    return np.concatenate([path, hwf], -1)


def _world_to_camera(path: np.ndarray) -> Tuple[np.ndarray, np.ndarray, float, float, float]:
    """-> R (camera-to-world rotation as Camera stores it), T, height, width, focal (floats of the hwf column)."""
    p = np.concatenate([path[:, :, 1:2], path[:, :, 0:1], -path[:, :, 2:3], path[:, :, 3:4], path[:, :, 4:5]], 2)
    H, W, fl = p[0, :, -1]
    row = np.tile(np.array([0, 0, 0, 1.0]).reshape([1, 1, 4]), (p.shape[0], 1, 1))
    w2c = np.linalg.inv(np.concatenate([p[..., :4], row], 1))
    return np.transpose(w2c[:, :3, :3], [0, 2, 1]), w2c[:, :3, -1], H, W, fl


def render_size(orig_w: float, orig_h: float, resolution) -> Tuple[int, int]:
    """utils/camera_utils.py:69-90 (loadRenderCam) at resolution_scale 1: loadCam's rule (ground_truth.scaled_size) with the
    width cap of resolution -1 at 6400."""
    from .ground_truth import scaled_size
    return scaled_size(orig_w, orig_h, resolution, 6400)


def spiral_cameras(poses_bounds: np.ndarray, *, dtu: bool, n_frames: int = 180, resolution=1,
                   device="cuda") -> List[Camera]:
    """The render cameras of spiral.py for an [N, 17] poses_bounds array (DTU: dtu=True)."""
    R, T, H, W, fl = _world_to_camera(spiral_poses(poses_bounds, dtu=dtu, n_frames=n_frames))
    fovy, fovx = focal2fov(fl, H), focal2fov(fl, W)
    width, height = render_size(W, H, resolution)
    return [Camera(R[i], T[i], fovx, fovy, width, height, uid=i, device=device) for i in range(R.shape[0])]


def is_dtu(source_path: str) -> bool:
    """scene/__init__.py:162: the reference takes every source path containing 'scan' for DTU."""
    return "scan" in source_path


def spiral_cameras_from_dir(source_path: str, *, n_frames: int = 180, resolution=1, device="cuda") -> List[Camera]:
    """spiral_cameras of <source_path>/poses_bounds.npy, DTU by the reference's 'scan' in source_path rule."""
    arr = np.load(os.path.join(source_path, "poses_bounds.npy"))
    return spiral_cameras(arr, dtu=is_dtu(source_path), n_frames=n_frames, resolution=resolution, device=device)

