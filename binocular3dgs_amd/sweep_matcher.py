"""The plane-sweep stereo matcher: keypoint matches of calibrated views WITHOUT a matcher network.

This is NOT the reference's matcher (PDC-Net+, a network with downloaded weights): it is an additional, classical source of
the `kp_<ref>_<src>_source` / `_target` arrays matcher_cloud.load_matches reads.  With the poses of <source>/sparse/0 known,
two-view matching is a search along the epipolar line: per node (every `stride`-th pixel) of a view the best of `hypotheses`
fronto-parallel inverse-depth planes by the zero-mean normalised cross-correlation of 7x7 gray patches, a uniqueness test, a
parabola refinement and a left/right consistency check.  The kernels are csrc/sweep.hip behind `_C.sweep_match_pair`; there is
no CPU path.

    depth_range     (near, far) from the COLMAP points of the folder
    pair_plan       host, float64 -> float32: the homographies of both directions of a view pair
    match_pair      both directions of one pair, one count read
    match_views     every pair of the selected views of a dataset folder -> the matches mapping
    write_matches   the .npz matcher_cloud.load_matches reads back unchanged

The uniqueness test compares the best hypothesis with those two or more steps away, so hypotheses much finer than about half a
pixel of disparity reject everything: choose `hypotheses` (and near / far) so that a step is about half a pixel to a pixel.
"""
from __future__ import annotations

import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dataset_readers as dr
from . import matcher_cloud as mc

RADIUS = 3


class SweepParams(NamedTuple):
    stride: int = 2
    hypotheses: int = 128
    min_score: float = 0.8
    margin: float = 0.05
    min_var: float = 4.0           # gray levels^2
    cyc_steps: float = 1.5
    near: Optional[float] = None   # None: depth_range()
    far: Optional[float] = None


class PairPlan(NamedTuple):
    homographies: np.ndarray       # float32 [2, D, 3, 3]
    proj: np.ndarray               # float32 [2, 12]
    inv_far: float
    step: float


def node_count(W: int, H: int, stride: int) -> int:
    return ((W - 2 * RADIUS - 1) // stride + 1) * ((H - 2 * RADIUS - 1) // stride + 1)


def _read_points(source_path: str) -> np.ndarray:
    sparse = os.path.join(source_path, "sparse/0")
    for name, reader in (("points3D.bin", dr.read_points3d_bin), ("points3D.txt", dr.read_points3d_txt)):
        path = os.path.join(sparse, name)
        if os.path.exists(path):
            return reader(path)[0]
    return np.zeros((0, 3))


def depth_range(source_path: str, views: mc.DatasetViews, ref_indices: Sequence[int]) -> Tuple[float, float]:
    """0.8 x the 1st and 1.2 x the 99th percentile of the depths of the COLMAP points in the selected views"""
    xyz = _read_points(source_path)
    depths = []
    for i in ref_indices:
        w2c = np.linalg.inv(views.c2ws[i].astype(np.float64))
        z = xyz @ w2c[2, :3] + w2c[2, 3]
        depths.append(z[z > 0])
    depths = np.concatenate(depths) if depths else np.zeros(0)
    if len(depths) == 0:
        raise ValueError(f"{source_path}/sparse/0 holds no points in front of the selected views: give the depth range with --near/--far")
    return 0.8 * float(np.percentile(depths, 1)), 1.2 * float(np.percentile(depths, 99))


def _direction(K: np.ndarray, w2c_a: np.ndarray, w2c_b: np.ndarray, inv_far: float, step: float, D: int):
    rel = w2c_b @ np.linalg.inv(w2c_a)
    Rm, t = rel[:3, :3], rel[:3, 3]
    Kinv = np.linalg.inv(K)
    n = np.array([0.0, 0.0, 1.0])
    hs = np.stack([K @ (Rm + np.outer(t, n) * (inv_far + step * k)) @ Kinv for k in range(D)])
    return hs, np.concatenate([(K @ Rm @ Kinv).ravel(), K @ t])


def pair_plan(intrinsic, c2w_a, c2w_b, near: float, far: float, hypotheses: int) -> PairPlan:
    """H_k = K (R + t n^T invd[k]) K^-1 with n = (0, 0, 1) and invd[k] = 1 / far + (1 / near - 1 / far) k / (D - 1), for a -> b
    and for b -> a, built in float64 and handed over as float32"""
    if not (0 < near < far):
        raise ValueError(f"the depth range needs 0 < near < far, not {near} .. {far}")
    if hypotheses < 2:
        raise ValueError("at least 2 hypotheses")
    K = np.asarray(intrinsic, np.float64)
    wa, wb = np.linalg.inv(np.asarray(c2w_a, np.float64)), np.linalg.inv(np.asarray(c2w_b, np.float64))
    inv_far, step = 1.0 / far, (1.0 / near - 1.0 / far) / (hypotheses - 1)
    hab, pab = _direction(K, wa, wb, inv_far, step, hypotheses)
    hba, pba = _direction(K, wb, wa, inv_far, step, hypotheses)
    return PairPlan(np.stack([hab, hba]).astype(np.float32), np.stack([pab, pba]).astype(np.float32), float(np.float32(inv_far)),
                    float(np.float32(step)))


def launch_pair(image_a: torch.Tensor, image_b: torch.Tensor, homographies: torch.Tensor, proj: torch.Tensor, plan: PairPlan, near: float,
                far: float, params: SweepParams):
    """The launch assembly alone, device tensors in and out, nothing read: what a graph captures.  -> the tuple of
    _C.sweep_match_pair"""
    from . import _C
    return _C.sweep_match_pair(image_a, image_b, homographies, proj, float(near), float(far), plan.inv_far, plan.step, int(params.stride),
                               RADIUS, float(params.min_score), float(params.margin), float(params.min_var), float(params.cyc_steps))


def match_pair(image_a, image_b, intrinsic, c2w_a, c2w_b, near: float, far: float, params: SweepParams = SweepParams()):
    """-> ((kp_a, kp_ab, score), (kp_b, kp_ba, score)): float32 [n,2], [n,2], [n] device tensors of the matches a -> b and
    b -> a in node order, sliced by the two counts (ONE read of the device per call)"""
    img_a = image_a if isinstance(image_a, torch.Tensor) else mc._dev_image(image_a, "cuda")
    dev = img_a.device
    img_b = image_b if isinstance(image_b, torch.Tensor) else mc._dev_image(image_b, dev)
    plan = pair_plan(intrinsic, c2w_a, c2w_b, near, far, int(params.hypotheses))
    hs, pj = (torch.from_numpy(plan.homographies).to(dev), torch.from_numpy(plan.proj).to(dev)) if dev.type == "cuda" else (
        torch.from_numpy(plan.homographies), torch.from_numpy(plan.proj))
    src, dst, score, count = launch_pair(mc._dev_image(img_a, dev), mc._dev_image(img_b, dev), hs, pj, plan, near, far, params)[:4]
    na, nb = (int(v) for v in count.tolist())
    return (src[0, :na], dst[0, :na], score[0, :na]), (src[1, :nb], dst[1, :nb], score[1, :nb])


def match_images(views: mc.DatasetViews, images, ref_indices: Sequence[int], near: float, far: float,
                 params: SweepParams = SweepParams()) -> Dict[str, np.ndarray]:
    """the matches mapping of the selected views, from images that are already on the device"""
    out: Dict[str, np.ndarray] = {}
    plan = mc.plan_pairs(views, ref_indices)
    done = {}
    for r, s, ref_cam, src_cam in plan:
        if (s, r) in done:
            fwd = done[(s, r)][1]
        else:
            done[(r, s)] = match_pair(images[r], images[s], ref_cam.intrinsic, ref_cam.c2w, src_cam.c2w, near, far, params)
            fwd = done[(r, s)][0]
        a, b = mc.match_keys(views.names[r], views.names[s])
        out[a], out[b] = fwd[0].cpu().numpy().reshape(-1, 2), fwd[1].cpu().numpy().reshape(-1, 2)
    return out


def resolve_range(source_path: str, views: mc.DatasetViews, ref_indices: Sequence[int], params: SweepParams) -> Tuple[float, float]:
    if params.near is not None and params.far is not None:
        return float(params.near), float(params.far)
    near, far = depth_range(source_path, views, ref_indices)
    return (float(params.near) if params.near is not None else near), (float(params.far) if params.far is not None else far)


def match_views(source_path: str, *, dataset_name: str = "LLFF", n_views: int = 3, resolution: int = 4,
                dtu_sparse_indices: Sequence[int] = mc.DTU_SPARSE_INDICES, params: SweepParams = SweepParams(),
                device="cuda") -> Dict[str, np.ndarray]:
    """{kp_<ref>_<src>_source / _target: float32 [N,2]} for every ordered pair of the selected views (the keys of
    matcher_cloud.match_keys); a pair without surviving matches yields [0,2] arrays"""
    views = mc.read_views(source_path, resolution)
    ref_indices = mc.select_views(len(views.names), dataset_name, n_views, dtu_sparse_indices)
    near, far = resolve_range(source_path, views, ref_indices, params)
    images = mc.load_images(views, resolution, device)
    return match_images(views, images, ref_indices, near, far, params)


def write_matches(path: str, matches: Dict[str, np.ndarray]) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fp:                                   # (a file object: numpy appends no suffix of its own)
        np.savez(fp, **{k: np.asarray(v, np.float32).reshape(-1, 2) for k, v in matches.items()})
