"""Edit a trained model on the device: similarity transforms, crops, merges, registration (csrc/edit.hip, INTEGRATION.md
section 23).

    T = Similarity(R, t, s)                                   # x' = s R x + t, float64 on the host
    D1, D2, D3 = sh_rotation_matrices(R)                      # the rotation of the SH bands 1..3 in preprocess.hip's basis
    model2 = transform(model, T)                              # xyz, quaternions, log scales AND features_rest
    points2 = transform_points(points, T)
    cameras2 = transform_cameras(cameras, T)                  # the same renders, depth scaled by s
    keep, seen = select(model, box=..., sphere=..., min_opacity=..., max_scale=..., cameras=..., masks=..., min_views=1)
    model2 = crop(model, **same)                              # importance.prune(model, keep)
    model3 = merge([a, b])
    T = orient_from_cameras(cameras, unit_radius=False)       # up -> +z, the focus of the optical axes -> origin
    T, history = register(src, dst, max_dist=...)             # trimmed point-to-point ICP, src -> dst

Rotating a Gaussian model means rotating its view-dependent colour: features_rest'[band l] = D_l features_rest[band l] with
Y_l(d)^T D_l = Y_l(R^T d)^T for every unit d.  The device arithmetic (fp64 in one fixed order, one rounding to float32) is
stated in include/b3gs_raster.h and restated in numpy by tests/edit_ref.py: the same bits.

python -m binocular3dgs_amd.edit -m MODEL_PATH [--iteration N] [--pruned]
      [--orient cameras [--unit_radius]] [--matrix FILE.txt] [--rotate AX AY AZ DEG] [--translate X Y Z] [--scale S]
      [--register_to CLOUD.ply --max_dist D [--with_scale]]
      [--box X0 Y0 Z0 X1 Y1 Z1] [--sphere X Y Z R] [--min_opacity A] [--max_scale S] [--masked_views N] [--merge OTHER.ply]
      [--dataset_out DST] [--model_out NEW_MODEL_PATH]

The transform options are applied in the order listed above (each composed on the left of the ones before it), then the crop
(in the new frame), then the merge.  Writes <MODEL_PATH>/point_cloud/iteration_<n>_edited/point_cloud.ply and transform.json
(the 4x4 matrix and s) next to it, and prints one JSON line.  --dataset_out DST also writes the source folder's COLMAP dataset in
the new frame (transform_dataset: the poses of sparse/0/images.bin, the points as sparse/0/points3D.ply, poses_bounds.npy moved,
everything else copied).  The other commands load point_cloud/iteration_<n>/point_cloud.ply of their -m folder, so
--model_out NEW_MODEL_PATH also writes the edited model there under that name, with transform.json and a copy of cfg_args: the
folder to hand to them as -m, with DST as -s.
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)
NEAR = 0.2          # the rasterizer's near cull (csrc/preprocess.hip): what "a view sees the Gaussian" means in select()


# ---- similarities --------------------------------------------------------------------------------------------------------------
class Similarity:
    """x' = s R x + t with s > 0 and R a proper rotation; float64 numpy.  A reflection, a non-uniform scale (from_matrix), a
    non-orthogonal R or a non-finite entry is a ValueError."""

    def __init__(self, R=None, t=None, s: float = 1.0):
        self.R = np.eye(3) if R is None else np.array(R, dtype=np.float64).reshape(3, 3)
        self.t = np.zeros(3) if t is None else np.array(t, dtype=np.float64).reshape(3)
        self.s = float(s)
        if not (np.isfinite(self.R).all() and np.isfinite(self.t).all() and math.isfinite(self.s)):
            raise ValueError("Similarity: a non-finite entry")
        if not self.s > 0.0:
            raise ValueError("Similarity: the scale is positive")
        if np.abs(self.R @ self.R.T - np.eye(3)).max() > 1e-9:
            raise ValueError("Similarity: R is not orthogonal (a non-uniform scale or a shear is not a similarity)")
        if np.linalg.det(self.R) < 0.0:
            raise ValueError("Similarity: R is a reflection")

    def compose(self, other: "Similarity") -> "Similarity":
        """self after other: x -> self(other(x))"""
        return Similarity(self.R @ other.R, self.s * (self.R @ other.t) + self.t, self.s * other.s)

    def inverse(self) -> "Similarity":
        return Similarity(self.R.T, -(self.R.T @ self.t) / self.s, 1.0 / self.s)

    def matrix(self) -> np.ndarray:
        M = np.eye(4)
        M[:3, :3] = self.s * self.R
        M[:3, 3] = self.t
        return M

    @classmethod
    def from_matrix(cls, M4) -> "Similarity":
        M = np.array(M4, dtype=np.float64)
        if M.shape != (4, 4) or not np.isfinite(M).all():
            raise ValueError("Similarity.from_matrix: a finite 4x4 matrix")
        if np.abs(M[3] - np.array([0.0, 0.0, 0.0, 1.0])).max() > 1e-12:
            raise ValueError("Similarity.from_matrix: the last row is (0, 0, 0, 1)")
        A = M[:3, :3]
        det = np.linalg.det(A)
        if det < 0.0:
            raise ValueError("Similarity.from_matrix: a reflection")
        if det == 0.0:
            raise ValueError("Similarity.from_matrix: a singular matrix")
        s = det ** (1.0 / 3.0)
        if np.abs(A @ A.T / (s * s) - np.eye(3)).max() > 1e-9:
            raise ValueError("Similarity.from_matrix: a non-uniform scale or a shear")
        return cls(A / s, M[:3, 3], s)

    def apply(self, x) -> np.ndarray:
        """float64 host points [n,3]"""
        return self.s * (np.asarray(x, dtype=np.float64) @ self.R.T) + self.t

    def quaternion(self) -> np.ndarray:
        """The unit quaternion (w, x, y, z) of R, w >= 0 (Shepperd's choice of the largest pivot)."""
        R = self.R
        tr = R[0, 0] + R[1, 1] + R[2, 2]
        cand = np.array([tr, R[0, 0], R[1, 1], R[2, 2]])
        k = int(np.argmax(cand))
        if k == 0:
            q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        elif k == 1:
            q = np.array([R[2, 1] - R[1, 2], 1.0 + 2.0 * R[0, 0] - tr, R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
        elif k == 2:
            q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + 2.0 * R[1, 1] - tr, R[1, 2] + R[2, 1]])
        else:
            q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + 2.0 * R[2, 2] - tr])
        q = q / np.sqrt((q * q).sum())
        return -q if q[0] < 0.0 else q

    def device_words(self) -> list:
        """The 101 doubles of B3gsSimilarity: R, t, s, ln s, q, D1, D2, D3."""
        D1, D2, D3 = sh_rotation_matrices(self.R)
        return [float(v) for v in np.concatenate([self.R.reshape(-1), self.t, [self.s, math.log(self.s)], self.quaternion(),
                                                  D1.reshape(-1), D2.reshape(-1), D3.reshape(-1)])]

    def __repr__(self):
        return f"Similarity(s={self.s!r}, R={self.R.tolist()!r}, t={self.t.tolist()!r})"


def sh_basis(d: np.ndarray):
    """The real SH of bands 1..3 at unit directions d [n,3] in the basis and signs of csrc/preprocess.hip -> ([n,3], [n,5], [n,7])."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    Y1 = np.stack([-SH_C1 * y, SH_C1 * z, -SH_C1 * x], axis=1)
    Y2 = np.stack([SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)], axis=1)
    Y3 = np.stack([SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
                   SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                   SH_C3[6] * x * (xx - 3.0 * yy)], axis=1)
    return Y1, Y2, Y3


def _fit_directions(n: int = 96) -> np.ndarray:
    """n fixed, well spread unit directions (a Fibonacci lattice): the sample the band matrices are fitted on"""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    r = np.sqrt(1.0 - z * z)
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation_matrices(R):
    """(D1 [3,3], D2 [5,5], D3 [7,7]) float64 with Y_l(d)^T D_l = Y_l(R^T d)^T for every unit d: a model rotated by R, seen along
    d, shows the colour the original showed along R^T d.  Each band is an invariant subspace, so D_l is the exact solution of
    the linear system Y_l(d_i)^T D_l = Y_l(R^T d_i)^T on any set of directions that spans the band: least squares on 96 fixed
    directions (condition number below 2), round-off only."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    d = _fit_directions()
    A, B = sh_basis(d), sh_basis(d @ R)          # (row vectors: d @ R is R^T d)
    return tuple(np.linalg.lstsq(a, b, rcond=None)[0] for a, b in zip(A, B))


# ---- the model, points and cameras under a similarity ---------------------------------------------------------------------------
def _new_model(like, xyz, features_dc, features_rest, scaling, rotation, opacity, sh_degree=None, active=None):
    from torch import nn
    from .gaussian_model import GaussianModel
    m = GaussianModel(like.max_sh_degree if sh_degree is None else sh_degree)
    rg = like._xyz.requires_grad
    for name, t in (("_xyz", xyz), ("_features_dc", features_dc), ("_features_rest", features_rest), ("_scaling", scaling),
                    ("_rotation", rotation), ("_opacity", opacity)):
        setattr(m, name, nn.Parameter(t.contiguous(), requires_grad=rg))
    m.active_sh_degree = like.active_sh_degree if active is None else active
    return m


def _rest_degree(features_rest: torch.Tensor) -> int:
    k = features_rest.shape[1] if features_rest.dim() == 3 else 0
    deg = {0: 0, 3: 1, 8: 2, 15: 3}.get(int(k))
    if deg is None:
        raise ValueError(f"features_rest holds {k} coefficients per channel: SH degrees 0..3 have 0, 3, 8 or 15")
    return deg


def transform(model, T: Similarity):
    """A new GaussianModel in the frame of T: positions, quaternions (q_R (x) q on the raw parameter), log scales (+ ln s) and
    features_rest (every band the tensor holds).  features_dc and opacity are copied.  No optimizer state is carried, as in
    importance.prune.  One launch, no host read."""
    from . import _C
    with torch.no_grad():
        xyz, rot, sc, rest = (p.detach().contiguous() for p in (model._xyz, model._rotation, model._scaling, model._features_rest))
        deg = _rest_degree(rest)
        out = [torch.empty_like(t) for t in (xyz, rot, sc, rest)]
        _C.transform_gaussians(deg, xyz, rot, sc, rest, T.device_words(), *out)
        return _new_model(model, out[0], model._features_dc.detach().clone(), out[3], out[2], out[1], model._opacity.detach().clone())


def transform_points(points: torch.Tensor, T: Similarity, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [N,3] on the device -> s R x + t, fp64 with one rounding.  `out` may be `points`."""
    from . import _C
    points = points.contiguous()
    out = torch.empty_like(points) if out is None else out
    _C.transform_points(points, T.device_words(), out)
    return out


def _camera_pose(cam):
    """(camera-to-world rotation, centre) in float64, with the camera's own trans / scale folded in"""
    R, Tt = np.asarray(cam.R, dtype=np.float64), np.asarray(cam.T, dtype=np.float64)
    C = -R @ Tt
    C = (C + np.asarray(getattr(cam, "trans", np.zeros(3)), dtype=np.float64)) * float(getattr(cam, "scale", 1.0))
    return R, C


def transform_cameras(cameras: Sequence, T: Similarity) -> list:
    """The cameras in the frame of T: world-to-view rotation W' = W R^T, centre C' = s R C + t, znear / zfar scaled by s.
    View coordinates scale by s: the same pixels, depth' = s depth.  Images and masks are shared with the originals."""
    from .camera import Camera, projection_matrix, world_to_view
    out = []
    for cam in cameras:
        Rc, C = _camera_pose(cam)
        R2 = T.R @ Rc
        C2 = T.s * (T.R @ C) + T.t
        c = Camera.__new__(Camera)
        c.__dict__.update({k: v for k, v in cam.__dict__.items() if k not in ("_host", "_b3gs_zkey", "same_depth_as")})
        c.R, c.T = R2, -(R2.T @ C2)
        c.trans, c.scale = np.zeros(3), 1.0
        c.znear, c.zfar = float(cam.znear) * T.s, float(cam.zfar) * T.s
        wvt = torch.tensor(world_to_view(c.R, c.T)).transpose(0, 1)
        c._set(wvt, projection_matrix(c.znear, c.zfar, c.FoVx, c.FoVy).transpose(0, 1))
        out.append(c)
    return out


# ---- selection -----------------------------------------------------------------------------------------------------------------
def _box_words(box) -> list:
    a, b = (np.asarray(v, dtype=np.float64) for v in box)
    if a.shape == (3, 4):
        M, half = a, b.reshape(3)
    else:
        lo, hi = a.reshape(3), b.reshape(3)
        M = np.concatenate([np.eye(3), -(0.5 * (lo + hi)).reshape(3, 1)], axis=1)
        half = 0.5 * (hi - lo)
    if not (np.isfinite(M).all() and np.isfinite(half).all()):
        raise ValueError("select: the box is finite")
    return [float(v) for v in M.reshape(-1)] + [float(v) for v in half]


def camera_words(cameras: Sequence, near: float = NEAR) -> np.ndarray:
    """float64 [V,19]: the conventional 3x4 world-to-view of the matrices the renderer uses, fx fy cx cy W H near"""
    from .camera import fov2focal
    rows = []
    for cam in cameras:
        wvt = cam._host_matrices()["wvt"] if hasattr(cam, "_host_matrices") else cam.world_view_transform.detach().cpu().numpy()
        W2V = np.asarray(wvt, dtype=np.float64).T[:3, :4]
        W, H = int(cam.image_width), int(cam.image_height)
        rows.append(np.concatenate([W2V.reshape(-1), [fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), W / 2.0, H / 2.0, W, H, near]]))
    return np.stack(rows)


def select(model, *, box=None, sphere=None, min_opacity: Optional[float] = None, max_scale: Optional[float] = None, cameras=None,
           masks=None, min_views: int = 1):
    """-> (bool mask [P], seen int32 [P]) on the device; the enabled tests are ANDed, a disabled one costs nothing.
    box:         (lo, hi) corners of an axis-aligned box, or (M [3,4] world-to-box, half [3]): |M (x, 1)| <= half
    sphere:      (centre, radius)
    min_opacity: sigmoid(opacity) >= min_opacity, as the float32 compare opacity_raw >= inverse_sigmoid(min_opacity)
    max_scale:   the largest axis exp(scaling) <= max_scale, as max scaling_raw <= log(max_scale) in float32
    cameras:     up to 64; `seen` counts the views whose frustum (z > 0.2, the pixel inside the image) holds the centre and,
                 with masks (per camera an [H,W] plane, nonzero = object), whose mask is set there; kept when seen >= min_views
    A Gaussian with a non-finite coordinate fails every geometric test.  One launch, no host read."""
    from . import _C
    dev = model._xyz.device
    sph = None
    if sphere is not None:
        c, r = sphere
        sph = [float(v) for v in np.asarray(c, dtype=np.float64).reshape(3)] + [float(r) * float(r)]
    logit = None
    if min_opacity is not None:
        if not 0.0 < min_opacity < 1.0:
            raise ValueError("select: min_opacity lies strictly between 0 and 1")
        logit = math.log(min_opacity / (1.0 - min_opacity))
    lms = None
    if max_scale is not None:
        if not max_scale > 0.0:
            raise ValueError("select: max_scale is positive")
        lms = math.log(max_scale)
    cams = mk = None
    if cameras is not None:
        if not 1 <= len(cameras) <= _C.MAX_SELECT_VIEWS:
            raise ValueError(f"select: 1 .. {_C.MAX_SELECT_VIEWS} cameras per call")
        cams = torch.from_numpy(camera_words(cameras)).to(dev)
        if masks is not None:
            if len(masks) != len(cameras):
                raise ValueError("select: one mask per camera")
            mk = torch.stack([(torch.as_tensor(m).reshape(int(c.image_height), int(c.image_width)) != 0) for m, c in zip(masks, cameras)])
            mk = mk.to(device=dev, dtype=torch.uint8)
    elif masks is not None:
        raise ValueError("select: masks need cameras")
    with torch.no_grad():
        keep, seen = _C.select_gaussians(model._xyz.detach().contiguous(), model._opacity.detach().contiguous(),
                                         model._scaling.detach().contiguous(), None if box is None else _box_words(box), sph, logit, lms,
                                         cams, mk, int(min_views))
    return keep.view(torch.bool), seen


def crop(model, **tests):
    """importance.prune(model, select(model, **tests)[0])"""
    from .importance import prune
    return prune(model, select(model, **tests)[0])


def merge(models: Sequence):
    """The concatenation of the models in order; a lower SH degree is zero-padded to the highest."""
    if not models:
        raise ValueError("merge: no model")
    deg = max(_rest_degree(m._features_rest) for m in models)
    K = (deg + 1) ** 2 - 1
    with torch.no_grad():
        rests = []
        for m in models:
            r = m._features_rest.detach().reshape(m._xyz.shape[0], -1, 3)
            pad = torch.zeros((r.shape[0], K - r.shape[1], 3), dtype=r.dtype, device=r.device)
            rests.append(torch.cat([r, pad], dim=1))
        cat = lambda name: torch.cat([getattr(m, name).detach() for m in models], dim=0)   # noqa: E731
        return _new_model(models[0], cat("_xyz"), cat("_features_dc"), torch.cat(rests, dim=0), cat("_scaling"), cat("_rotation"),
                          cat("_opacity"), sh_degree=max(max(m.max_sh_degree for m in models), deg),
                          active=max(m.active_sh_degree for m in models))


# ---- a frame from the cameras ------------------------------------------------------------------------------------------------------
def orient_from_cameras(cameras: Sequence, unit_radius: bool = False) -> Similarity:
    """Host-only float64.  Up = the normalised mean of the cameras' up vectors (-y of the camera) -> +z; the origin = the
    least-squares point nearest all optical axes; x = the first camera's right vector projected off up; unit_radius scales
    the mean camera distance from the origin to 1.  Raises when the axes do not pin a point (parallel) or up is undefined."""
    poses = [_camera_pose(c) for c in cameras]
    if not poses:
        raise ValueError("orient_from_cameras: no camera")
    up = -np.sum([R[:, 1] for R, _ in poses], axis=0)
    n = np.linalg.norm(up)
    if not n > 1e-9 * len(poses):
        raise ValueError("orient_from_cameras: the cameras' up vectors cancel")
    up = up / n
    A, b = np.zeros((3, 3)), np.zeros(3)
    for R, C in poses:
        d = R[:, 2] / np.linalg.norm(R[:, 2])
        Pm = np.eye(3) - np.outer(d, d)
        A += Pm
        b += Pm @ C
    if np.linalg.cond(A) > 1e12:
        raise ValueError("orient_from_cameras: the optical axes are parallel: no nearest point")
    origin = np.linalg.solve(A, b)
    x = poses[0][0][:, 0] - up * (up @ poses[0][0][:, 0])
    if not np.linalg.norm(x) > 1e-9:
        raise ValueError("orient_from_cameras: the first camera's right vector is along up")
    x = x / np.linalg.norm(x)
    Ro = np.stack([x, np.cross(up, x), up])
    s = 1.0
    if unit_radius:
        mean = float(np.mean([np.linalg.norm(C - origin) for _, C in poses]))
        if not mean > 0.0:
            raise ValueError("orient_from_cameras: every camera sits at the focus")
        s = 1.0 / mean
    return Similarity(Ro, -s * (Ro @ origin), s)


# ---- registration --------------------------------------------------------------------------------------------------------------
def umeyama(sums, origin_a, origin_b, with_scale: bool):
    """Umeyama's closed form (S. Umeyama, "Least-squares estimation of transformation parameters between two point patterns",
    PAMI 1991) from the 18 sums of b3gs_similarity_sums over the pairs (a, b) -> (Similarity a -> b, rms of the residuals of
    the fit)."""
    n = sums[0]
    mu_a, mu_b = sums[1:4] / n, sums[4:7] / n
    var_a = sums[7] / n - (mu_a * mu_a).sum()
    var_b = sums[17] / n - (mu_b * mu_b).sum()
    cov = sums[8:17].reshape(3, 3) / n - np.outer(mu_b, mu_a)
    U, D, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0.0:
        S[2] = -1.0
    R = (U * S) @ Vt
    tr = float((D * S).sum())
    if with_scale and not var_a > 0.0:
        raise ValueError("register: the matched source points coincide: no scale")
    c = tr / var_a if with_scale else 1.0
    t = (mu_b + origin_b) - c * (R @ (mu_a + origin_a))
    err = var_b - 2.0 * c * tr + c * c * var_a
    return Similarity(R, t, c), math.sqrt(max(err, 0.0))


def _bbox_centre(p: torch.Tensor) -> np.ndarray:
    lo_hi = torch.stack([p.amin(dim=0), p.amax(dim=0)]).cpu().numpy().astype(np.float64)
    return 0.5 * (lo_hi[0] + lo_hi[1])


def register(src: torch.Tensor, dst: torch.Tensor, *, max_dist: float, init: Optional[Similarity] = None, iterations: int = 30,
             with_scale: bool = False, tol: float = 1e-10):
    """Trimmed point-to-point ICP of src onto dst (float32 [N,3] / [M,3] on the device) -> (Similarity, history).
    Per iteration: transform_points(src, T) -> the nearest point of dst within max_dist (b3gs_nearest_query_index over a grid
    built once) -> the sums of the pairs (src_i, dst_j) (b3gs_similarity_sums: the 17 of the fit and sum |b~|^2, which the
    residual needs) -> ONE host read of 18 doubles -> Umeyama's closed form in numpy float64 gives
    the next T outright (nothing is composed, so nothing drifts).  history holds (pairs, rms of the fit's residuals) per
    iteration; the loop stops when neither changes by more than tol, relative.  Fewer than 3 pairs is a ValueError."""
    from . import _C
    from .mesh_tools import NearestGrid
    if src.dim() != 2 or src.shape[1] != 3 or dst.dim() != 2 or dst.shape[1] != 3 or src.shape[0] < 3 or dst.shape[0] < 3:
        raise ValueError("register: src and dst are [n,3] with at least 3 points each")
    src, dst = src.contiguous(), dst.contiguous()
    T = Similarity() if init is None else init
    grid = NearestGrid(dst, max_dist)
    oa, ob = _bbox_centre(src), _bbox_centre(dst)           # (min / max: the same value whatever the order of the reduction)
    la, lb = [float(v) for v in oa], [float(v) for v in ob]
    out = torch.empty(18, dtype=torch.float64, device=src.device)
    cur = torch.empty_like(src)
    history = []
    for _ in range(int(iterations)):
        transform_points(src, T, cur)
        dist, index = grid.query_index(cur)
        _C.similarity_sums(src, dst, index, dist, float(max_dist), None, la, lb, out)
        sums = out.cpu().numpy()                              # the one host read
        n = int(sums[0])
        if n < 3:
            raise ValueError(f"register: {n} pairs within max_dist = {max_dist}: fewer than 3")
        T, rms = umeyama(sums, oa, ob, with_scale)
        history.append((n, rms))
        if len(history) > 1:
            n0, r0 = history[-2]
            if abs(n - n0) <= tol * n0 and abs(rms - r0) <= tol * max(r0, 1e-300):
                break
    return T, history


# ---- the dataset folder under a similarity ------------------------------------------------------------------------------------
STALE = ("points3D.bin", "points3D.txt", "points3D.ply", "images.bin", "images.txt", "cameras.bin", "cameras.txt")


def transform_pose(qvec, tvec, T: Similarity):
    """COLMAP's world-to-camera pose (x_cam = R(q) x + t) in the frame of T: R' = R(q) R_T^T, C' = s R_T C + t_T, t' = -R' C', so
    that x_cam' = s x_cam for x' = T(x) -- transform_cameras' rule.  -> (qvec' with w >= 0, tvec')"""
    from .dataset_readers import quaternion_to_rotation
    q = np.asarray(qvec, dtype=np.float64)
    Rw = quaternion_to_rotation(q / np.linalg.norm(q))
    C = -Rw.T @ np.asarray(tvec, dtype=np.float64)
    R2 = Rw @ T.R.T
    return Similarity(R2).quaternion(), -R2 @ (T.s * (T.R @ C) + T.t)


def transform_poses_bounds(poses_bounds, T: Similarity) -> np.ndarray:
    """The [N, 17] rows of an LLFF / DTU poses_bounds.npy in the frame of T.  Each row is a 3x5 block [camera-to-world axes |
    centre | hwf] and the near / far bounds.  The three axis columns are directions in the world, so each becomes R_T d whatever
    the order LLFF keeps them in (the fixed reordering of camera_path acts on the right, R_T on the left); the centre becomes
    s R_T C + t_T, both bounds are multiplied by s, the hwf column stays.  float64."""
    a = np.array(poses_bounds, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 17 or a.shape[0] < 1 or not np.isfinite(a).all():
        raise ValueError("not a finite [N, 17] array of poses and bounds")
    blocks = a[:, :15].reshape(-1, 3, 5).copy()
    blocks[:, :, :3] = T.R @ blocks[:, :, :3]
    blocks[:, :, 3] = T.s * (blocks[:, :, 3] @ T.R.T) + T.t
    a[:, :15] = blocks.reshape(-1, 15)
    a[:, 15:] *= T.s
    return a


def transform_dataset(src: str, dst: str, T: Similarity) -> dict:
    """Writes the COLMAP dataset folder `src` under T as `dst`: sparse/0/images.bin with the moved poses (ids, names, camera ids
    and 2-D points kept), sparse/0/cameras.bin as read, the 3-D points moved in float64 as sparse/0/points3D.ply (the file the
    reader prefers; the unmoved points3D.bin / .txt are NOT copied), poses_bounds.npy -- the file camera_path (spiral) takes its
    poses and depth bounds from -- moved by transform_poses_bounds, every other file of sparse/0, every other top-level file and
    every other folder (the images, the masks) copied.  Refused by name, before anything is written: a Blender folder
    (transforms_train.json: its reader takes the poses from the json files, which are not rewritten), a folder without sparse/0,
    a poses_bounds.npy that is no finite [N, 17] array, and a `dst` that is `src` or lies inside it.  spiral takes a folder for
    DTU when its path contains 'scan': keep that in the name of `dst`.  A matcher cloud or match files computed in the old frame
    are not part of the folder: compute them again, or train with --init_points sparse.  Host only."""
    import shutil
    from . import dataset_readers as dr
    from .init_points import fetch_point_cloud
    from .undistort import _read_sparse, write_cameras_bin, write_images_bin
    a, b = os.path.realpath(src), os.path.realpath(dst)
    if a == b:
        raise ValueError("the output folder must not be the source folder")
    if os.path.commonpath([a, b]) == a:
        raise ValueError(f"the output folder {dst} lies inside the source folder {src}: it would be copied into itself")
    if os.path.exists(os.path.join(src, "transforms_train.json")):
        raise ValueError(f"{src}: a Blender dataset (transforms_train.json): its reader takes the poses from the transforms_*.json "
                         "files, not from sparse/0 -- not rewritten")
    sparse = os.path.join(src, "sparse/0")
    if not os.path.isdir(sparse):
        raise ValueError(f"{src}: no sparse/0: only COLMAP dataset folders are rewritten"
                         + (" (the readers take the training poses from sparse/0, never from poses_bounds.npy alone)"
                            if os.path.exists(os.path.join(src, "poses_bounds.npy")) else ""))
    bounds = None
    if os.path.exists(os.path.join(src, "poses_bounds.npy")):
        try:
            bounds = transform_poses_bounds(np.load(os.path.join(src, "poses_bounds.npy")), T)
        except ValueError as e:
            raise ValueError(f"{src}/poses_bounds.npy: {e}") from None
    extr, intr = _read_sparse(sparse)
    xyz = rgb = None
    for name, reader in (("points3D.ply", fetch_point_cloud), ("points3D.bin", dr.read_points3d_bin), ("points3D.txt", dr.read_points3d_txt)):
        if os.path.exists(os.path.join(sparse, name)):
            xyz, rgb = reader(os.path.join(sparse, name))
            if name == "points3D.ply":
                rgb = np.asarray(rgb, dtype=np.float64) * 255.0
            break
    moved = {}
    for iid, rec in extr.items():
        q, t = transform_pose(rec[0], rec[1], T)
        moved[iid] = (q, t) + tuple(rec[2:])
    os.makedirs(os.path.join(dst, "sparse/0"), exist_ok=True)
    write_cameras_bin(os.path.join(dst, "sparse/0/cameras.bin"), intr)
    write_images_bin(os.path.join(dst, "sparse/0/images.bin"), moved)
    if xyz is not None:
        dr.write_point_ply(os.path.join(dst, "sparse/0/points3D.ply"), T.apply(xyz), np.clip(np.rint(rgb), 0, 255))
    for f in sorted(os.listdir(sparse)):
        if f not in STALE and os.path.isfile(os.path.join(sparse, f)):
            shutil.copyfile(os.path.join(sparse, f), os.path.join(dst, "sparse/0", f))
    for f in sorted(os.listdir(src)):
        a, b = os.path.join(src, f), os.path.join(dst, f)
        if f == "poses_bounds.npy":
            np.save(b, bounds)
        elif os.path.isfile(a):
            shutil.copyfile(a, b)
        elif os.path.isdir(a) and f != "sparse":
            shutil.copytree(a, b, dirs_exist_ok=True)
    return {"dataset": os.path.abspath(dst), "images": len(moved), "points": 0 if xyz is None else int(len(xyz)),
            "poses_bounds": 0 if bounds is None else int(len(bounds))}


def _ply_sh_degree(path: str) -> int:
    """the SH degree a model PLY holds, from the number of its f_rest_* properties"""
    from .init_points import read_ply_vertices
    n = sum(1 for name in read_ply_vertices(path).dtype.names if name.startswith("f_rest_"))
    deg = {0: 0, 9: 1, 24: 2, 45: 3}.get(n)
    if deg is None:
        raise ValueError(f"{path}: {n} f_rest_* properties: SH degrees 0..3 have 0, 9, 24 or 45")
    return deg


# ---- the command line ----------------------------------------------------------------------------------------------------------
def _rotation_about(axis, deg: float) -> np.ndarray:
    a = np.asarray(axis, dtype=np.float64)
    n = np.linalg.norm(a)
    if not n > 0.0:
        raise ValueError("--rotate: the axis is not zero")
    a = a / n
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = math.radians(deg)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def _scene_cameras(cfg, source_path):
    from .scene import Scene
    scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=True, n_views=int(cfg.get("n_views", 3)),
                               dataset_name=cfg.get("dataset_name", "LLFF"), suffix=cfg.get("suffix"),
                               resolution=cfg.get("resolution", -1), white_background=bool(cfg.get("white_background", False)),
                               init_points=cfg.get("init_points", "matcher"), shuffle=False)
    return list(scene.getTrainCameras())


def run(model_path: str, source_path: Optional[str] = None, iteration: int = -1, pruned: bool = False, orient: Optional[str] = None,
        unit_radius: bool = False, matrix: Optional[str] = None, rotate=None, translate=None, scale: Optional[float] = None,
        register_to: Optional[str] = None, max_dist: Optional[float] = None, with_scale: bool = False, box=None, sphere=None,
        min_opacity: Optional[float] = None, max_scale: Optional[float] = None, masked_views: Optional[int] = None,
        merge_with: Optional[str] = None, dataset_out: Optional[str] = None, model_out: Optional[str] = None) -> dict:
    from .gaussian_model import GaussianModel
    from .init_points import load_ply
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    sh = int(cfg.get("sh_degree", 1))
    model = GaussianModel(sh)
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it) + ("_pruned" if pruned else ""), "point_cloud.ply"))
    cams = None
    if orient or masked_views is not None or dataset_out:
        source_path = source_path or cfg.get("source_path")
        if not source_path:
            raise ValueError("no source path: pass -s or keep cfg_args next to the model")
    if orient or masked_views is not None:
        cams = _scene_cameras(cfg, source_path)
    T = Similarity()
    if orient:
        T = orient_from_cameras(cams, unit_radius).compose(T)
    if matrix:
        T = Similarity.from_matrix(np.loadtxt(matrix)).compose(T)
    if rotate is not None:
        T = Similarity(_rotation_about(rotate[:3], rotate[3])).compose(T)
    if translate is not None:
        T = Similarity(t=translate).compose(T)
    if scale is not None:
        T = Similarity(s=scale).compose(T)
    res = {"P_before": int(model._xyz.shape[0]), "iteration": it}
    if register_to:
        from .init_points import read_ply_vertices
        if max_dist is None:
            raise ValueError("--register_to needs --max_dist")
        rows = read_ply_vertices(register_to)
        gt = torch.from_numpy(np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)).cuda()
        moved = transform_points(model._xyz.detach(), T)
        Tr, hist = register(moved, gt, max_dist=max_dist, with_scale=with_scale)
        T = Tr.compose(T)
        res["register"] = {"iterations": len(hist), "pairs": hist[-1][0], "rms": hist[-1][1]}
    edited = transform(model, T)
    tests = {}
    if box is not None:
        tests["box"] = (box[:3], box[3:])
    if sphere is not None:
        tests["sphere"] = (sphere[:3], sphere[3])
    if min_opacity is not None:
        tests["min_opacity"] = min_opacity
    if max_scale is not None:
        tests["max_scale"] = max_scale
    if masked_views is not None:
        moved_cams = transform_cameras(cams, T)
        if len(moved_cams) > 64:
            raise ValueError(f"--masked_views: {len(moved_cams)} cameras, at most 64")
        masks = [getattr(c, "gt_alpha_mask", None) for c in moved_cams]
        tests.update(cameras=moved_cams, masks=None if any(m is None for m in masks) else masks, min_views=masked_views)
    if tests:
        edited = crop(edited, **tests)
    if merge_with:
        edited = merge([edited, load_ply(merge_with, _ply_sh_degree(merge_with))])
    out_dir = os.path.join(model_path, "point_cloud", "iteration_" + str(it) + "_edited")
    os.makedirs(out_dir, exist_ok=True)
    edited.save_ply(os.path.join(out_dir, "point_cloud.ply"))
    with open(os.path.join(out_dir, "transform.json"), "w") as fp:
        json.dump({"matrix": T.matrix().tolist(), "s": T.s}, fp)
    res.update({"P_after": int(edited._xyz.shape[0]), "s": T.s, "matrix": T.matrix().tolist(),
                "ply": os.path.join(out_dir, "point_cloud.ply")})
    if dataset_out:
        res.update(transform_dataset(source_path, dataset_out, T))
    if model_out:
        import shutil
        new_dir = os.path.join(model_out, "point_cloud", "iteration_" + str(it))
        os.makedirs(new_dir, exist_ok=True)
        for f in ("point_cloud.ply", "transform.json"):
            shutil.copyfile(os.path.join(out_dir, f), os.path.join(new_dir, f))
        if os.path.exists(os.path.join(model_path, "cfg_args")):
            shutil.copyfile(os.path.join(model_path, "cfg_args"), os.path.join(model_out, "cfg_args"))
        res["model"] = os.path.abspath(model_out)
    print(json.dumps(res))
    return res


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.edit", description=__doc__.split("\n")[0])
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--pruned", action="store_true", help="start from iteration_<n>_pruned")
    p.add_argument("--orient", choices=("cameras",), default=None)
    p.add_argument("--unit_radius", action="store_true")
    p.add_argument("--matrix", default=None, metavar="FILE.txt", help="a 4x4 similarity matrix")
    p.add_argument("--rotate", type=float, nargs=4, default=None, metavar=("AX", "AY", "AZ", "DEG"))
    p.add_argument("--translate", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    p.add_argument("--scale", type=float, default=None)
    p.add_argument("--register_to", default=None, metavar="CLOUD.ply")
    p.add_argument("--max_dist", type=float, default=None)
    p.add_argument("--with_scale", action="store_true")
    p.add_argument("--box", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    p.add_argument("--sphere", type=float, nargs=4, default=None, metavar=("X", "Y", "Z", "R"))
    p.add_argument("--min_opacity", type=float, default=None)
    p.add_argument("--max_scale", type=float, default=None)
    p.add_argument("--masked_views", type=int, default=None, metavar="N", help="keep what at least N training views see (inside their masks)")
    p.add_argument("--merge", default=None, metavar="OTHER.ply")
    p.add_argument("--dataset_out", default=None, metavar="DST", help="also write the source dataset folder in the new frame")
    p.add_argument("--model_out", default=None, metavar="NEW_MODEL_PATH",
                   help="also write the edited model as NEW_MODEL_PATH/point_cloud/iteration_<n>, with cfg_args: a -m folder for the other commands")
    a = p.parse_args(argv)
    run(a.model_path, a.source_path, a.iteration, a.pruned, a.orient, a.unit_radius, a.matrix, a.rotate, a.translate, a.scale,
        a.register_to, a.max_dist, a.with_scale, a.box, a.sphere, a.min_opacity, a.max_scale, a.masked_views, a.merge, a.dataset_out,
        a.model_out)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
