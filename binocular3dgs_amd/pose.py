"""Camera pose gradients and photometric pose refinement from the per-Gaussian backward (csrc/pose.hip, INTEGRATION.md
section 24).

    g = camera_gradient(model, cam, pipe, bg, loss_fn)        # device double[6]: dL/d(omega, t) of the CAMERA
    cam2, history = refine_pose(model, cam, image)            # Adam on the 6-vector, coarse to fine
    cams2, twists = refine_poses(model, cameras)              # each camera against its own original_image
    cam2 = moved_camera(cam, xi, pivot)
    T = se3_exp(xi); xi = se3_log(T)
    G1, G2, G3 = sh_generators()

Rendering a scene from a moved camera is rendering the inversely moved scene from the fixed camera.  A rigid motion of the
scene moves the means, multiplies the quaternions on the left and rotates the SH bands (edit.transform), so dL/d(pose) is a
LINEAR reduction of dL/dxyz, dL/drotation and dL/dfeatures_rest, which the backward produces anyway: no second
differentiable rasterizer.  b3gs_pose_gradient does the reduction for up to 8 views in one launch, fp64, the same bits on
every call (include/b3gs_raster.h states the arithmetic, tests/pose_ref.py restates it in numpy).

Conventions.  A twist xi = (omega, t) is a 6-vector in the WORLD frame about a pivot c: the motion is
x -> c + exp(omega) (x - c) + V(omega) t = Tr(c) se3_exp(xi) Tr(-c).  The kernel returns the gradient for a twist of the
SCENE; a camera moved by M sees what the fixed camera sees of the scene moved by M^-1, so the CAMERA's gradient is the
negative: pose_gradient() returns that.  moved_camera applies the motion on the left of the camera-to-world pose.

python -m binocular3dgs_amd.localize and evaluate --align_poses are the commands on top of refine_pose.
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Sequence

import numpy as np
import torch

R3, R6, R6H, R10H = 1.7320508075688772, 2.4494897427831779, 1.2247448713915890, 1.5811388300841898
# G_l^k[j][m] for j < m (antisymmetric): (axis, j, m, value), derived in csrc/pose.hip's header
_GEN = {1: ((0, 0, 1, 1.0), (1, 1, 2, 1.0), (2, 0, 2, 1.0)),
        2: ((0, 0, 3, 1.0), (0, 1, 2, R3), (0, 1, 4, 1.0), (1, 0, 1, -1.0), (1, 2, 3, R3), (1, 3, 4, 1.0), (2, 0, 4, 2.0), (2, 1, 3, 1.0)),
        3: ((0, 0, 5, R6H), (0, 1, 4, R10H), (0, 1, 6, R6H), (0, 2, 3, R6), (0, 2, 5, R10H), (1, 0, 1, -R6H), (1, 1, 2, -R10H),
            (1, 3, 4, R6), (1, 4, 5, R10H), (1, 5, 6, R6H), (2, 0, 6, 3.0), (2, 1, 5, 2.0), (2, 2, 4, 1.0))}

# refine_pose's step sizes: radians, and fractions of the camera-to-pivot distance, per Adam step; chosen on the synthetic
# scene of tests/test_gpu_pose.py
LR_ROT, LR_TRANS, LR_FINAL = 4e-3, 2e-3, 0.1


# ---- SE(3) ---------------------------------------------------------------------------------------------------------------------
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(th: float):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3.  Below 1e-2 by their series to th^6 (the next terms are below
    1e-20); above, (1 - cos th) as 2 sin^2(th / 2): nothing cancels."""
    if th < 1e-2:
        t2 = th * th
        return (1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0)), 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0)),
                1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
    h = math.sin(0.5 * th)
    return math.sin(th) / th, 2.0 * h * h / (th * th), (th - math.sin(th)) / (th * th * th)


def se3_exp(xi) -> np.ndarray:
    """xi = (omega, t) float64 [6] -> the 4x4 matrix [[exp(omega), V t], [0, 1]], V = I + B K + C K^2 (closed form)"""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, t = xi[:3], xi[3:]
    A, B, C = _abc(float(np.linalg.norm(w)))
    K = _hat(w)
    K2 = K @ K
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * K2
    T[:3, 3] = (np.eye(3) + B * K + C * K2) @ t
    return T


def se3_log(T) -> np.ndarray:
    """The inverse of se3_exp for a rigid 4x4 matrix with a rotation angle below pi -> float64 [6]"""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    R = T[:3, :3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin(th) * axis
    s, c = float(np.linalg.norm(v)), 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    th = math.atan2(s, c)
    if th < 1e-4:
        w = v * (1.0 + th * th / 6.0)
    elif s > 1e-6:
        w = v * (th / s)
    else:                                           # next to pi: the axis from the diagonal of (R + I) / 2, signs from v
        a = np.sqrt(np.maximum(0.5 * (np.diag(R) + 1.0), 0.0))
        k = int(np.argmax(a))
        a = np.array([(0.25 * (R[k, j] + R[j, k]) / a[k]) if j != k else a[k] for j in range(3)])
        if float(a @ v) < 0.0:
            a = -a
        w = a / np.linalg.norm(a) * th
    A, B, _ = _abc(th)
    t2 = th * th                                    # (1 - A / 2B) / th^2: by its series below 0.05 (the next term is below 1e-18)
    D = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0 + t2 * t2 * t2 / 1209600.0 if th < 0.05 else (1.0 - A / (2.0 * B)) / t2
    K = _hat(w)
    return np.concatenate([w, (np.eye(3) - 0.5 * K + D * (K @ K)) @ T[:3, 3]])


def twist_matrix(xi, pivot) -> np.ndarray:
    """Tr(c) se3_exp(xi) Tr(-c): the 4x4 world motion of the twist xi about the pivot c"""
    c = np.asarray(pivot, dtype=np.float64).reshape(3)
    M = se3_exp(xi)
    M[:3, 3] = (c - M[:3, :3] @ c) + M[:3, 3]
    return M


def sh_generators():
    """(G1 [3,3,3], G2 [3,5,5], G3 [3,7,7]) float64: G_l[k] = d/dtheta D_l(exp(theta e_k)) at theta = 0 with D_l =
    edit.sh_rotation_matrices' band matrices -- the constants of csrc/pose.hip (antisymmetric; [G^x, G^y] = G^z and cyclic)."""
    out = []
    for band in (1, 2, 3):
        n = 2 * band + 1
        G = np.zeros((3, n, n))
        for k, j, m, a in _GEN[band]:
            G[k, j, m], G[k, m, j] = a, -a
        out.append(G)
    return tuple(out)


# ---- the reduction -------------------------------------------------------------------------------------------------------------
def pose_gradient(model, grads: Sequence, *, pivot, skip: Optional[Sequence] = None) -> torch.Tensor:
    """device float64 [V,6]: per view the gradient (d/domega [3], d/dt [3]) of its loss with respect to a twist of the CAMERA.
    grads: up to 8 triples (g_xyz [P,3], g_rotation [P,4], g_features_rest [P,K,3]) -- the gradients of that view's loss with
    respect to model._xyz, model._rotation (raw) and model._features_rest; a None g_features_rest counts as zeros.
    skip: per view None or a bool / uint8 [P]; rows with a non-zero entry are left out unread (e.g. radii == 0).

    Conventions: the twist is in the WORLD frame about `pivot` (x -> pivot + exp(omega) (x - pivot) + t to first order), and
    the camera's gradient is MINUS the scene's, which is what b3gs_pose_gradient sums: moving the camera by M shows the scene
    moved by M^-1.  So a descent step on the camera is moved_camera(cam, -lr * g, pivot).  One launch, no host read."""
    from . import _C
    from .edit import _rest_degree
    if not 1 <= len(grads) <= _C.MAX_POSE_VIEWS:
        raise ValueError(f"pose_gradient: 1 .. {_C.MAX_POSE_VIEWS} views per call")
    if skip is not None and len(skip) != len(grads):
        raise ValueError("pose_gradient: one skip entry per view")
    xyz, rot, rest = (p.detach().contiguous() for p in (model._xyz, model._rotation, model._features_rest))
    deg = _rest_degree(rest)
    if deg > 0 and all(g[2] is None for g in grads):
        deg = 0                      # no view-dependent colour took part in any loss: the term is zero
    gx = [g[0].detach().contiguous() for g in grads]
    gr = [g[1].detach().contiguous() for g in grads]
    gf = [] if deg == 0 else [(torch.zeros_like(rest) if g[2] is None else g[2].detach().contiguous()) for g in grads]
    sk = None if skip is None else [None if s is None else s.contiguous() for s in skip]
    out = torch.empty((len(grads), 6), dtype=torch.float64, device=xyz.device)
    _C.pose_gradient(deg, xyz, rot, rest, gx, gr, gf, sk, [float(v) for v in np.asarray(pivot, dtype=np.float64).reshape(3)], out)
    return out.neg_()


# ---- cameras -------------------------------------------------------------------------------------------------------------------
def moved_camera(cam, xi, pivot):
    """`cam` with its camera-to-world pose multiplied on the left by the twist xi about `pivot`: R' = exp(omega) R,
    C' = c + exp(omega) (C - c) + V t.  Built as edit.transform_cameras builds cameras (the same constructor path, so xi = 0
    returns the camera's own matrices bit for bit); images and masks are shared with `cam`."""
    from .camera import Camera, projection_matrix, world_to_view
    from .edit import _camera_pose
    c = np.asarray(pivot, dtype=np.float64).reshape(3)
    M = se3_exp(xi)
    Rm, tm = M[:3, :3], M[:3, 3]
    Rc, C = _camera_pose(cam)
    plain = not np.any(np.asarray(getattr(cam, "trans", np.zeros(3)))) and float(getattr(cam, "scale", 1.0)) == 1.0
    T0 = np.asarray(cam.T, dtype=np.float64) if plain else -(Rc.T @ C)
    R2 = Rm @ Rc
    out = Camera.__new__(Camera)
    out.__dict__.update({k: v for k, v in cam.__dict__.items() if k not in ("_host", "_b3gs_zkey", "same_depth_as")})
    # x_cam = R2^T (x - C') with C' = c + Rm (C - c) + tm:  T' = (Rc^T c - R2^T (c + tm)) + T  (exactly T at xi = 0)
    out.R, out.T = R2, (Rc.T @ c - R2.T @ (c + tm)) + T0
    out.trans, out.scale = np.zeros(3), 1.0
    wvt = torch.tensor(world_to_view(out.R, out.T)).transpose(0, 1)
    out._set(wvt, projection_matrix(out.znear, out.zfar, out.FoVx, out.FoVy).transpose(0, 1))
    return out


def camera_centre(cam) -> np.ndarray:
    from .edit import _camera_pose
    return _camera_pose(cam)[1]


def _at_size(cam, W: int, H: int):
    """the same camera with a W x H image plane (same field of view: the matrices do not change)"""
    if (int(cam.image_width), int(cam.image_height)) == (W, H):
        return cam
    from .camera import Camera
    out = Camera.__new__(Camera)
    out.__dict__.update(cam.__dict__)
    out.image_width, out.image_height = int(W), int(H)
    out.original_image = out.gt_alpha_mask = out.bg_mask = None
    return out


def camera_gradient(model, cam, pipe, bg, loss_fn: Callable, *, pivot=None, return_loss: bool = False):
    """device float64 [6]: the gradient of loss_fn(out) with respect to a world-frame twist of `cam` about `pivot` (default:
    the camera centre, so that omega turns the camera on the spot).  One drop-in render() with the model's parameters
    requiring grad; loss_fn gets the render's dict with the keys "render" [3,H,W], "depth" and "alpha" [1,H,W] added to
    render()'s own; torch.autograd.grad with respect to _xyz, _rotation and _features_rest only; one pose_gradient launch over
    the rows with radii > 0.  The model's .grad fields are left as they were.  return_loss: -> (gradient, the detached loss)."""
    from .render import render
    params = [model._xyz, model._rotation, model._features_rest]
    was = [p.requires_grad for p in params]
    try:
        for p in params:
            p.requires_grad_(True)
        with torch.enable_grad():
            pkg = render(cam, model, pipe, bg)
            out = dict(pkg)
            out["depth"], out["alpha"] = pkg["rendered_depth"], pkg["rendered_alpha"]
            loss = loss_fn(out)
            want = [p for p in params if p.numel() > 0]
            got = torch.autograd.grad(loss, want, allow_unused=True)
    finally:
        for p, w in zip(params, was):
            p.requires_grad_(w)
    got = list(got) + [None] * (3 - len(got))
    if got[0] is None or got[1] is None:
        raise ValueError("camera_gradient: the loss does not depend on the render")
    c = camera_centre(cam) if pivot is None else pivot
    g = pose_gradient(model, [tuple(got)], pivot=c, skip=[pkg["radii"].detach() == 0])[0]
    return (g, loss.detach()) if return_loss else g


# ---- refinement ----------------------------------------------------------------------------------------------------------------
def _resized(image: torch.Tensor, W: int, H: int) -> torch.Tensor:
    """[C,h,w] float in [0,1] -> [C,H,W] by the project's bicubic resize (ground_truth.prepare_ground_truth: PIL's BICUBIC on
    8 bits per channel); the image itself when the size does not change"""
    if (int(image.shape[2]), int(image.shape[1])) == (W, H):
        return image
    from .ground_truth import prepare_ground_truth
    src = torch.clamp(image.detach() * 255.0 + 0.5, 0.0, 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()
    return prepare_ground_truth([src], (W, H), device=image.device)[0][0]


def photometric_loss(image: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], lambda_dssim: float) -> torch.Tensor:
    """(1 - lambda) L1 + lambda (1 - SSIM) through loss_utils, both images multiplied by the mask when there is one"""
    from .loss_utils import l1_loss, ssim
    if mask is not None:
        l1 = l1_loss(image, gt, mask)
        image, gt = image * mask, gt * mask
    else:
        l1 = l1_loss(image, gt)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ssim(image, gt))


def refine_pose(model, cam, image: torch.Tensor, *, mask: Optional[torch.Tensor] = None, iters: int = 100, lr_rot: float = LR_ROT,
                lr_trans: float = LR_TRANS, lambda_dssim: float = 0.2, scales: Sequence[int] = (4, 2, 1), pipe=None, bg=None, pivot=None):
    """Align `cam` to `image` ([3,H,W] on the device, optionally `mask` [1,H,W]) by photometric descent on its pose with the
    model fixed -> (camera, history).

    Adam (0.9, 0.999) on the 6-vector, on the host: every iteration renders, takes camera_gradient of
    (1 - lambda) L1 + lambda (1 - SSIM) (loss_utils), reads the six doubles and composes the step on the left of the pose
    (moved_camera: the next gradient is again taken at the identity).  That 48-byte read is the ONLY host read of an
    iteration; the losses stay on the device until the end.  Coarse to fine: the iterations are split evenly over `scales`,
    scale s renders W/s x H/s against the image resized once (the bicubic resize of ground_truth).  The twist is about
    `pivot` (default: the mean of the model's positions, read once before the loop): omega steps are lr_rot radians, t steps
    lr_trans times the camera-to-pivot distance, so one setting serves scenes of any size; both decay geometrically to 0.1 of
    their value over the run.
    history: {"loss": [...], "xi_norm": [...]} per iteration (the loss BEFORE that iteration's step; |xi| of the motion so
    far, xi = se3_log about the pivot), "twist": that xi at the end, "pivot"."""
    from .render import PipelineParams
    dev = model._xyz.device
    pipe = PipelineParams() if pipe is None else pipe
    bg = torch.zeros(3, dtype=torch.float32, device=dev) if bg is None else bg
    c = (model._xyz.detach().double().mean(dim=0).cpu().numpy() if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3))
    dist = float(np.linalg.norm(camera_centre(cam) - c))
    dist = dist if dist > 0.0 else 1.0
    W, H = int(cam.image_width), int(cam.image_height)
    iters = int(iters)
    scales = [int(s) for s in scales]
    if not scales or min(scales) < 1:
        raise ValueError("refine_pose: scales are positive integers")
    counts = [iters // len(scales) + (1 if k < iters % len(scales) else 0) for k in range(len(scales))]
    cur, total = cam, np.eye(4)
    m, v = np.zeros(6), np.zeros(6)
    unit = np.array([lr_rot] * 3 + [lr_trans * dist] * 3)
    losses, norms, step = [], [], 0
    to_pivot, from_pivot = np.eye(4), np.eye(4)
    to_pivot[:3, 3], from_pivot[:3, 3] = -c, c
    for s, n in zip(scales, counts):
        if n == 0:
            continue
        Ws, Hs = max(W // s, 1), max(H // s, 1)
        gt = _resized(image, Ws, Hs)
        mk = None if mask is None else _resized(mask, Ws, Hs)
        loss_fn = lambda out: photometric_loss(out["render"], gt, mk, lambda_dssim)       # noqa: E731
        for _ in range(n):
            g, loss = camera_gradient(model, _at_size(cur, Ws, Hs), pipe, bg, loss_fn, pivot=c, return_loss=True)
            gh = g.cpu().numpy()                                                           # the one host read
            losses.append(loss)
            step += 1
            m = 0.9 * m + 0.1 * gh
            v = 0.999 * v + 0.001 * gh * gh
            decay = LR_FINAL ** ((step - 1) / max(iters - 1, 1))
            delta = -decay * unit * (m / (1.0 - 0.9 ** step)) / (np.sqrt(v / (1.0 - 0.999 ** step)) + 1e-15)
            delta = np.where(np.isfinite(delta), delta, 0.0)
            cur = moved_camera(cur, delta, c)
            total = twist_matrix(delta, c) @ total
            norms.append(float(np.linalg.norm(se3_log(to_pivot @ total @ from_pivot))))
    host = torch.stack(losses).double().cpu().tolist() if losses else []
    return cur, {"loss": host, "xi_norm": norms, "twist": se3_log(to_pivot @ total @ from_pivot).tolist(), "pivot": c.tolist()}


def refine_poses(model, cameras: Sequence, *, masks: Optional[Sequence] = None, **kw):
    """refine_pose of every camera against its own original_image (masks: per camera None or [1,H,W]) ->
    (the refined cameras, their twists about the pivot as float64 [n,6], the histories)."""
    cams, twists, hist = [], [], []
    for k, cam in enumerate(cameras):
        if cam.original_image is None:
            raise ValueError("refine_poses: a camera without an image")
        c2, h = refine_pose(model, cam, cam.original_image, mask=None if masks is None else masks[k], **kw)
        cams.append(c2)
        twists.append(h["twist"])
        hist.append(h)
    return cams, np.asarray(twists, dtype=np.float64).reshape(len(cams), 6), hist
