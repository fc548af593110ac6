"""float64 numpy restatements the matcher-cloud tests are held against where the reference's own statement cannot be recorded
(OpenCV's triangulatePoints is not installed where the goldens are made) or where a tolerance has to be derived from the
reference's own rounding noise.  Nothing here is imported by the package."""
import numpy as np


def dlt_homogeneous(P0, P1, kp0, kp1):
    """[N,4] float64: per match the right singular vector of the smallest singular value of the 4x4 system with rows
    x*P[2] - P[0], y*P[2] - P[1] of both views (what cv2.triangulatePoints solves)."""
    P0, P1 = np.asarray(P0, np.float64), np.asarray(P1, np.float64)
    kp0, kp1 = np.asarray(kp0, np.float64), np.asarray(kp1, np.float64)
    out = np.empty((len(kp0), 4))
    for i in range(len(kp0)):
        A = np.stack([kp0[i, 0] * P0[2] - P0[0], kp0[i, 1] * P0[2] - P0[1], kp1[i, 0] * P1[2] - P1[0], kp1[i, 1] * P1[2] - P1[1]])
        out[i] = np.linalg.svd(A)[2][-1]
    return out


def dlt_points_f32(P0, P1, kp0, kp1):
    """[N,3] float32, rounded where the reference rounds: the homogeneous point leaves triangulatePoints as float32 (its inputs
    are float32) and `points / points[3]` divides in float32."""
    h = dlt_homogeneous(P0, P1, kp0, kp1).astype(np.float32)
    return (h / h[:, 3:4])[:, :3]


def dlt_points_f64(P0, P1, kp0, kp1):
    h = dlt_homogeneous(P0, P1, kp0, kp1)
    return (h / h[:, 3:4])[:, :3]


def ssim_f64(src_patch, ref_patch, window):
    """Mean over channels of the windowed SSIM of two [N,121,3] patch stacks, every step in float64 (window [121])."""
    x, y, w = np.asarray(src_patch, np.float64), np.asarray(ref_patch, np.float64), np.asarray(window, np.float64).reshape(1, -1, 1)
    mu1, mu2 = (w * x).sum(1), (w * y).sum(1)
    s1, s2, s12 = (w * x * x).sum(1) - mu1 * mu1, (w * y * y).sum(1) - mu2 * mu2, (w * x * y).sum(1) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean(-1)


def sheet_points_f64(W, H, intrinsic, c2w, depth):
    """World points of constant depth behind every pixel, pixel order, float64: [x, y, 1] * depth @ inverse(K^T), then c2w."""
    K, E = np.asarray(intrinsic, np.float64), np.asarray(c2w, np.float64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cam = np.stack([xs * depth, ys * depth, np.full_like(xs, depth)], -1).reshape(-1, 3) @ np.linalg.inv(K.T)
    return (np.concatenate([cam, np.ones((len(cam), 1))], 1) @ E.T)[:, :3]


def project_f64(points, intrinsic, c2w):
    """pixel coordinates [N,2] of world points, float64"""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    p = np.asarray(points, np.float64) @ w2c[:3, :3].T + w2c[:3, 3]
    q = p @ np.asarray(intrinsic, np.float64).T
    return q[:, :2] / q[:, 2:]
