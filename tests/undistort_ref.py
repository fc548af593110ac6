"""The yardstick of binocular3dgs_amd/undistort.py: numpy only, float64 and integers.

distort() repeats csrc/undistort.hip's operation order line by line (every product and sum is its own float64 rounding, as the
library, built without FMA contraction, evaluates it), so the four models without a transcendental (SIMPLE_RADIAL, RADIAL,
OPENCV, FULL_OPENCV) give the device's bits; the fisheye models differ from it only where libm's atan / sqrt and the device's
differ in the last place.  undistort() is the same Newton iteration with the same constants, undistort_map() the same
fixed-point conversion, remap() the same integer bilinear resampling, pinhole_for() the sizing rule.
"""
import numpy as np

MODEL_PARAMS = {"SIMPLE_RADIAL": 4, "RADIAL": 5, "OPENCV": 8, "OPENCV_FISHEYE": 8, "FULL_OPENCV": 12, "SIMPLE_RADIAL_FISHEYE": 4,
                "RADIAL_FISHEYE": 5}
POLYNOMIAL = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "FULL_OPENCV")
FISHEYE = ("OPENCV_FISHEYE", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
NEWTON_ITERS = 50
NEWTON_STEP2 = 1e-22
NEWTON_H = 1e-6
FISHEYE_EPS = 1e-8
MAP_LIMIT = 1 << 30


def split(model, params):
    """-> fx, fy, cx, cy, k (the coefficients behind them, COLMAP's order)"""
    p = np.asarray(params, dtype=np.float64)
    assert p.shape == (MODEL_PARAMS[model],), (model, p.shape)
    if len(p) in (4, 5):
        return p[0], p[0], p[1], p[2], p[3:]
    return p[0], p[1], p[2], p[3], p[4:]


def distort(model, params, u, v):
    """Normalised (u, v) float64 arrays -> the distorted normalised point, in the device's operation order."""
    k = split(model, params)[4]
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        u2, v2 = u * u, v * v
        r2 = u2 + v2
        if model == "SIMPLE_RADIAL":
            rad = k[0] * r2
            return u + u * rad, v + v * rad
        if model == "RADIAL":
            rad = k[0] * r2 + k[1] * (r2 * r2)
            return u + u * rad, v + v * rad
        if model in ("OPENCV", "FULL_OPENCV"):
            uv = u * v
            if model == "OPENCV":
                rad = k[0] * r2 + k[1] * (r2 * r2)
            else:
                r4 = r2 * r2
                r6 = r4 * r2
                num = ((1.0 + k[0] * r2) + k[1] * r4) + k[4] * r6
                den = ((1.0 + k[5] * r2) + k[6] * r4) + k[7] * r6
                rad = num / den
            tu = (2.0 * k[2]) * uv + k[3] * (r2 + 2.0 * u2)
            tv = (2.0 * k[3]) * uv + k[2] * (r2 + 2.0 * v2)
            if model == "OPENCV":
                return (u + u * rad) + tu, (v + v * rad) + tv
            return u * rad + tu, v * rad + tv
        r = np.sqrt(r2)
        small = r < FISHEYE_EPS
        rs = np.where(small, 1.0, r)
        th = np.arctan(rs)
        t2 = th * th
        if model == "OPENCV_FISHEYE":
            t4 = t2 * t2
            t6, t8 = t4 * t2, t4 * t4
            thd = th * ((((1.0 + k[0] * t2) + k[1] * t4) + k[2] * t6) + k[3] * t8)
            s = thd / rs
            ou, ov = u * s, v * s
        else:
            s = th / rs
            uu, vv = u * s, v * s
            rad = k[0] * t2
            if model == "RADIAL_FISHEYE":
                rad = rad + k[1] * (t2 * t2)
            ou, ov = uu + uu * rad, vv + vv * rad
        return np.where(small, u, ou), np.where(small, v, ov)


def undistort(model, params, ud, vd):
    """-> (u, v, converged bool): Newton's iteration of the device, point by point in lockstep (a point that has finished, either
    way, is frozen).  u, v of an unconverged point are NaN here; callers return the input there."""
    ud = np.asarray(ud, dtype=np.float64)
    vd = np.asarray(vd, dtype=np.float64)
    u, v = ud.copy(), vd.copy()
    done = np.zeros(ud.shape, dtype=bool)
    conv = np.zeros(ud.shape, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(NEWTON_ITERS):
            if done.all():
                break
            hu = NEWTON_H * np.maximum(1.0, np.abs(u))
            hv = NEWTON_H * np.maximum(1.0, np.abs(v))
            f0u, f0v = distort(model, params, u, v)
            f1u, f1v = distort(model, params, u + hu, v)
            f2u, f2v = distort(model, params, u, v + hv)
            j00, j10 = (f1u - f0u) / hu, (f1v - f0v) / hu
            j01, j11 = (f2u - f0u) / hv, (f2v - f0v) / hv
            ru, rv = f0u - ud, f0v - vd
            det = j00 * j11 - j01 * j10
            bad = ~(det > 1e-300) | ~(det < 1e300) | ~(j00 + j11 > 0.0)
            du = (j11 * ru - j01 * rv) / det
            dv = (j00 * rv - j10 * ru) / det
            s2 = du * du + dv * dv
            bad |= ~(s2 < 1e300)
            live = ~done & ~bad
            u = np.where(live, u - du, u)
            v = np.where(live, v - dv, v)
            now = live & (s2 < NEWTON_STEP2)
            conv |= now
            done |= bad | now
    return np.where(conv, u, np.nan), np.where(conv, v, np.nan), conv


def camera_points(model, params, xy, inverse):
    """Pixel coordinates [n,2] float64 -> ([n,2], converged uint8 [n]) as b3gs_camera_points"""
    fx, fy, cx, cy, _ = split(model, params)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x, y = xy[:, 0], xy[:, 1]
    u, v = (x - cx) / fx, (y - cy) / fy
    if inverse:
        ou, ov, ok = undistort(model, params, u, v)
    else:
        ou, ov = distort(model, params, u, v)
        ok = np.ones(x.shape, dtype=bool)
    with np.errstate(all="ignore"):
        out = np.stack([np.where(ok, fx * ou + cx, x), np.where(ok, fy * ov + cy, y)], axis=1)
    return out, ok.astype(np.uint8)


def to_fixed(x):
    with np.errstate(all="ignore"):
        t = np.floor(x * 256.0 + 0.5)
        fin = np.isfinite(t)
        t = np.minimum(np.maximum(np.where(fin, t, 0.0), -float(MAP_LIMIT)), float(MAP_LIMIT))
    return np.where(fin, t, -float(MAP_LIMIT)).astype(np.int32)


def undistort_map(model, params, pinhole):
    """pinhole = (W', H', fx', fy'), principal point at (W'/2, H'/2) -> int32 [H', W', 2]"""
    W, H, fxo, fyo = int(pinhole[0]), int(pinhole[1]), float(pinhole[2]), float(pinhole[3])
    fx, fy, cx, cy, _ = split(model, params)
    i = np.arange(W, dtype=np.float64)[None, :].repeat(H, axis=0)
    j = np.arange(H, dtype=np.float64)[:, None].repeat(W, axis=1)
    u = ((i + 0.5) - W * 0.5) / fxo
    v = ((j + 0.5) - H * 0.5) / fyo
    du, dv = distort(model, params, u, v)
    with np.errstate(all="ignore"):
        x = (fx * du + cx) - 0.5
        y = (fy * dv + cy) - 0.5
    return np.stack([to_fixed(x), to_fixed(y)], axis=2)


def remap(image, m):
    """uint8 [Hs,Ws,C] (or [Hs,Ws]) through int32 [H,W,2] -> (uint8 [H,W,C], valid uint8 [H,W])"""
    img = np.asarray(image)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        img = img[:, :, None]
    Hs, Ws, _ = img.shape
    X, Y = m[..., 0].astype(np.int64), m[..., 1].astype(np.int64)
    valid = (X >= -128) & (X < 256 * Ws - 128) & (Y >= -128) & (Y < 256 * Hs - 128)
    x0, y0 = X >> 8, Y >> 8
    ax, ay = (X & 255)[..., None], (Y & 255)[..., None]
    xa, xb = np.clip(x0, 0, Ws - 1), np.clip(x0 + 1, 0, Ws - 1)
    ya, yb = np.clip(y0, 0, Hs - 1), np.clip(y0 + 1, 0, Hs - 1)
    p = img.astype(np.int64)
    s = ((256 - ax) * (256 - ay) * p[ya, xa] + ax * (256 - ay) * p[ya, xb] + (256 - ax) * ay * p[yb, xa] + ax * ay * p[yb, xb])
    out = ((s + 32768) >> 16) * valid[..., None]
    return out.astype(np.uint8), (valid * 255).astype(np.uint8)


def border_centres(width, height):
    """The centres of the border pixels: left column, right column, top row, bottom row -> four [n,2] arrays"""
    ys = np.arange(height, dtype=np.float64) + 0.5
    xs = np.arange(width, dtype=np.float64) + 0.5
    left = np.stack([np.full(height, 0.5), ys], axis=1)
    right = np.stack([np.full(height, width - 0.5), ys], axis=1)
    top = np.stack([xs, np.full(width, 0.5)], axis=1)
    bottom = np.stack([xs, np.full(width, height - 0.5)], axis=1)
    return left, right, top, bottom


def pinhole_for(model, width, height, params, blank=0.0, max_scale=2.0, size=None):
    """-> (W', H', fx, fy) by the rule of binocular3dgs_amd.undistort.pinhole_for"""
    fx, fy, cx, cy, _ = split(model, params)
    if size is not None:
        return int(size[0]), int(size[1]), float(fx), float(fy)
    sides = []
    for pts in border_centres(width, height):
        out, ok = camera_points(model, params, pts, True)
        if not ok.any():
            raise ValueError("no border pixel of one side can be undistorted: give size=")
        out = out[ok.astype(bool)]
        sides.append(((out[:, 0] - cx) / fx, (out[:, 1] - cy) / fy))
    lu, ru, tv, bv = sides[0][0], sides[1][0], sides[2][1], sides[3][1]
    left = (1 - blank) * lu.max() + blank * lu.min()
    right = (1 - blank) * ru.min() + blank * ru.max()
    top = (1 - blank) * tv.max() + blank * tv.min()
    bottom = (1 - blank) * bv.min() + blank * bv.max()
    half_u, half_v = min(-left, right), min(-top, bottom)
    if not (half_u > 0 and half_v > 0):
        raise ValueError("the undistorted image is empty: give size=")
    W = min(max(int(np.floor(2 * fx * half_u)), 1), int(round(max_scale * width)))
    H = min(max(int(np.floor(2 * fy * half_v)), 1), int(round(max_scale * height)))
    return W, H, float(fx), float(fy)


# ---- the cameras of the tests: a 37 x 29 source, strong coefficients, an off-centre principal point, fx != fy where the model
# ---- has two focal lengths
TEST_SIZE = (37, 29)
TEST_CAMERAS = {
    "SIMPLE_RADIAL": (31.0, 17.3, 15.6, -0.21),
    "RADIAL": (31.0, 17.3, 15.6, -0.25, 0.06),
    "OPENCV": (31.0, 27.5, 17.3, 15.6, -0.25, 0.06, 0.011, -0.008),
    "FULL_OPENCV": (31.0, 27.5, 17.3, 15.6, -0.25, 0.06, 0.011, -0.008, 0.012, 0.05, 0.013, 0.002),
    "OPENCV_FISHEYE": (31.0, 27.5, 17.3, 15.6, 0.05, -0.02, 0.01, -0.005),
    "SIMPLE_RADIAL_FISHEYE": (31.0, 17.3, 15.6, 0.08),
    "RADIAL_FISHEYE": (31.0, 17.3, 15.6, 0.08, -0.03),
}
TEST_PINHOLE = (41, 31, 28.0, 33.0)
