"""The numpy float64 statement of csrc/edit.hip and of the host loop of binocular3dgs_amd/edit.py (include/b3gs_raster.h states
the arithmetic): the basis of csrc/preprocess.hip, the transform in the header's operation order (one rounding to float32), the
selection tests, the brute-force nearest index, the fold order of the similarity sums, Umeyama's closed form and the ICP loop.
The device equals these bit for bit (tests/test_gpu_edit.py).

Mutants (as in lossfn_ref.py): transform(..., mut="sh_identity") leaves features_rest unrotated, mut="quat_right" multiplies the
quaternion on the wrong side.  tests/test_edit_ref_cpu.py shows that the render-invariance bound sees both.
"""
import math

import numpy as np

F = np.float32
TPB = 256
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def sh_basis(d):
    """Y_1 [n,3], Y_2 [n,5], Y_3 [n,7] at unit directions d [n,3]: the terms of csrc/preprocess.hip's colour sum, coefficient by
    coefficient (-C1 y, +C1 z, -C1 x, ...)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return (np.stack([-SH_C1 * y, SH_C1 * z, -SH_C1 * x], 1),
            np.stack([SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)], 1),
            np.stack([SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
                      SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                      SH_C3[6] * x * (xx - 3 * yy)], 1))


def unpack(words):
    """the 101 doubles of B3gsSimilarity -> dict"""
    w = np.asarray(words, np.float64)
    assert w.shape == (101,)
    return {"R": w[0:9].reshape(3, 3), "t": w[9:12], "s": w[12], "ln_s": w[13], "q": w[14:18], "D": (w[18:27].reshape(3, 3),
            w[27:52].reshape(5, 5), w[52:101].reshape(7, 7))}


def transform_points(points, words):
    """out_i = s * ((R_i0 x + R_i1 y) + R_i2 z) + t_i"""
    T = unpack(words)
    p = np.asarray(points, F).astype(np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    R, t, s = T["R"], T["t"], T["s"]
    return np.stack([s * ((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], axis=1).astype(F)


def transform(xyz, rotation, scaling, features_rest, words, sh_degree, mut=None):
    """-> (xyz', rotation', scaling', features_rest') float32, the header's operation order"""
    T = unpack(words)
    r = np.asarray(rotation, F).astype(np.float64).reshape(-1, 4)
    rw, rx, ry, rz = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    qw, qx, qy, qz = T["q"]
    if mut == "quat_right":          # rotation (x) q: the wrong side
        rot = np.stack([((rw * qw - rx * qx) - ry * qy) - rz * qz, ((rw * qx + rx * qw) + ry * qz) - rz * qy,
                        ((rw * qy - rx * qz) + ry * qw) + rz * qx, ((rw * qz + rx * qy) - ry * qx) + rz * qw], axis=1)
    else:
        rot = np.stack([((qw * rw - qx * rx) - qy * ry) - qz * rz, ((qw * rx + qx * rw) + qy * rz) - qz * ry,
                        ((qw * ry - qx * rz) + qy * rw) + qz * rx, ((qw * rz + qx * ry) - qy * rx) + qz * rw], axis=1)
    sc = np.asarray(scaling, F).astype(np.float64) + T["ln_s"]
    f = np.asarray(features_rest, F).astype(np.float64)
    out = f.copy()
    if mut != "sh_identity":
        first = 0
        for band in range(1, sh_degree + 1):
            n, D = 2 * band + 1, T["D"][band - 1]
            for m in range(n):
                acc = D[m, 0] * f[:, first, :]
                for k in range(1, n):
                    acc = acc + D[m, k] * f[:, first + k, :]
                out[:, first + m, :] = acc
            first += n
    return transform_points(xyz, words), rot.astype(F), sc.astype(F), out.astype(F)


# ---- selection -----------------------------------------------------------------------------------------------------------------
def _rows(M, x, y, z):
    return [((M[k, 0] * x + M[k, 1] * y) + M[k, 2] * z) + M[k, 3] for k in range(3)]


def select(xyz, opacity, scaling, box=None, sphere=None, logit_min=None, log_max_scale=None, cameras=None, masks=None, min_views=1):
    """-> (keep bool [P], seen int32 [P]).  box: (M [3,4], half [3]); sphere: (centre [3], r2); logit_min / log_max_scale: the
    float32 thresholds; cameras: float64 [V,19]; masks: uint8 [V,H,W] or None."""
    p32 = np.asarray(xyz, F).reshape(-1, 3)
    P = p32.shape[0]
    finite = np.isfinite(p32).all(axis=1)
    with np.errstate(all="ignore"):
        p = p32.astype(np.float64)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        keep = np.ones(P, bool)
        seen = np.zeros(P, np.int32)
        if box is not None:
            M, half = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
            q = _rows(M, x, y, z)
            keep &= finite & (np.abs(q[0]) <= half[0]) & (np.abs(q[1]) <= half[1]) & (np.abs(q[2]) <= half[2])
        if sphere is not None:
            c, r2 = np.asarray(sphere[0], np.float64), float(sphere[1])
            dx, dy, dz = x - c[0], y - c[1], z - c[2]
            keep &= finite & ((dx * dx + dy * dy) + dz * dz <= r2)
        if cameras is not None:
            for v, c in enumerate(np.asarray(cameras, np.float64)):
                X, Y, Z = _rows(c[:12].reshape(3, 4), x, y, z)
                ok = finite & (Z > c[18])
                pu, pv = (c[12] * X) / Z + c[14], (c[13] * Y) / Z + c[15]
                ok &= (pu >= 0.0) & (pu < c[16]) & (pv >= 0.0) & (pv < c[17])
                if masks is not None:
                    mk = np.asarray(masks)[v]
                    iu = np.where(ok, np.floor(np.where(ok, pu, 0.0)), 0).astype(np.int64)
                    iv = np.where(ok, np.floor(np.where(ok, pv, 0.0)), 0).astype(np.int64)
                    inside = (iu < mk.shape[1]) & (iv < mk.shape[0])
                    ok &= inside & (mk[np.minimum(iv, mk.shape[0] - 1), np.minimum(iu, mk.shape[1] - 1)] != 0)
                seen += ok.astype(np.int32)
            keep &= seen >= min_views
        if logit_min is not None:
            keep &= np.asarray(opacity, F).reshape(-1) >= F(logit_min)
        if log_max_scale is not None:
            keep &= np.asarray(scaling, F).reshape(-1, 3).max(axis=1) <= F(log_max_scale)
    return keep, seen


# ---- nearest point with its index -------------------------------------------------------------------------------------------------
def nearest_index(a, b, max_dist, chunk=512):
    """(min(max_dist, sqrt(min_j d2)), argmin_j d2 -- the smallest j among equal d2 -- or -1 when sqrt(min d2) > max_dist),
    d2 = (dx dx + dy dy) + dz dz in float32: brute force."""
    a, b = np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
    dist, index = np.empty(len(a), F), np.empty(len(a), np.int32)
    for s in range(0, len(a), chunk):
        d = a[s:s + chunk, None, :] - b[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = d2.argmin(axis=1)                      # (the first of equal minima)
        root = np.sqrt(d2[np.arange(len(j)), j], dtype=F)
        dist[s:s + chunk] = np.minimum(F(max_dist), root)
        index[s:s + chunk] = np.where(root <= F(max_dist), j, -1)
    return dist, index


# ---- the sums of a similarity fit ----------------------------------------------------------------------------------------------
def _butterfly(v):
    """xor butterfly 32, 16, .., 1 over the last axis (64 lanes): every lane ends with the same sum"""
    lanes = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ d]
    return v[..., 0]


def similarity_sums(a, b, index, dist, gate, mask, origin_a, origin_b):
    """float64 [18] in the kernel's order: thread t of workgroup g adds i = 256 g + t, + 256 nb, .. in order; the workgroup's
    butterfly, (wave 0 + wave 1) + (wave 2 + wave 3); one wave folds the partials b = lane, lane + 64, .. and its butterfly."""
    a, b = np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
    index = np.asarray(index, np.int64)
    N = len(a)
    ok = (index >= 0) & (index < len(b)) & (np.asarray(dist, F) <= F(gate))
    if mask is not None:
        ok &= np.asarray(mask, bool)
    at = a.astype(np.float64) - np.asarray(origin_a, np.float64)
    bt = b[np.clip(index, 0, len(b) - 1)].astype(np.float64) - np.asarray(origin_b, np.float64)
    terms = np.concatenate([np.ones((N, 1)), at, bt, ((at[:, 0] * at[:, 0] + at[:, 1] * at[:, 1]) + at[:, 2] * at[:, 2])[:, None],
                            (bt[:, :, None] * at[:, None, :]).reshape(N, 9),
                            ((bt[:, 0] * bt[:, 0] + bt[:, 1] * bt[:, 1]) + bt[:, 2] * bt[:, 2])[:, None]], axis=1)
    terms = np.where(ok[:, None], terms, 0.0)
    nb = min(max((N + 8 * TPB - 1) // (8 * TPB), 1), 256)
    per = nb * TPB
    J = (N + per - 1) // per
    terms = np.concatenate([terms, np.zeros((J * per - N, 18))]).reshape(J, nb, TPB, 18)
    t = np.zeros((nb, TPB, 18))
    for j in range(J):
        t = t + terms[j]
    wv = _butterfly(np.moveaxis(t.reshape(nb, 4, 64, 18), 2, 3))          # [nb, 4, 18]
    part = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])                 # [nb, 18]
    lanes = np.zeros((64, 18))
    for b0 in range(0, nb, 64):
        seg = part[b0:b0 + 64]
        lanes[:len(seg)] = lanes[:len(seg)] + seg
    return _butterfly(lanes.T)


# ---- Umeyama and the ICP loop --------------------------------------------------------------------------------------------------
def umeyama(sums, origin_a, origin_b, with_scale):
    """-> (R, t, s, rms): the closed form of Umeyama (PAMI 1991) from the 18 sums"""
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
    c = tr / var_a if with_scale else 1.0
    t = (mu_b + origin_b) - c * (R @ (mu_a + origin_a))
    err = var_b - 2.0 * c * tr + c * c * var_a
    return R, t, c, math.sqrt(max(err, 0.0))


def quaternion_of(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax(np.array([tr, R[0, 0], R[1, 1], R[2, 2]])))
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


def point_words(R, t, s):
    """the 101 words with the SH matrices left at the identity: all that the point transform reads"""
    return np.concatenate([np.asarray(R, np.float64).reshape(-1), np.asarray(t, np.float64), [s, math.log(s)], quaternion_of(R),
                           np.eye(3).reshape(-1), np.eye(5).reshape(-1), np.eye(7).reshape(-1)])


def register(src, dst, max_dist, iterations=30, with_scale=False, tol=1e-10):
    """The loop of edit.register with every device stage replaced by its statement above -> ((R, t, s), history)."""
    src, dst = np.asarray(src, F).reshape(-1, 3), np.asarray(dst, F).reshape(-1, 3)
    oa = 0.5 * (src.min(axis=0).astype(np.float64) + src.max(axis=0).astype(np.float64))
    ob = 0.5 * (dst.min(axis=0).astype(np.float64) + dst.max(axis=0).astype(np.float64))
    R, t, s = np.eye(3), np.zeros(3), 1.0
    history = []
    for _ in range(iterations):
        cur = transform_points(src, point_words(R, t, s))
        dist, index = nearest_index(cur, dst, max_dist)
        sums = similarity_sums(src, dst, index, dist, max_dist, None, oa, ob)
        n = int(sums[0])
        if n < 3:
            raise ValueError("fewer than 3 pairs")
        R, t, s, rms = umeyama(sums, oa, ob, with_scale)
        history.append((n, rms))
        if len(history) > 1:
            n0, r0 = history[-2]
            if abs(n - n0) <= tol * n0 and abs(rms - r0) <= tol * max(r0, 1e-300):
                break
    return (R, t, s), history


# ---- the seeded cases the CPU test (the oracle, d_ref, the mutants) and the GPU test (the device) share ------------------------
CASE_SEED = 7          # chosen so that d_ref < 1e-4 (tests/test_edit_ref_cpu.py asserts it)
CASE_W, CASE_H, CASE_P = 64, 48, 2000
_cache = {}


def random_similarity(seed, smin=0.5, smax=2.0):
    """(R, t, s): a rotation from a normal quaternion, t in [-2, 2]^3, s log-uniform in [smin, smax]"""
    g = np.random.default_rng(seed)
    q = g.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return R, g.uniform(-2.0, 2.0, 3), float(np.exp(g.uniform(math.log(smin), math.log(smax))))


def render_case(seed=CASE_SEED):
    """(The SH matrices, the quaternion and the moved cameras of the case come from the code under test -- Similarity.device_words,
    edit.transform_cameras: what stands against them is the dense oracle (d_ref) and the basis restated above, not this module.)
    P = 2000 Gaussians of sh_degree 3 with features_rest of order 1, two cameras at 64 x 48, a random similarity with s in
    [0.5, 2] -> dict(model, cameras, T, moved_cameras, words); CPU tensors."""
    import torch
    from binocular3dgs_amd import edit, synth
    from binocular3dgs_amd.gaussian_model import GaussianModel
    p = synth.synth_gaussians(CASE_P, seed, CASE_W, CASE_H, K=16, scale_mult=3.0)
    g = torch.Generator().manual_seed(seed + 1)
    p["features_rest"] = torch.randn(CASE_P, 15, 3, generator=g)
    model = GaussianModel.from_tensors(p["xyz"], p["features_dc"], p["features_rest"], p["scaling"], p["rotation"], p["opacity"],
                                       sh_degree=3, requires_grad=False)
    cams = synth.synth_cameras(CASE_W, CASE_H, yaws=(0.0, 8.0))
    T = edit.Similarity(*random_similarity(seed + 2))
    return {"model": model, "cameras": cams, "T": T, "moved_cameras": edit.transform_cameras(cams, T), "words": T.device_words()}


def moved_model(case, mut=None):
    """the yardstick's transform of the case's model -> GaussianModel (CPU)"""
    import torch
    from binocular3dgs_amd.gaussian_model import GaussianModel
    m = case["model"]
    xyz, rot, sc, rest = transform(m._xyz.numpy(), m._rotation.numpy(), m._scaling.numpy(), m._features_rest.numpy(), case["words"], 3, mut)
    t = torch.from_numpy
    return GaussianModel.from_tensors(t(xyz), m._features_dc, t(rest), t(sc), t(rot), m._opacity, sh_degree=3, requires_grad=False)


def oracle_render(model, cam):
    """(colour [3,H,W], depth [1,H,W], alpha [1,H,W]) float64 numpy from oracle/dense_torch.py"""
    import torch
    from oracle import dense_torch
    with torch.no_grad():
        r = dense_torch.render_dense(
            means3D=model._xyz, opacities=torch.sigmoid(model._opacity.double()), scales=torch.exp(model._scaling.double()),
            rotations=torch.nn.functional.normalize(model._rotation.double()), shs=model.get_features,
            viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center, bg=torch.zeros(3),
            W=cam.image_width, H=cam.image_height, tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), sh_degree=3)
    return r["color"].numpy(), r["depth"].numpy(), r["alpha"].numpy()


def render_difference(a, b, s):
    """largest per-pixel difference of two (colour, depth, alpha) renders: colour and alpha absolute, depth'/s relative to depth"""
    dc = float(np.abs(a[0] - b[0]).max())
    da = float(np.abs(a[2] - b[2]).max())
    dd = float((np.abs(a[1] - b[1] / s) / np.maximum(np.abs(a[1]), 1.0)).max())
    return max(dc, da, dd)


def oracle_originals(seed=CASE_SEED):
    if ("orig", seed) not in _cache:
        case = render_case(seed)
        _cache[("orig", seed)] = (case, [oracle_render(case["model"], c) for c in case["cameras"]])
    return _cache[("orig", seed)]


def d_of(mut=None, seed=CASE_SEED):
    """the largest pixel difference between the oracle's render of (model, cameras) and of (yardstick-transformed model,
    transformed cameras); mut=None: d_ref"""
    if (mut, seed) not in _cache:
        case, orig = oracle_originals(seed)
        mm = moved_model(case, mut)
        _cache[(mut, seed)] = max(render_difference(o, oracle_render(mm, c), case["T"].s) for o, c in zip(orig, case["moved_cameras"]))
    return _cache[(mut, seed)]


def surface_points(n, seed=0):
    """n float32 points on a bumpy height field without a symmetry (the registration cases)"""
    g = np.random.default_rng(seed)
    x, y = g.uniform(-1.0, 1.0, n), g.uniform(-0.7, 0.7, n)
    z = 0.3 * np.sin(2.1 * x + 0.4) * np.cos(1.3 * y) + 0.15 * x * y + 0.1 * np.exp(-8.0 * ((x - 0.3) ** 2 + (y + 0.2) ** 2)) + 0.2 * x
    return np.stack([x, y, z], axis=1).astype(F)
