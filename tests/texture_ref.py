"""The numpy yardstick of the mesh texture calls (csrc/texture.hip): a restatement of the statements 1-9 of the section
"texturing an extracted mesh" of include/b3gs_raster.h.  Integer layout, np.float32 statement by statement, vectorised over the
texels of the atlas; the visibility inputs (triangle id and depth per pixel) are those of tests/meshraster_ref.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402

F = np.float32
MIN_CELL, MAX_CELL, MAX_SIDE = 4, 256, 16384
FLT_MAX = np.finfo(F).max


# ---- statement 1: the atlas ----------------------------------------------------------------------------------------------
def atlas_height(nf, n, Wt):
    """-> Ht, 0 when there is no such atlas"""
    if nf < 1 or not MIN_CELL <= n <= MAX_CELL or not n + 1 <= Wt <= MAX_SIDE:
        return 0
    cpr = Wt // (n + 1)
    cells = (nf + 1) // 2
    Ht = n * ((cells + cpr - 1) // cpr)
    return Ht if Ht <= MAX_SIDE else 0


def owners(nf, n, Wt):
    """-> (face int64 [Ht, Wt] (-1: unowned), i, j int64 [Ht, Wt]: the local indices in the even frame)"""
    Ht = atlas_height(nf, n, Wt)
    assert Ht
    cpr = Wt // (n + 1)
    Y, X = np.mgrid[0:Ht, 0:Wt].astype(np.int64)
    cx, cy = X // (n + 1), Y // n
    li, lj = X - cx * (n + 1), Y - cy * n
    odd = (li + lj >= n).astype(np.int64)
    f = 2 * (cy * cpr + cx) + odd
    f = np.where((cx >= cpr) | (f >= nf), -1, f)
    return f, np.where(odd == 1, n - li, li), np.where(odd == 1, n - 1 - lj, lj)


def corners(nf, n, Wt):
    """-> float32 [F, 3, 2]: texel-centre coordinates (x, y) of the corners of every triangle"""
    cpr = Wt // (n + 1)
    out = np.zeros((nf, 3, 2), F)
    for f in range(nf):
        c = f // 2
        x0, y0 = (c % cpr) * (n + 1), (c // cpr) * n
        if f % 2:
            out[f] = [(x0 + n, y0 + n - 1), (x0 + 2, y0 + n - 1), (x0 + n, y0 + 1)]
        else:
            out[f] = [(x0, y0), (x0 + n - 2, y0), (x0, y0 + n - 2)]
    return out


def bilinear_footprint(x, y, w, h):
    """statements 5 and 7 -> [(column, row, weight)] of the four neighbours (python floats; exact for the lattice points the
    tests use)"""
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    fx, fy = x - x0, y - y0
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    return [(x0, y0, (1 - fx) * (1 - fy)), (x1, y0, fx * (1 - fy)), (x0, y1, (1 - fx) * fy), (x1, y1, fx * fy)]


# ---- statements 2-6 ------------------------------------------------------------------------------------------------------
def _bary(n, i, j):
    leg = F(n - 2)
    b1, b2 = i.astype(F) / leg, j.astype(F) / leg
    b0 = (F(1.0) - b1) - b2
    assert b0.dtype == F
    return b0, b1, b2


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sample(plane, sx, sy):
    """statement 5 for one plane [h, w] at float32 positions inside it -> float32"""
    h, w = plane.shape
    xf, yf = np.floor(sx), np.floor(sy)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = sx - xf, sy - yf
    gx, gy = F(1.0) - fx, F(1.0) - fy
    top = gx * plane[y0, x0] + fx * plane[y0, x1]
    bot = gx * plane[y1, x0] + fx * plane[y1, x1]
    out = gy * top + fy * bot
    assert out.dtype == F
    return out


def camera_centre(cam):
    """statement 4, first line"""
    c = np.asarray(cam, dtype=F)
    return np.array([-((c[a] * c[9] + c[3 + a] * c[10]) + c[6 + a] * c[11]) for a in range(3)], dtype=F)


def accumulate(accum, vertices, faces, cams, W, H, n, triangle_id, depth, images, slack, two_sided=False):
    """statements 2-6: accum float32 [Ht, Wt, 4] is added to in place -> the number of triangles with an index outside 0 .. V-1"""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cams = np.asarray(cams, dtype=F).reshape(-1, 14)
    images = np.asarray(images, dtype=F)
    Ht, Wt = accum.shape[:2]
    assert accum.dtype == F and atlas_height(len(faces), n, Wt) == Ht and len(cams) <= 8
    valid = ((faces >= 0) & (faces < len(vertices))).all(axis=1)
    f, li, lj = owners(len(faces), n, Wt)
    live = (f >= 0) & valid[np.maximum(f, 0)]
    fs, i, j = f[live], li[live], lj[live]
    with np.errstate(all="ignore"):
        b0, b1, b2 = _bary(n, i, j)
        v0, v1, v2 = (vertices[faces[fs, k]].T for k in range(3))               # [3, T]
        q = [(b0 * v0[a] + b1 * v1[a]) + b2 * v2[a] for a in range(3)]
        e1, e2 = v1 - v0, v2 - v0
        m = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        length = np.sqrt(_dot(m, m))
        has_normal = (length > 0) & (length <= FLT_MAX)
        nrm = [m[a] / length for a in range(3)]
        acc = accum[live].copy()
        slack = F(slack)
        for v, c in enumerate(cams):
            p = [((c[3 * r] * q[0] + c[3 * r + 1] * q[1]) + c[3 * r + 2] * q[2]) + c[9 + r] for r in range(3)]
            sx = c[12] * (p[0] / p[2]) + (F(0.5) * F(W) - F(0.5))
            sy = c[13] * (p[1] / p[2]) + (F(0.5) * F(H) - F(0.5))
            ok = has_normal & (p[2] > rr.NEAR) & (p[2] <= FLT_MAX) & (sx >= 0) & (sx <= F(W - 1)) & (sy >= 0) & (sy <= F(H - 1))
            sxs, sys_ = np.where(ok, sx, F(0)), np.where(ok, sy, F(0))
            px, py = np.rint(sxs).astype(np.int64), np.rint(sys_).astype(np.int64)
            tid, d = triangle_id[v][py, px], depth[v][0][py, px]
            ok &= (tid < 0) | (tid == fs) | (p[2] <= d + slack)
            centre = camera_centre(c)
            g = [centre[a] - q[a] for a in range(3)]
            gl = np.sqrt(_dot(g, g))
            ok &= (gl > 0) & (gl <= FLT_MAX)
            cosine = _dot(nrm, g) / gl
            if two_sided:
                cosine = np.abs(cosine)
            ok &= cosine > 0
            w = cosine * cosine
            assert w.dtype == F and sx.dtype == F
            for ch in range(3):
                s = _sample(images[v, ch], sxs, sys_)
                acc[:, ch] = np.where(ok, acc[:, ch] + w * s, acc[:, ch])
            acc[:, 3] = np.where(ok, acc[:, 3] + w, acc[:, 3])
    accum[live] = acc
    return int((~valid).sum())


# ---- statement 8 ---------------------------------------------------------------------------------------------------------
def to_byte(r):
    with np.errstate(all="ignore"):
        r = np.fmin(np.fmax(np.asarray(r, dtype=F), F(0.0)), F(1.0))          # (fmax, fmin: a NaN gives 0)
        return np.rint(F(255.0) * r).astype(np.uint8)


def finalize(accum, colours, nverts, faces, n):
    """-> (texture uint8 [Ht, Wt, 3], coverage [2])"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    Ht, Wt = accum.shape[:2]
    f, li, lj = owners(len(faces), n, Wt)
    valid = ((faces >= 0) & (faces < nverts)).all(axis=1)
    tex = np.zeros((Ht, Wt, 3), np.uint8)
    owned = f >= 0
    seen = owned & (accum[..., 3] > 0)
    with np.errstate(all="ignore"):
        for ch in range(3):
            tex[..., ch][seen] = to_byte(accum[..., ch][seen] / accum[..., 3][seen])
        back = owned & ~seen & valid[np.maximum(f, 0)]
        if colours is not None and back.any():
            col = np.asarray(colours, dtype=np.uint8).astype(F)
            b = [np.fmax(x, F(0.0)) for x in _bary(n, li[back], lj[back])]
            s = (b[0] + b[1]) + b[2]
            b = [x / s for x in b]
            idx = faces[f[back]]
            for ch in range(3):
                val = (b[0] * col[idx[:, 0], ch] + b[1] * col[idx[:, 1], ch]) + b[2] * col[idx[:, 2], ch]
                tex[..., ch][back] = to_byte(val / F(255.0))
    return tex, [int(seen.sum()), int(owned.sum())]


def bake(vertices, colours, faces, cams, W, H, images, n, Wt, slack, two_sided=False, ref=None):
    """bake_texture for cameras of one size: the rasterizer's yardstick per run of 8, accumulate, finalize
    -> (texture, coverage, bad faces, accum)"""
    cams = np.asarray(cams, dtype=F).reshape(-1, 14)
    accum = np.zeros((atlas_height(len(faces), n, Wt), Wt, 4), F)
    bad = 0
    for s in range(0, len(cams), 8):
        r = rr.render(vertices, None, faces, cams[s:s + 8], W, H, shading="normal") if ref is None else {k: ref[k][s:s + 8] for k in ("triangle_id", "depth")}
        bad = accumulate(accum, vertices, faces, cams[s:s + 8], W, H, n, r["triangle_id"], r["depth"], np.asarray(images)[s:s + 8], slack, two_sided)
    tex, cov = finalize(accum, colours, len(vertices), faces, n)
    return tex, cov, bad, accum


# ---- statement 9 ---------------------------------------------------------------------------------------------------------
def resolve_textured(vertices, faces, cams, W, H, ref, texture, n, bg=(0.0, 0.0, 0.0)):
    """the colour output of the textured resolve, float32 [nviews, 3, H, W], from the triangle ids of the rasterizer's yardstick
    `ref` (rr.render of the same mesh and cameras)"""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cams = np.asarray(cams, dtype=F).reshape(-1, 14)
    Ht, Wt = texture.shape[:2]
    uv = corners(len(faces), n, Wt)
    out = np.empty((len(cams), 3, H, W), F)
    out[:] = np.asarray(bg, dtype=F).reshape(1, 3, 1, 1)
    tex = texture.astype(F)
    for v in range(len(cams)):
        X, Y, pz, _, _, _ = rr.project(vertices, cams[v], W, H)
        ids = ref["triangle_id"][v]
        for f in np.unique(ids[ids >= 0]):
            a, b, c = (int(k) for k in faces[f])
            t = rr.setup([int(X[a]), int(X[b]), int(X[c])], [int(Y[a]), int(Y[b]), int(Y[c])], W, H)
            jj, ii = np.nonzero(ids == f)
            E, _ = rr.edge_values(t, ii, jj)
            w, z = rr.depth_of(t, E, pz[[a, b, c]])
            with np.errstate(all="ignore"):
                u = ((w[0] * uv[f, 0, 0] + w[1] * uv[f, 1, 0]) + w[2] * uv[f, 2, 0]) * z
                s = ((w[0] * uv[f, 0, 1] + w[1] * uv[f, 1, 1]) + w[2] * uv[f, 2, 1]) * z
                u = np.fmin(np.fmax(u, F(0.0)), F(Wt - 1))
                s = np.fmin(np.fmax(s, F(0.0)), F(Ht - 1))
                for ch in range(3):
                    out[v, ch, jj, ii] = _sample(tex[..., ch], u, s) / F(255.0)
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------------
def quad(x0, y0, x1, y1, z, W, H, facing=True):
    """two triangles over the pixel rectangle (x0, y0) .. (x1, y1) of the identity camera at depth z; facing: the normal
    (p1 - p0) x (p2 - p0) points to the camera (-z)"""
    v = rr.at_pixels([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], z, W, H)
    f = np.array([[0, 3, 2], [0, 2, 1]] if facing else [[0, 2, 3], [0, 1, 2]], np.int32)
    return v, f


def pattern(n, W, H, seed=0):
    """n images float32 [n, 3, H, W] of multiples of 1/255"""
    return (np.random.default_rng(seed).integers(0, 256, size=(n, 3, H, W)).astype(F) / F(255.0)).astype(F)
