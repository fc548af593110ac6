"""numpy restatement of csrc/poisson.hip (include/b3gs_raster.h, screened Poisson reconstruction): float32 unless stated, one
operation per statement, in the kernels' order; sums across nodes are the kernels' fixed fp64 trees.

    oriented_points(cams, depths, alphas, colours, stride, alpha_min, rel_jump, min_cos, median)  -> points, normals, weights, colours
    splat(points, normals, weights, dims, origin, voxel) -> density [nz,ny,nx], vector [3,nz,ny,nx], dropped
    rhs(vector), apply(density, screen, x), dot(u, v)
    solve(density, vector, screen, iters, tol) -> dict(x, rhs, iterations, done, status, rr, bb)
    to_volume(density, x, spread, origin, voxel) -> a volume of mesh_ref (tsdf, weight, rgb) and iso
    reconstruct(points, normals, weights, dims, origin, voxel, screen, iters, tol, spread, min_weight) -> vertices, colours, faces, info
    fibonacci_sphere / the shapes the tests share

The hooks `screening` (False: the operator without its screening term) and `fold_order` ("reversed": nodes and partials taken from the
last to the first) exist for the mutants of tests/test_poisson_ref_cpu.py only.
"""
import numpy as np

F = np.float32
D = np.float64


# ---- oriented samples --------------------------------------------------------------------------------------------------
def oriented_points(cams, depths, alphas, colours, stride=1, alpha_min=0.5, rel_jump=0.05, min_cos=0.1, median=False, zero_normal_rule=True):
    """zero_normal_rule=False drops the |n| > 0 test (a mutant for the tests only).  cams: [n,14] rows (rotation 9 row-major, translation 3, fx, fy), world -> camera; depths / alphas [H,W], colours [3,H,W]."""
    out = [[], [], [], []]
    alpha_min, rel_jump, min_cos = F(alpha_min), F(rel_jump), F(min_cos)
    with np.errstate(all="ignore"):
        for cam, depth, alpha, colour in zip(cams, depths, alphas, colours):
            c = np.asarray(cam, F)
            depth, alpha, colour = np.asarray(depth, F), np.asarray(alpha, F), np.asarray(colour, F)
            H, W = depth.shape[-2:]
            depth, alpha = depth.reshape(H, W), alpha.reshape(H, W)
            if W < 3 or H < 3:
                continue
            py, px = np.mgrid[1:H - 1, 1:W - 1]
            ok = (px % stride == 0) & (py % stride == 0)
            z = depth if median else depth / alpha
            offs = ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))
            zs, Ps = [], []
            cx, cy = F(0.5) * F(W) - F(0.5), F(0.5) * F(H) - F(0.5)
            for ox, oy in offs:
                ok = ok & (alpha[py + oy, px + ox] >= alpha_min)
                zq = z[py + oy, px + ox]
                u = ((px + ox).astype(F) - cx) / c[12]
                w = ((py + oy).astype(F) - cy) / c[13]
                zs.append(zq)
                Ps.append((u * zq, w * zq, zq))
            lim = rel_jump * zs[0]
            for k in range(1, 5):
                ok = ok & (np.abs(zs[k] - zs[0]) <= lim)
            e = [Ps[2][x] - Ps[1][x] for x in range(3)]
            f = [Ps[4][x] - Ps[3][x] for x in range(3)]
            n = (f[1] * e[2] - f[2] * e[1], f[2] * e[0] - f[0] * e[2], f[0] * e[1] - f[1] * e[0])
            nn = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            if zero_normal_rule:
                ok = ok & (nn > 0)
            P = Ps[0]
            pn = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
            d0 = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
            cs = (F(0.0) - d0) / (nn * pn)
            ok = ok & (cs > min_cos)
            u = [n[x] / nn for x in range(3)]
            t = [P[x] - c[9 + x] for x in range(3)]
            pos = np.stack([(c[x] * t[0] + c[3 + x] * t[1]) + c[6 + x] * t[2] for x in range(3)], axis=-1)
            nrm = np.stack([(c[x] * u[0] + c[3 + x] * u[1]) + c[6 + x] * u[2] for x in range(3)], axis=-1)
            col = np.stack([colour[x][py, px] for x in range(3)], axis=-1)
            assert pos.dtype == F and nrm.dtype == F and cs.dtype == F
            out[0].append(pos[ok]), out[1].append(nrm[ok]), out[2].append(cs[ok]), out[3].append(col[ok])   # (py, px) order
    if not out[0]:
        return np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F), np.zeros((0, 3), F)
    return tuple(np.concatenate(a).astype(F) for a in out)


# ---- splat -------------------------------------------------------------------------------------------------------------
def splat(points, normals, weights, dims, origin, voxel):
    """-> density [nz,ny,nx] float32, vector [3,nz,ny,nx] float32, the number of dropped samples"""
    nx, ny, nz = dims
    points, normals, weights = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3), np.asarray(weights, F).reshape(-1)
    n = nx * ny * nz
    acc = np.zeros((4, n), D)
    with np.errstate(all="ignore"):
        c = (points - np.asarray(origin, F)[None, :]) / F(voxel) - F(0.5)
        base = np.floor(c)
        frac = c - base
        ok = np.ones(len(points), bool)
        for a, d in enumerate(dims):
            ok &= (base[:, a] >= 0) & (base[:, a] <= F(d - 2))
    dropped = int((~ok).sum())
    idx = np.nonzero(ok)[0]                                          # sample order
    b = base[idx].astype(np.int64)
    key = (b[:, 2] * ny + b[:, 1]) * nx + b[:, 0]
    order = np.argsort(key, kind="stable")
    idx, b, key = idx[order], b[order], key[order]
    # the rank of every member inside its cell
    first = np.r_[True, key[1:] != key[:-1]] if len(key) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(key)), 0)) if len(key) else np.zeros(0, np.int64)
    rank = np.arange(len(key)) - start
    fr, w, nr = frac[idx], weights[idx], normals[idx]
    for corner in range(8):                                           # a node meets its cells in (dz, dy, dx) order
        dx, dy, dz = corner & 1, corner >> 1 & 1, corner >> 2
        tx = fr[:, 0] if dx else F(1.0) - fr[:, 0]
        ty = fr[:, 1] if dy else F(1.0) - fr[:, 1]
        tz = fr[:, 2] if dz else F(1.0) - fr[:, 2]
        t = (tx * ty) * tz
        assert t.dtype == F
        wt = w.astype(D) * t.astype(D)
        node = ((b[:, 2] + dz) * ny + (b[:, 1] + dy)) * nx + (b[:, 0] + dx)
        for r in range(int(rank.max()) + 1 if len(rank) else 0):      # members in order: one per node and pass
            sel = rank == r
            acc[0, node[sel]] = acc[0, node[sel]] + wt[sel]
            for a in range(3):
                acc[1 + a, node[sel]] = acc[1 + a, node[sel]] + wt[sel] * nr[sel, a].astype(D)
    out = acc.astype(F)
    return out[0].reshape(nz, ny, nx), out[1:].reshape(3, nz, ny, nx), dropped


# ---- sums --------------------------------------------------------------------------------------------------------------
def _butterfly(v):
    """[..., 64] -> [...]: the xor butterfly 32, 16, .., 1 (lane 0's value)"""
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ d]
    return v[..., 0]


def partials(q):
    """fp64 [n] -> one partial per 256 consecutive values (missing ones are +0)"""
    q = np.asarray(q, D).reshape(-1)
    nb = (len(q) + 255) // 256
    pad = np.zeros(nb * 256, D)
    pad[:len(q)] = q
    s = _butterfly(pad.reshape(nb, 4, 64))
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def fold(part, order="linear"):
    """one wave: lane l adds the partials l, l + 64, .. in order from +0, then the butterfly"""
    part = np.asarray(part, D)
    if order == "reversed":
        part = part[::-1]
    rows = (len(part) + 63) // 64
    pad = np.zeros(rows * 64, D)
    pad[:len(part)] = part
    s = np.zeros(64, D)
    for row in pad.reshape(rows, 64):
        s = s + row
    return _butterfly(s)


def dot(u, v, order="linear"):
    q = np.asarray(u, F).astype(D).reshape(-1) * np.asarray(v, F).astype(D).reshape(-1)
    return fold(partials(q[::-1] if order == "reversed" else q), order)                 # (the mutant walks the nodes backwards too)


# ---- right-hand side and operator ----------------------------------------------------------------------------------------
def _shifted(a, axis, step, fill):
    """out[c] = a[c + step] along `axis` where that exists; else `fill` (None: the node itself)"""
    if step == 0:
        return np.array(a, copy=True)
    out = np.array(a, copy=True) if fill is None else np.full_like(a, fill)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(step, None), slice(None, -step)
    else:
        src[axis], dst[axis] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def rhs(vector):
    vx, vy, vz = (np.asarray(v, F) for v in vector)                   # axes (z, y, x)
    div = ((_shifted(vx, 2, 1, 0) - _shifted(vx, 2, -1, 0)) + (_shifted(vy, 1, 1, 0) - _shifted(vy, 1, -1, 0))) + \
        (_shifted(vz, 0, 1, 0) - _shifted(vz, 0, -1, 0))
    b = F(0.0) - F(0.5) * div
    assert b.dtype == F
    return b


def apply(density, screen, x, screening=True):
    x, density = np.asarray(x, F), np.asarray(density, F)
    s = (((x - _shifted(x, 2, -1, None)) + (x - _shifted(x, 2, 1, None))) + ((x - _shifted(x, 1, -1, None)) + (x - _shifted(x, 1, 1, None)))) + \
        ((x - _shifted(x, 0, -1, None)) + (x - _shifted(x, 0, 1, None)))
    if not screening:
        return s
    sd = F(screen) * density
    out = s + sd * x
    assert out.dtype == F
    return out


# ---- conjugate gradients -------------------------------------------------------------------------------------------------
def solve(density, vector, screen, iters, tol, survivors=1, screening=True, fold_order="linear", history=None, trace=None):
    """-> dict: x, rhs float32 [nz,ny,nx]; iterations, done, status; rr, bb float64.  history (a list) receives |r| / |b| after
    every iteration, trace (a list) the float64 sums p.Ap and r.r of every iteration."""
    b = rhs(vector)
    x = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    bb = dot(b, b, fold_order)
    rr = bb
    thr = (D(F(tol)) * D(F(tol))) * bb
    status = 0 if survivors > 0 else 1
    done = bool(status) or bool(rr <= thr)
    it = 0
    bf = F(0.0)
    with np.errstate(all="ignore"):
        for k in range(iters):
            if done:
                break
            if k > 0:
                p = r + bf * p
            ap = apply(density, screen, p, screening)
            pap = dot(p, ap, fold_order)
            if pap == 0.0:
                done = True
                break
            af = F(rr / pap)
            x = x + af * p
            r = r - af * ap
            rn = dot(r, r, fold_order)
            if trace is not None:
                trace.extend((float(pap), float(rn)))
            bf = F(rn / rr)
            rr = rn
            it += 1
            if history is not None:
                history.append(float(np.sqrt(rr / bb)))
            if rn <= thr:
                done = True
    assert x.dtype == F and r.dtype == F and p.dtype == F
    return {"x": x, "rhs": b, "iterations": it, "done": done, "status": status, "rr": float(rr), "bb": float(bb)}


# ---- level and volume --------------------------------------------------------------------------------------------------
def box_sum(density, spread):
    a = np.asarray(density, F)
    for axis in (2, 1, 0):                                            # x, then y, then z
        n = a.shape[axis]
        out = np.zeros_like(a)
        for d in range(-spread, spread + 1):                          # index order: the lowest neighbour first, from +0
            if abs(d) < n:
                out = out + _shifted(a, axis, d, 0)
        a = out
    assert a.dtype == F
    return a


def to_volume(density, x, spread, origin=(0.0, 0.0, 0.0), voxel=1.0, fold_order="linear"):
    density, x = np.asarray(density, F), np.asarray(x, F)
    num = fold(partials(density.astype(D).reshape(-1) * x.astype(D).reshape(-1)), fold_order)
    den = fold(partials(density.astype(D).reshape(-1)), fold_order)
    with np.errstate(all="ignore"):
        iso = F(num / den)
    vol = {"tsdf": x - iso, "weight": box_sum(density, spread), "rgb": np.zeros(x.shape + (3,), F),
           "origin": tuple(float(v) for v in origin), "voxel": float(voxel)}
    assert vol["tsdf"].dtype == F
    return vol, iso


def reconstruct(points, normals, weights, dims, origin, voxel, screen=4.0, iters=None, tol=1e-4, spread=1, min_weight=0.0,
                screening=True, fold_order="linear", history=None):
    import mesh_ref as mr
    density, vector, dropped = splat(points, normals, weights, dims, origin, voxel)
    iters = 4 * max(dims) if iters is None else iters
    sol = solve(density, vector, screen, iters, tol, len(np.asarray(weights).reshape(-1)) - dropped, screening, fold_order, history)
    vol, iso = to_volume(density, sol["x"], spread, origin, voxel, fold_order)
    v, c, f = mr.extract(vol, min_weight)
    info = dict(sol, iso=iso, dropped=dropped, density=density, vector=vector, volume=vol)
    return v, c, f, info


# ---- the shapes the tests share ----------------------------------------------------------------------------------------
def fibonacci_sphere(n, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """n points of the Fibonacci lattice on a sphere with their outward unit normals -> points, normals float32 [n, 3]"""
    k = np.arange(n, dtype=D) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    nrm = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return (nrm * radius + np.asarray(centre, D)[None, :]).astype(F), nrm.astype(F)


def sphere_case(n=3000, res=32, pad=4):
    """A unit sphere in a grid of (res + 2 pad)^3 nodes: the sphere's diameter spans `res` voxels."""
    voxel = 2.0 / res
    dims = (res + 2 * pad,) * 3
    origin = (-1.0 - pad * voxel,) * 3
    p, nr = fibonacci_sphere(n)
    return {"points": p, "normals": nr, "weights": np.ones(n, F), "dims": dims, "origin": origin, "voxel": voxel}
