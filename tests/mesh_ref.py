"""numpy restatement of csrc/mesh.hip (include/b3gs_raster.h, ABI 17): float32, one operation per statement, in the kernels' order.

    integrate(vol, cams, depths, alphas, colours, W, H, truncation, near, alpha_min)   the running average, view by view
    tables()                                                                           the 6 x 16 case table from the rule
    extract(vol, min_weight) -> vertices, colours, faces                               welded marching tetrahedra
    edge_uses / euler_characteristic / signed_volume                                   the mesh checks of the tests
    sphere_volume / random_volume / plane_scene                                        the inputs the tests share

A volume is a dict: tsdf, weight [nz,ny,nx] float32, rgb [nz,ny,nx,3] float32, origin (3 floats), voxel (float).
A camera is a row of 14 float32: world -> camera rotation (9, row-major), translation (3), fx, fy.
"""
import itertools

import numpy as np

F = np.float32
SLOT_DIR = (1, 2, 4, 3, 5, 6, 7)            # direction bits (x = 1, y = 2, z = 4) of the 7 edge slots a voxel owns
PERMS = tuple(itertools.permutations(range(3)))


def new_volume(dims, origin=(0.0, 0.0, 0.0), voxel=1.0):
    nx, ny, nz = dims
    return {"tsdf": np.ones((nz, ny, nx), F), "weight": np.zeros((nz, ny, nx), F), "rgb": np.zeros((nz, ny, nx, 3), F),
            "origin": tuple(float(v) for v in origin), "voxel": float(voxel)}


def centres(vol):
    """-> px [nx], py [ny], pz [nz]: origin + (i + 0.5) * voxel"""
    nz, ny, nx = vol["tsdf"].shape
    return [F(vol["origin"][a]) + (np.arange(n, dtype=F) + F(0.5)) * F(vol["voxel"]) for a, n in enumerate((nx, ny, nz))]


# ---- integration -------------------------------------------------------------------------------------------------------
def integrate(vol, cams, depths, alphas, colours, truncation, near=0.2, alpha_min=0.5):
    """In place; views in index order.  depths / alphas: [H,W], colours: [3,H,W], float32."""
    cx_, cy_, cz_ = centres(vol)
    px, py, pz = cx_[None, None, :], cy_[None, :, None], cz_[:, None, None]
    tsdf, w, rgb = vol["tsdf"], vol["weight"], vol["rgb"]
    trunc, near, alpha_min = F(truncation), F(near), F(alpha_min)
    with np.errstate(all="ignore"):
        for cam, depth, alpha, colour in zip(cams, depths, alphas, colours):
            c = np.asarray(cam, dtype=F)
            depth, alpha, colour = np.asarray(depth, F), np.asarray(alpha, F), np.asarray(colour, F)
            H, W = depth.shape[-2:]
            depth, alpha = depth.reshape(H, W), alpha.reshape(H, W)
            x = ((c[0] * px + c[1] * py) + c[2] * pz) + c[9]
            y = ((c[3] * px + c[4] * py) + c[5] * pz) + c[10]
            z = ((c[6] * px + c[7] * py) + c[8] * pz) + c[11]
            ok = z > near
            un = x / z
            vn = y / z
            uf = np.rint(c[12] * un + (F(0.5) * F(W) - F(0.5)))
            vf = np.rint(c[13] * vn + (F(0.5) * F(H) - F(0.5)))
            ok = ok & (uf >= 0) & (uf <= F(W - 1)) & (vf >= 0) & (vf <= F(H - 1))
            ui = np.where(ok, uf, 0).astype(np.int64)
            vi = np.where(ok, vf, 0).astype(np.int64)
            al = alpha[vi, ui]
            ok = ok & (al >= alpha_min)
            d = depth[vi, ui] / al
            sdf = d - z
            ok = ok & (sdf >= -trunc)
            val = np.minimum(F(1.0), sdf / trunc)
            wn = w + F(1.0)
            tsdf[...] = np.where(ok, (tsdf * w + val) / wn, tsdf)
            for ch in range(3):
                rgb[..., ch] = np.where(ok, (rgb[..., ch] * w + colour[ch][vi, ui]) / wn, rgb[..., ch])
            w[...] = np.where(ok, wn, w)
    assert tsdf.dtype == F and w.dtype == F and rgb.dtype == F
    return vol


# ---- the case table ----------------------------------------------------------------------------------------------------
def tet_corners(t):
    """cell corners (bit x = 1, y = 2, z = 4) of tetrahedron t: 0, e_a, e_a + e_b, 7 for the t-th permutation (a, b, c)"""
    a, b, _ = PERMS[t]
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def _pos(corner):
    return np.array([corner & 1, corner >> 1 & 1, corner >> 2], dtype=np.float64)


def tables():
    """table[t][case] = list of triangles, a triangle = 3 edges, an edge = (p, q), p < q, corners of the tetrahedron.
    Case bit p: corner p is inside.  The rule: one corner p alone on its side, the others q < r < s: (pq, pr, ps); two inside
    a < b, two outside c < d: (ac, ad, bd), (ac, bd, bc).  With the vertices at the edge midpoints the normal must point
    from the inside corners to the outside ones; otherwise the second and third vertex of every triangle change places."""
    table = []
    for t in range(6):
        cn = tet_corners(t)
        rows = []
        for case in range(16):
            ins = [p for p in range(4) if case >> p & 1]
            outs = [p for p in range(4) if not case >> p & 1]
            if not ins or not outs:
                rows.append([])
                continue
            if len(ins) == 1 or len(outs) == 1:
                p, others = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                tris = [[(p, o) for o in others]]
            else:
                (a, b), (c, d) = ins, outs
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            mid = [(_pos(cn[p]) + _pos(cn[q])) / 2 for p, q in tris[0]]
            normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
            away = np.mean([_pos(cn[p]) for p in outs], axis=0) - np.mean([_pos(cn[p]) for p in ins], axis=0)
            s = float(normal @ away)
            assert abs(s) > 1e-9
            if s < 0:
                tris = [[tr[0], tr[2], tr[1]] for tr in tris]
            rows.append([[tuple(sorted(e)) for e in tr] for tr in tris])
        table.append(rows)
    return table


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        _TABLE = tables()
    return _TABLE


# ---- extraction --------------------------------------------------------------------------------------------------------
def _offset(bits, nx, ny):
    return (bits & 1) + (bits >> 1 & 1) * nx + (bits >> 2) * nx * ny


def _shift(a, dz, dy, dx):
    """out[k, j, i] = a[k - dz, j - dy, i - dx] where that exists, else False"""
    out = np.zeros_like(a)
    nz, ny, nx = a.shape
    out[dz:, dy:, dx:] = a[:nz - dz, :ny - dy, :nx - dx]
    return out


def classify(vol, min_weight):
    """-> inside [nz,ny,nx], cell_valid [nz,ny,nx] (indexed by the cell's corner 0), active [nz,ny,nx,7] edge slots"""
    tsdf, weight = vol["tsdf"], vol["weight"]
    nz, ny, nx = tsdf.shape
    inside = tsdf < 0
    ok = weight >= F(min_weight)
    valid = np.zeros((nz, ny, nx), bool)
    if min(nx, ny, nz) >= 2:
        v = np.ones((nz - 1, ny - 1, nx - 1), bool)
        for c in range(8):
            cx, cy, cz = c & 1, c >> 1 & 1, c >> 2
            v &= ok[cz:cz + nz - 1, cy:cy + ny - 1, cx:cx + nx - 1]
        valid[:nz - 1, :ny - 1, :nx - 1] = v
    active = np.zeros((nz, ny, nx, 7), bool)
    for s, d in enumerate(SLOT_DIR):
        dx, dy, dz = d & 1, d >> 1 & 1, d >> 2
        change = np.zeros((nz, ny, nx), bool)
        change[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        used = np.zeros((nz, ny, nx), bool)
        for c in range(8):
            if c & d:
                continue
            used |= _shift(valid, c >> 2, c >> 1 & 1, c & 1)
        active[..., s] = change & used
    return inside, valid, active


def extract(vol, min_weight=1.0):
    """-> vertices float32 [V,3], colours uint8 [V,3], faces int32 [F,3]"""
    tsdf, rgb = vol["tsdf"], vol["rgb"]
    nz, ny, nx = tsdf.shape
    inside, valid, active = classify(vol, min_weight)
    flat = active.reshape(-1, 7)
    vid = (np.cumsum(flat.reshape(-1)) - 1).reshape(-1, 7)
    lin, slot = np.nonzero(flat)
    dirs = np.asarray(SLOT_DIR)[slot]
    idx = [lin % nx, lin // nx % ny, lin // (nx * ny)]
    hi = lin + _offset(dirs, nx, ny)
    tf, cf = tsdf.reshape(-1), rgb.reshape(-1, 3)
    d0, d1 = tf[lin], tf[hi]
    with np.errstate(all="ignore"):
        t = d0 / (d0 - d1)
    vertices = np.empty((len(lin), 3), F)
    colours = np.empty((len(lin), 3), np.uint8)
    for a in range(3):
        p0 = F(vol["origin"][a]) + (idx[a].astype(F) + F(0.5)) * F(vol["voxel"])
        p1 = F(vol["origin"][a]) + ((idx[a] + (dirs >> a & 1)).astype(F) + F(0.5)) * F(vol["voxel"])
        vertices[:, a] = p0 + t * (p1 - p0)
        col = (cf[lin, a] + t * (cf[hi, a] - cf[lin, a])) * F(255.0)
        colours[:, a] = np.rint(np.minimum(np.maximum(col, F(0.0)), F(255.0))).astype(np.uint8)
    assert vertices.dtype == F and t.dtype == F
    # triangles in (cell, tetrahedron, table) order
    cells = np.nonzero(valid.reshape(-1))[0]
    mf = inside.reshape(-1)
    table = _table()
    keys, tris = [], []
    for tt in range(6):
        cn = tet_corners(tt)
        case = np.zeros(len(cells), np.int64)
        for p in range(4):
            case |= mf[cells + _offset(cn[p], nx, ny)].astype(np.int64) << p
        for cs in range(1, 15):
            sel = np.nonzero(case == cs)[0]
            if not len(sel):
                continue
            for r, tri in enumerate(table[tt][cs]):
                ids = []
                for p, q in tri:
                    owner = cells[sel] + _offset(cn[p], nx, ny)
                    ids.append(vid[owner, SLOT_DIR.index(cn[q] & ~cn[p])])
                    assert flat[owner, SLOT_DIR.index(cn[q] & ~cn[p])].all()
                tris.append(np.stack(ids, axis=1))
                keys.append((sel * 6 + tt) * 2 + r)
    if not tris:
        return vertices, colours, np.zeros((0, 3), np.int32)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    return vertices, colours, tris[np.argsort(keys, kind="stable")].astype(np.int32)


def cases_seen(vol, min_weight=1.0):
    """-> bool [6, 16]: the (tetrahedron, case) pairs that occur in valid cells"""
    nz, ny, nx = vol["tsdf"].shape
    inside, valid, _ = classify(vol, min_weight)
    cells = np.nonzero(valid.reshape(-1))[0]
    seen = np.zeros((6, 16), bool)
    for tt in range(6):
        case = np.zeros(len(cells), np.int64)
        for p, corner in enumerate(tet_corners(tt)):
            case |= inside.reshape(-1)[cells + _offset(corner, nx, ny)].astype(np.int64) << p
        seen[tt, np.unique(case)] = True
    return seen


# ---- mesh checks -------------------------------------------------------------------------------------------------------
def edge_uses(faces):
    """-> (edges [E,2] with a < b, how many triangles use each)"""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)


def euler_characteristic(n_vertices, faces):
    edges, _ = edge_uses(faces)
    return int(n_vertices) - len(edges) + len(faces)


def signed_volume(vertices, faces):
    """sum of det(a, b, c) / 6 over the triangles, in float64: positive when the normals point outwards"""
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- the volumes and scenes the tests share -----------------------------------------------------------------------------
def sphere_volume(dims=(20, 18, 16), radius=6.0):
    """An exact sphere SDF (in voxels, over a truncation of 4) around the middle of the volume, every voxel observed."""
    vol = new_volume(dims)
    px, py, pz = centres(vol)
    c = [F(d / 2) for d in dims]
    dist = np.sqrt((px[None, None, :] - c[0]) ** 2 + (py[None, :, None] - c[1]) ** 2 + (pz[:, None, None] - c[2]) ** 2).astype(F)
    vol["tsdf"][...] = (dist - F(radius)) / F(4.0)
    vol["weight"][...] = 1.0
    vol["rgb"][...] = np.stack(np.broadcast_arrays(px[None, None, :] / F(dims[0]), py[None, :, None] / F(dims[1]),
                                                   pz[:, None, None] / F(dims[2])), axis=-1)
    return vol


def random_volume(dims=(9, 8, 7), seed=5, observed=0.93):
    """A random field in [-1, 1] with random 0 / 1 weights (93 % ones: a cell needs 8 of them)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    vol = new_volume(dims, origin=(-0.5, 0.25, 1.0), voxel=0.125)
    vol["tsdf"][...] = rng.uniform(-1, 1, (nz, ny, nx)).astype(F)
    vol["weight"][...] = (rng.uniform(size=(nz, ny, nx)) < observed).astype(F)
    vol["rgb"][...] = rng.uniform(size=(nz, ny, nx, 3)).astype(F)
    return vol


def plane_scene(W=40, H=30, z0=2.8):
    """Three cameras looking down +z from x = -0.3, 0, 0.3 at the plane z = z0; -> (cams [3,14], depths, alphas, colours)"""
    cams = np.zeros((3, 14), F)
    for k, x in enumerate((-0.3, 0.0, 0.3)):
        cams[k, [0, 4, 8]] = 1.0
        cams[k, 9] = -x
        cams[k, 12:] = 20.0
    alpha = np.ones((H, W), F)
    depth = np.full((H, W), z0, F) * alpha
    colour = np.full((3, H, W), 0.5, F)
    return cams, [depth] * 3, [alpha] * 3, [colour] * 3
