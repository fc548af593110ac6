"""The rule of csrc/simplify.hip (include/b3gs_raster.h) restated in numpy and nothing else: the grid, the clusters,
the faces that survive, the colours and the two placements.  Float32 statements are one operation each; the fp64 statements
of the mean and of the quadric are one operation each, in the header's order.  The device gives ONE THREAD per cluster, which
adds its members in vertex-index order and its faces in face-index order; `_ordered_sum` below adds the j-th term of every
cluster at once, for j = 0, 1, ..: per cluster that is the same sequence of additions.

    simplify(vertices, colours, faces, cell, placement) -> vertices, colours, faces, info
    count_triangles(vertices, faces, cell)              -> the triangles simplify() would leave
    sphere_mesh / grid_mesh / roof_mesh                 the inputs the tests share
"""
import numpy as np

F = np.float32
D = np.float64
MAX_CELLS = 1024


def cell_coords(vertices, cell):
    """-> (origin float32 [3], integer cell coordinates int64 [V, 3]); ValueError as the device counts them"""
    v = np.asarray(vertices, F).reshape(-1, 3)
    if not np.isfinite(v).all():
        raise ValueError("not finite")
    o = v.min(axis=0)
    with np.errstate(all="ignore"):
        c = np.floor((v - o[None, :]) / F(cell))
    assert c.dtype == F
    if not ((c >= 0) & (c < MAX_CELLS)).all():
        raise ValueError("more than 1024 cells")
    return o, c.astype(np.int64)


def clusters(vertices, cell):
    """-> dict: origin, key [V], cid [V] (rank of the key among the distinct keys), members (vertex indices in (cluster, vertex
    index) order), start [K + 1]"""
    o, c = cell_coords(vertices, cell)
    key = (c[:, 2] << 20) | (c[:, 1] << 10) | c[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    head = np.ones(len(skey), bool)
    head[1:] = skey[1:] != skey[:-1]
    cid = np.empty(len(key), np.int64)
    cid[order] = np.cumsum(head) - 1
    start = np.concatenate([np.nonzero(head)[0], [len(key)]]).astype(np.int64)
    return {"origin": o, "key": key, "cid": cid, "members": order, "start": start, "cell_of_cluster": c[order[start[:-1]]]}


def surviving_faces(cid, faces):
    """-> (survive bool [F], degenerate count, duplicate count)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= len(cid)):
        raise ValueError("face index")
    tri = cid[f] if len(f) else np.zeros((0, 3), np.int64)
    degenerate = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    s = np.sort(tri, axis=1)
    survive = np.zeros(len(f), bool)
    live = np.nonzero(~degenerate)[0]
    if len(live):
        order = live[np.lexsort((s[live, 2], s[live, 1], s[live, 0]))]        # stable: ties stay in face-index order
        t = s[order]
        first = np.ones(len(order), bool)
        first[1:] = (t[1:] != t[:-1]).any(axis=1)
        survive[order[first]] = True
    return survive, int(degenerate.sum()), int(len(live) - survive.sum())


def _ordered_sum(terms, start):
    """terms [N, ...] fp64 grouped by cluster (group k = rows start[k] .. start[k+1]-1) -> the sums [K, ...], every group added
    row by row from 0.0"""
    K = len(start) - 1
    acc = np.zeros((K,) + terms.shape[1:], D)
    n = start[1:] - start[:-1]
    for j in range(int(n.max()) if K else 0):
        sel = np.nonzero(n > j)[0]
        acc[sel] = acc[sel] + terms[start[sel] + j]
    return acc


def incidences(cid, faces, K):
    """The (cluster, face) list: a face once per distinct cluster of its corners, sorted stably by cluster
    -> (face index per incidence, start [K + 1])"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tri = cid[f]
    keep = np.ones(tri.shape, bool)
    keep[:, 1] = tri[:, 1] != tri[:, 0]
    keep[:, 2] = (tri[:, 2] != tri[:, 0]) & (tri[:, 2] != tri[:, 1])
    cl = tri.reshape(-1)[keep.reshape(-1)]
    fi = np.repeat(np.arange(len(f)), 3)[keep.reshape(-1)]
    order = np.argsort(cl, kind="stable")
    start = np.searchsorted(cl[order], np.arange(K + 1), side="left")
    return fi[order], start.astype(np.int64)


def means(vertices, cl):
    """-> m fp64 [K, 3]: the ordered fp64 sum of the members / n"""
    v = np.asarray(vertices, F).reshape(-1, 3).astype(D)
    n = (cl["start"][1:] - cl["start"][:-1]).astype(D)
    return _ordered_sum(v[cl["members"]], cl["start"]) / n[:, None]


def quadric_offsets(vertices, faces, cl, m, cell):
    """-> y fp64 [K, 3]"""
    v = np.asarray(vertices, F).reshape(-1, 3).astype(D)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    K = len(m)
    y = np.zeros((K, 3), D)
    if not len(f):
        return y
    fi, start = incidences(cl["cid"], f, K)
    kk = np.repeat(np.arange(K), start[1:] - start[:-1])
    p0, p1, p2 = v[f[fi, 0]], v[f[fi, 1]], v[f[fi, 2]]
    u, w = p1 - p0, p2 - p0
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    q = p0 - m[kk]
    d = (nx * q[:, 0] + ny * q[:, 1]) + nz * q[:, 2]
    terms = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, d * nx, d * ny, d * nz], axis=1)
    A00, A01, A02, A11, A12, A22, r0, r1, r2 = _ordered_sum(terms, start).T
    lam = 1e-3 * ((A00 + A11) + A22)
    with np.errstate(all="ignore"):
        a00, a11, a22 = A00 + lam, A11 + lam, A22 + lam
        l00 = np.sqrt(a00)
        l10 = A01 / l00
        l20 = A02 / l00
        l11 = np.sqrt(a11 - l10 * l10)
        l21 = (A12 - l20 * l10) / l11
        l22 = np.sqrt((a22 - l20 * l20) - l21 * l21)
        z0 = r0 / l00
        z1 = (r1 - l10 * z0) / l11
        z2 = ((r2 - l20 * z0) - l21 * z1) / l22
        y2 = z2 / l22
        y1 = (z1 - l21 * y2) / l11
        y0 = ((z0 - l10 * y1) - l20 * y2) / l00
        sol = np.stack([y0, y1, y2], axis=1)
        ok = (lam != 0.0) & np.isfinite(sol).all(axis=1)
        ok &= ~(np.abs(np.where(np.isfinite(sol), sol, 0.0)).max(axis=1) > D(F(cell)))
    y[ok] = sol[ok]
    return y


def simplify(vertices, colours, faces, cell, placement="quadric"):
    """-> (vertices float32 [V', 3], colours uint8 [V', 3], faces int32 [F', 3], info); info: clusters, vertices_dropped,
    triangles_degenerate, triangles_duplicate (the device's statistics), and for the tests mean (fp64 [V', 3]), cluster_cell
    (int [V', 3]), origin, kept_faces (input indices of the survivors), cluster_of_vertex (new id per input vertex or -1)"""
    assert placement in ("quadric", "mean")
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    V = len(vertices)
    if V == 0:
        if len(faces):
            raise ValueError("face index")
        return vertices, colours, faces, {"clusters": 0, "vertices_dropped": 0, "triangles_degenerate": 0, "triangles_duplicate": 0}
    cl = clusters(vertices, cell)
    K = len(cl["start"]) - 1
    survive, ndeg, ndup = surviving_faces(cl["cid"], faces)
    used = np.zeros(K, bool)
    used[cl["cid"][faces[survive].astype(np.int64)].reshape(-1)] = True
    newid = np.where(used, np.cumsum(used) - 1, -1)
    n = cl["start"][1:] - cl["start"][:-1]
    csum = np.add.reduceat(colours[cl["members"]].astype(np.int64), cl["start"][:-1], axis=0)
    col = ((2 * csum + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    m = means(vertices, cl)
    y = quadric_offsets(vertices, faces, cl, m, cell) if placement == "quadric" else np.zeros_like(m)
    pos = (m + y).astype(F)
    out_faces = newid[cl["cid"][faces[survive].astype(np.int64)]].astype(np.int32).reshape(-1, 3)
    info = {"clusters": K, "vertices_dropped": V - int(used.sum()), "triangles_degenerate": ndeg, "triangles_duplicate": ndup,
            "mean": m[used], "cluster_cell": cl["cell_of_cluster"][used], "origin": cl["origin"], "kept_faces": np.nonzero(survive)[0],
            "cluster_of_vertex": newid[cl["cid"]]}
    return pos[used], col[used], out_faces, info


def stats(info):
    return {k: info[k] for k in ("clusters", "vertices_dropped", "triangles_degenerate", "triangles_duplicate")}


def count_triangles(vertices, faces, cell):
    cl = clusters(np.asarray(vertices, F).reshape(-1, 3), cell)
    return int(surviving_faces(cl["cid"], faces)[0].sum())


# ---- the meshes the tests share ------------------------------------------------------------------------------------------
def sphere_mesh(dims=(24, 24, 24), radius=8.0):
    """The marching-tetrahedra sphere of tests/mesh_ref.py: voxel 1, centre dims / 2 -> vertices, colours, faces"""
    import mesh_ref as mr
    return mr.extract(mr.sphere_volume(dims, radius))


def grid_mesh(nx, ny, step=1.0, z=0.0):
    """A planar nx x ny vertex grid cut into 2 (nx-1) (ny-1) triangles"""
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    v = np.stack([i.reshape(-1) * step, j.reshape(-1) * step, np.full(nx * ny, z)], axis=1).astype(F)
    a = (j[:-1, :-1] * nx + i[:-1, :-1]).reshape(-1)
    f = np.stack([np.stack([a, a + 1, a + nx], axis=1), np.stack([a + 1, a + nx + 1, a + nx], axis=1)], axis=1).reshape(-1, 3)
    c = np.stack([(i.reshape(-1) * 7) % 256, (j.reshape(-1) * 5) % 256, ((i + j).reshape(-1) * 3) % 256], axis=1).astype(np.uint8)
    return v, c, f.astype(np.int32)


def roof_mesh(slope, n=17, cell=4.0):
    """Two planes z = slope * (ridge - |x - ridge|) over an n x n unit grid (x, y = 0 .. n-1); with cell = 4 the ridge x = 6
    runs through the middle of the cells 4 <= x < 8 -> vertices, colours, faces, ridge"""
    v, c, f = grid_mesh(n, n)
    ridge = 6.0
    v[:, 2] = (F(slope) * (F(ridge) - np.abs(v[:, 0] - F(ridge)))).astype(F)
    return v, c, f, ridge
