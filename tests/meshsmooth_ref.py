"""The numpy yardstick of the mesh smoothing stage (csrc/meshsmooth.hip): a restatement of the statements a-h of the section
"smoothing an extracted mesh" of include/b3gs_raster.h.  Integer work for the adjacency; np.float64 / np.float32 arrays with one
operation per statement for the filter, the normals and the shaded resolve, vectorised over the vertices (or pixels) with
the neighbours (faces) of every vertex taken in the stated order.  The shaded resolve is built on meshraster_ref.  It also
builds the test meshes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshraster_ref as rr  # noqa: E402

F = np.float32
D = np.float64
TOTALS = ("bad_faces", "nonfinite_vertices", "edges", "boundary_edges", "non_manifold_edges", "pinned_vertices", "isolated_vertices",
          "good_faces")
SHADE_SMOOTH, SHADE_LIT = 2, 3


# ---- a - e: the adjacency ------------------------------------------------------------------------------------------------
def topology(vertices, faces):
    """-> dict: offsets int32 [V + 1], indices int32 [pairs], pinned uint8 [V], inc_ranges int32 [V, 2], inc_faces int32 [slots]
    (the live slots, sorted by vertex then face), the eight totals by name and as `totals`, euler, closed"""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, nf = len(vertices), len(faces)
    good = ((faces >= 0) & (faces < V)).all(axis=1) if nf else np.zeros(0, bool)
    g = faces[good]
    # b. the six ordered pairs of every good face, in face order; equal ends dropped
    a, b, c = g[:, 0], g[:, 1], g[:, 2]
    first = np.stack([a, b, b, c, c, a], axis=1).reshape(-1)
    second = np.stack([b, a, c, b, a, c], axis=1).reshape(-1)
    live = first != second
    first, second = first[live], second[live]
    order = np.lexsort((second, first))                       # by (first, second); equal pairs need no order among themselves
    first, second = first[order], second[order]
    head = np.ones(len(first), bool)
    head[1:] = (first[1:] != first[:-1]) | (second[1:] != second[:-1])
    starts = np.nonzero(head)[0]
    df, ds = first[starts], second[starts]
    offsets = np.searchsorted(df, np.arange(V + 1), side="left").astype(np.int32)
    # c. the run length of a distinct pair with first < second = the good faces that contain the edge
    m = np.diff(np.append(starts, len(first)))
    und = df < ds
    pinned = np.zeros(V, np.uint8)
    odd = und & (m != 2)
    pinned[df[odd]] = 1
    pinned[ds[odd]] = 1
    # d. the incidence slots: a vertex the face names twice has one
    gi = np.nonzero(good)[0]
    sv = np.stack([a, b, c], axis=1)
    keep = np.ones(sv.shape, bool)
    keep[:, 1] = b != a
    keep[:, 2] = (c != a) & (c != b)
    slot_v, slot_f = sv[keep], np.repeat(gi[:, None], 3, axis=1)[keep]
    o = np.lexsort((slot_f, slot_v))
    slot_v, slot_f = slot_v[o], slot_f[o]
    lo = np.searchsorted(slot_v, np.arange(V), side="left")
    hi = np.searchsorted(slot_v, np.arange(V), side="right")
    deg = np.diff(offsets)
    with np.errstate(invalid="ignore"):
        nonfinite = int((~(np.abs(vertices) <= np.finfo(F).max).all(axis=1)).sum())
    t = {"bad_faces": int(nf - good.sum()), "nonfinite_vertices": nonfinite, "edges": int(und.sum()),
         "boundary_edges": int((und & (m == 1)).sum()), "non_manifold_edges": int((und & (m > 2)).sum()),
         "pinned_vertices": int(pinned.sum()), "isolated_vertices": int((deg == 0).sum()), "good_faces": int(good.sum())}
    out = dict(t)
    out.update({"totals": [t[k] for k in TOTALS], "offsets": offsets, "indices": ds.astype(np.int32), "pinned": pinned,
                "inc_lo": lo, "inc_hi": hi, "inc_faces": slot_f.astype(np.int32), "edge_faces": m[und],
                "euler": (V - t["isolated_vertices"]) - t["edges"] + t["good_faces"],
                "closed": t["boundary_edges"] == 0 and t["non_manifold_edges"] == 0})
    return out


def neighbours(topo, i):
    return topo["indices"][topo["offsets"][i]:topo["offsets"][i + 1]].tolist()


def incident(topo, i):
    return topo["inc_faces"][topo["inc_lo"][i]:topo["inc_hi"][i]].tolist()


# ---- f: the filter -------------------------------------------------------------------------------------------------------
def step(pos, topo, k, pin_boundary):
    """one Jacobi step with factor k: float32 [V, 3] -> float32 [V, 3]"""
    pos = np.asarray(pos, dtype=F)
    off, idx = topo["offsets"].astype(np.int64), topo["indices"].astype(np.int64)
    deg = np.diff(off)
    s = np.zeros(pos.shape, D)
    for r in range(int(deg.max()) if len(deg) else 0):            # s += (double) x_j, the r-th neighbour of every vertex that has one
        has = deg > r
        s[has] = s[has] + pos[idx[off[:-1][has] + r]].astype(D)
    move = deg > 0
    if pin_boundary:
        move &= topo["pinned"] == 0
    out = pos.copy()
    with np.errstate(all="ignore"):
        x = pos[move].astype(D)
        m = s[move] / deg[move].astype(D)[:, None]
        d = m - x
        t = D(k) * d
        out[move] = (x + t).astype(F)
    return out


def smooth(vertices, faces, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, topo=None):
    pos = np.array(vertices, dtype=F).reshape(-1, 3)
    topo = topology(pos, faces) if topo is None else topo
    for _ in range(iterations):
        pos = step(pos, topo, lam, pin_boundary)
        if mu != 0.0:
            pos = step(pos, topo, mu, pin_boundary)
    return pos


# ---- g: vertex normals ---------------------------------------------------------------------------------------------------
def face_normals64(vertices, faces):
    """fp64 from float32, one operation per statement -> float64 [F, 3] (rows of bad faces are not meaningful)"""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3).astype(D)
    f = np.clip(np.asarray(faces, dtype=np.int64).reshape(-1, 3), 0, max(len(v) - 1, 0))
    if len(v) == 0 or len(f) == 0:
        return np.zeros((len(f), 3), D)
    with np.errstate(all="ignore"):
        p0 = v[f[:, 0]]
        u, w = v[f[:, 1]] - p0, v[f[:, 2]] - p0
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return np.stack([nx, ny, nz], axis=1)


def vertex_normals(vertices, faces, topo=None):
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    topo = topology(vertices, faces) if topo is None else topo
    fn = face_normals64(vertices, faces)
    lo, cnt = topo["inc_lo"], topo["inc_hi"] - topo["inc_lo"]
    N = np.zeros((len(vertices), 3), D)
    with np.errstate(all="ignore"):
        for r in range(int(cnt.max()) if len(cnt) else 0):        # N += n, the r-th incident face of every vertex that has one
            has = cnt > r
            N[has] = N[has] + fn[topo["inc_faces"][lo[has] + r]]
        l = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        unit = (l > 0) & (l <= np.finfo(D).max)
        out = np.zeros((len(vertices), 3), F)
        out[unit] = (N[unit] / l[unit][:, None]).astype(F)
    return out


# ---- h: the shaded resolve -----------------------------------------------------------------------------------------------
def resolve_shaded(vertices, normals, faces, cams, W, H, ref, mode, bg=(0.0, 0.0, 0.0)):
    """the colour output of the shaded resolve, float32 [nviews, 3, H, W], from the triangle ids of the rasterizer's yardstick
    `ref` (rr.render of the same mesh and cameras)"""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    normals = np.asarray(normals, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cams = np.asarray(cams, dtype=F).reshape(-1, 14)
    out = np.empty((len(cams), 3, H, W), F)
    out[:] = np.asarray(bg, dtype=F).reshape(1, 3, 1, 1)
    for v in range(len(cams)):
        X, Y, pz, _, _, _ = rr.project(vertices, cams[v], W, H)
        rot = cams[v][:9]
        ids = ref["triangle_id"][v]
        for f in np.unique(ids[ids >= 0]):
            a, b, c = (int(k) for k in faces[f])
            t = rr.setup([int(X[a]), int(X[b]), int(X[c])], [int(Y[a]), int(Y[b]), int(Y[c])], W, H)
            jj, ii = np.nonzero(ids == f)
            E, _ = rr.edge_values(t, ii, jj)
            w, z = rr.depth_of(t, E, pz[[a, b, c]])
            n = normals[[a, b, c]]
            with np.errstate(all="ignore"):
                g = [((w[0] * n[0, r] + w[1] * n[1, r]) + w[2] * n[2, r]) * z for r in range(3)]
                q = [(rot[3 * r] * g[0] + rot[3 * r + 1] * g[1]) + rot[3 * r + 2] * g[2] for r in range(3)]
                l = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
                unit = (l > 0) & (l <= np.finfo(F).max)
                q = [np.where(unit, q[r] / l, F(0.0)).astype(F) for r in range(3)]
                if t["winding"] > 0:
                    q = [-x for x in q]
                if mode in (SHADE_SMOOTH, "smooth"):
                    col = [(q[r] + F(1.0)) * F(0.5) for r in range(3)]
                else:
                    lit = np.fmax(-q[2], F(0.0))
                    val = F(0.85) * lit
                    val = val + F(0.15)
                    col = [val, val, val]
            for ch in range(3):
                assert col[ch].dtype == F
                out[v, ch, jj, ii] = col[ch]
    return out


# ---- meshes --------------------------------------------------------------------------------------------------------------
TRIANGLE = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32))
TETRAHEDRON = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))
_QUAD = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.25], [0, 1, 0]], F)
TWO_TRIANGLES = (_QUAD, np.array([[0, 1, 2], [0, 2, 3]], np.int32))                # consistent winding over the shared edge
TWO_TRIANGLES_FLIPPED = (_QUAD, np.array([[0, 1, 2], [0, 3, 2]], np.int32))        # the second one the other way round
THREE_ON_AN_EDGE = (np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]], F), np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.int32))
TWICE = (TRIANGLE[0], np.array([[0, 1, 2], [0, 1, 2]], np.int32))
DEGENERATE = (TRIANGLE[0], np.array([[0, 0, 1]], np.int32))
OCTAHEDRON = (np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F),
              np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32))


def with_isolated(mesh, n=1):
    v, f = mesh
    return np.concatenate([v, np.full((n, 3), 7.0, F)]), f


def with_bad_face(mesh):
    v, f = mesh
    return v, np.concatenate([f, np.array([[0, 1, len(v)], [-1, 0, 1]], np.int32)])


def grid(nx, ny, noise=0.0, seed=0):
    """an open height field of nx x ny vertices, two triangles per cell, seeded noise on z"""
    jj, ii = np.mgrid[0:ny, 0:nx]
    z = np.random.default_rng(seed).normal(0.0, noise, size=(ny, nx)) if noise else np.zeros((ny, nx))
    v = np.stack([ii, jj, z], axis=-1).reshape(-1, 3).astype(F)
    q = (jj[:-1, :-1] * nx + ii[:-1, :-1]).reshape(-1)
    f = np.stack([np.stack([q, q + 1, q + nx + 1], axis=1), np.stack([q, q + nx + 1, q + nx], axis=1)], axis=1).reshape(-1, 3)
    return v, f.astype(np.int32)


def trimmed_grid(V, nf, seed=0):
    """exactly V vertices and nf triangles: a noisy square grid cut after nf triangles, then isolated vertices up to V"""
    m = int(np.ceil(np.sqrt(nf / 2.0))) + 1
    v, f = grid(m, m, 0.2, seed)
    assert len(v) <= V and len(f) >= nf
    pad = np.random.default_rng(seed + 1).normal(size=(V - len(v), 3)).astype(F)
    return np.concatenate([v, pad]), f[:nf]


def icosphere(level=3, noise=0.0, seed=0):
    """a closed unit sphere: the icosahedron subdivided `level` times (3: 642 vertices, 1280 triangles), outward winding, seeded
    radial noise"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    v = [np.asarray(p, D) / np.linalg.norm(p) for p in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    for _ in range(level):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    v = np.array(v)
    if noise:
        v = v * (1.0 + np.random.default_rng(seed).normal(0.0, noise, size=(len(v), 1)))
    return v.astype(F), np.array(f, np.int32)


def hub_fan(n=200):
    """n triangles around vertex 0: the hub has n + 1 neighbours (an open fan), so one lane walks a long list"""
    a = 2.0 * np.pi * np.arange(n + 1) / (n + 3)
    rim = np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(5 * a)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(F)
    f = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 2 + np.arange(n)], axis=1).astype(np.int32)
    return v, f


def radial_rms(v, centre=(0.0, 0.0, 0.0)):
    """(the RMS deviation of the vertices' distance to `centre` from its mean, that mean), fp64"""
    r = np.linalg.norm(np.asarray(v, D) - np.asarray(centre, D), axis=1)
    return float(np.sqrt(((r - r.mean()) ** 2).mean())), float(r.mean())
