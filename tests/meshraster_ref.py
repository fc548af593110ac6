"""The numpy yardstick of the mesh rasterizer (csrc/meshraster.hip): a restatement of the statements 1-5 and 7 of the section
"rendering an extracted mesh" of include/b3gs_raster.h.  int64 for the edge functions, np.float32 statement by statement,
one fp64 division per barycentric weight; vectorised per triangle over its clamped box.  It also builds the test meshes."""
import numpy as np

F = np.float32
NEAR = F(0.2)
GUARD = 1 << 22
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
SMALL_BOX, WAVE_BOX = 32, 4096


def camera_space(vertices, cam):
    """statement 1, first line -> float32 [V, 3]"""
    c = np.asarray(cam, dtype=F)
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((c[3 * r] * x + c[3 * r + 1] * y) + c[3 * r + 2] * z) + c[9 + r] for r in range(3)], axis=1).astype(F)


def project(vertices, cam, W, H):
    """statements 1 and 2 per vertex -> (X int64 [V], Y int64 [V], pz float32 [V], good bool [V], sx, sy float32)"""
    c = np.asarray(cam, dtype=F)
    p = camera_space(vertices, c)
    with np.errstate(all="ignore"):
        sx = c[12] * (p[:, 0] / p[:, 2]) + (F(0.5) * F(W) - F(0.5))
        sy = c[13] * (p[:, 1] / p[:, 2]) + (F(0.5) * F(H) - F(0.5))
        rx, ry = np.rint(sx * F(256.0)), np.rint(sy * F(256.0))
        good = (p[:, 2] > NEAR) & (p[:, 2] <= np.finfo(F).max) & (np.abs(rx) < F(GUARD)) & (np.abs(ry) < F(GUARD))
    X = np.where(good, rx, 0).astype(np.int64)
    Y = np.where(good, ry, 0).astype(np.int64)
    assert sx.dtype == F and rx.dtype == F
    return X, Y, p[:, 2], good, sx, sy


def setup(X, Y, W, H):
    """statement 3 for one triangle (X, Y: three python ints each) -> None for zero area, else a dict"""
    area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if area == 0:
        return None
    s = 1 if area > 0 else -1
    edges = []
    for k in range(3):
        p, q = (k + 1) % 3, (k + 2) % 3
        dx, dy = s * (X[q] - X[p]), s * (Y[q] - Y[p])
        edges.append((dx, dy, X[p], Y[p], 0 if (dy < 0 or (dy == 0 and dx > 0)) else 1))
    x0, x1 = max(-(-min(X) // 256), 0), min(max(X) // 256, W - 1)
    y0, y1 = max(-(-min(Y) // 256), 0), min(max(Y) // 256, H - 1)
    return {"A": s * area, "winding": s, "edges": edges, "box": (x0, y0, x1, y1)}


def box_pixels(t):
    x0, y0, x1, y1 = t["box"]
    return max(x1 - x0 + 1, 0) * max(y1 - y0 + 1, 0)


def edge_values(t, i, j):
    """E_k at the pixel centres (i, j): int64 arrays -> [3, ...] int64 and the coverage mask"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    E = np.stack([np.int64(dx) * (256 * j - np.int64(yp)) - np.int64(dy) * (256 * i - np.int64(xp)) for dx, dy, xp, yp, _ in t["edges"]])
    inside = np.ones(E.shape[1:], dtype=bool)
    for k, e in enumerate(t["edges"]):
        inside &= E[k] >= e[4]
    return E, inside


def depth_of(t, E, pz):
    """statement 4 -> (w float32 [3, ...], z float32)"""
    with np.errstate(all="ignore"):
        w = [(E[k].astype(np.float64) / np.float64(t["A"])).astype(F) * (F(1.0) / F(pz[k])) for k in range(3)]
        iz = (w[0] + w[1]) + w[2]
        z = F(1.0) / iz
    assert z.dtype == F
    return w, z


def render(vertices, colours, faces, cams, W, H, bg=(0.0, 0.0, 0.0), shading="colour", cull_backface=False, face_pixels=None):
    """-> {"triangle_id" int32 [n,H,W], "depth", "alpha" float32 [n,1,H,W], "colour" float32 [n,3,H,W], "rejected" int32 [n],
    "bad" int, "face_pixels" int32 [F] (added to `face_pixels` when given)}.  shading "both": "colour" holds the vertex
    colours and "normal" the normal map (one pass over the triangles for the two)."""
    vertices = np.asarray(vertices, dtype=F).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cams = np.asarray(cams, dtype=F).reshape(-1, 14)
    n, V, nf = len(cams), len(vertices), len(faces)
    fp = np.zeros(nf, dtype=np.int32) if face_pixels is None else np.array(face_pixels, dtype=np.int32)
    valid = ((faces >= 0) & (faces < V)).all(axis=1)
    out = {"triangle_id": np.full((n, H, W), -1, np.int32), "depth": np.zeros((n, 1, H, W), F), "alpha": np.zeros((n, 1, H, W), F),
           "colour": np.empty((n, 3, H, W), F), "rejected": np.zeros(n, np.int32), "bad": int((~valid).sum())}
    out["colour"][:] = np.asarray(bg, dtype=F).reshape(1, 3, 1, 1)
    if shading == "both":
        out["normal"] = out["colour"].copy()
    normal_to = out.get("normal", out["colour"])
    for v in range(n):
        X, Y, pz, good, _, _ = project(vertices, cams[v], W, H)
        vis = np.full((H, W), EMPTY, dtype=np.uint64)
        tris = {}
        for f in range(nf):
            if not valid[f] or not good[faces[f]].all():
                out["rejected"][v] += 1
                continue
            a, b, c = (int(q) for q in faces[f])
            t = setup([int(X[a]), int(X[b]), int(X[c])], [int(Y[a]), int(Y[b]), int(Y[c])], W, H)
            if t is None or (cull_backface and t["winding"] > 0) or box_pixels(t) == 0:
                continue
            tris[f] = t
            x0, y0, x1, y1 = t["box"]
            jj, ii = np.mgrid[y0:y1 + 1, x0:x1 + 1]
            E, inside = edge_values(t, ii, jj)
            _, z = depth_of(t, E, pz[[a, b, c]])
            word = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
            sub = vis[y0:y1 + 1, x0:x1 + 1]
            sub[...] = np.where(inside, np.minimum(sub, word), sub)
        pc = camera_space(vertices, cams[v]) if shading != "colour" else None
        for f in np.unique((vis[vis != EMPTY] & np.uint64(0xFFFFFFFF)).astype(np.int64)):
            t = tris[int(f)]
            jj, ii = np.nonzero((vis != EMPTY) & ((vis & np.uint64(0xFFFFFFFF)) == np.uint64(f)))
            E, inside = edge_values(t, ii, jj)
            assert inside.all()
            idx = faces[f]
            w, z = depth_of(t, E, pz[idx])
            assert np.array_equal(z.view(np.uint32), (vis[jj, ii] >> np.uint64(32)).astype(np.uint32))
            out["triangle_id"][v, jj, ii] = f
            out["depth"][v, 0, jj, ii] = z
            out["alpha"][v, 0, jj, ii] = 1.0
            fp[f] += len(ii)
            if shading != "normal":
                col = np.asarray(colours, dtype=np.uint8)[idx].astype(F)
                for ch in range(3):
                    s = (w[0] * col[0, ch] + w[1] * col[1, ch]) + w[2] * col[2, ch]
                    out["colour"][v, ch, jj, ii] = (s * z) / F(255.0)
            if shading != "colour":
                normal_to[v, :, jj, ii] = face_normal_colour(pc[idx], t["winding"])[None, :]
    out["face_pixels"] = fp
    return out


def face_normal_colour(p, winding):
    """statement 7, B3GS_MESH_SHADE_NORMAL: p float32 [3, 3] camera-space corners -> float32 [3]"""
    with np.errstate(all="ignore"):
        u, v = p[1] - p[0], p[2] - p[0]
        n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=F)
        l = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        q = n / l if (l > 0 and np.isfinite(l)) else np.zeros(3, F)
        if winding > 0:
            q = -q
        out = (q + F(1.0)) * F(0.5)
    assert out.dtype == F
    return out


# ---- cameras and meshes --------------------------------------------------------------------------------------------------
def camera_row(R=None, t=None, fx=16.0, fy=16.0):
    row = np.zeros(14, F)
    row[:9] = np.eye(3).reshape(9) if R is None else np.asarray(R, dtype=np.float64).reshape(9)
    row[9:12] = 0.0 if t is None else np.asarray(t)
    row[12], row[13] = fx, fy
    return row


def orbit_cameras(n, centre, radius, fx, fy=None, height=0.0):
    """n cameras on a circle about the y axis through `centre`, looking at it (x right, y down, z forward)"""
    rows = []
    centre = np.asarray(centre, dtype=np.float64)
    for k in range(n):
        a = 2.0 * np.pi * k / n + 0.3
        eye = centre + np.array([radius * np.sin(a), height, -radius * np.cos(a)])
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(np.array([0.0, 1.0, 0.0]), fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        rows.append(camera_row(R, -R @ eye, fx, fx if fy is None else fy))
    return np.stack(rows)


def at_pixels(pix, z, W, H, fx=16.0, fy=16.0):
    """Vertices that the identity camera (camera_row()) projects to the screen positions `pix` ([n, 2], in pixels) at depth z:
    exact whenever fx, fy and z are powers of two and the positions multiples of 1/256."""
    pix = np.asarray(pix, dtype=np.float64).reshape(-1, 2)
    z = np.broadcast_to(np.asarray(z, dtype=np.float64), (len(pix),))
    x = (pix[:, 0] - (0.5 * W - 0.5)) / fx * z
    y = (pix[:, 1] - (0.5 * H - 0.5)) / fy * z
    return np.stack([x, y, z], axis=1).astype(F)


def grey(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3)).astype(np.uint8)


def random_mesh(nf, W, H, seed, zlo=1.0, zhi=4.0, span=6.0):
    """nf triangles of a few pixels each, scattered over (and a little beyond) the image of the identity camera"""
    rng = np.random.default_rng(seed)
    c = rng.uniform([-3.0, -3.0], [W + 3.0, H + 3.0], size=(nf, 1, 2))
    pix = c + rng.uniform(-span, span, size=(nf, 3, 2))
    z = rng.uniform(zlo, zhi, size=(nf, 3))
    v = at_pixels(pix.reshape(-1, 2), z.reshape(-1), W, H)
    return v, grey(len(v), seed), np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)


def uv_sphere(centre, radius, nu=12, nv=8, outward=True):
    """A closed sphere, wound so that (p1 - p0) x (p2 - p0) points outward (or inward)"""
    centre = np.asarray(centre, dtype=np.float64)
    verts = [centre + [0.0, -radius, 0.0]]
    for j in range(1, nv):
        th = np.pi * j / nv
        for i in range(nu):
            ph = 2.0 * np.pi * i / nu
            verts.append(centre + radius * np.array([np.sin(th) * np.cos(ph), -np.cos(th), np.sin(th) * np.sin(ph)]))
    verts.append(centre + [0.0, radius, 0.0])
    verts = np.array(verts)
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu
    faces = []
    for i in range(nu):
        faces.append([0, ring(1, i), ring(1, i + 1)])
        faces.append([len(verts) - 1, ring(nv - 1, i + 1), ring(nv - 1, i)])
        for j in range(1, nv - 1):
            faces.append([ring(j, i), ring(j + 1, i), ring(j + 1, i + 1)])
            faces.append([ring(j, i), ring(j + 1, i + 1), ring(j, i + 1)])
    faces = np.array(faces, dtype=np.int32)
    p = verts[faces]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    flip = ((nrm * (p.mean(axis=1) - centre)).sum(axis=1) > 0) != outward
    faces[flip] = faces[flip][:, [0, 2, 1]]
    return verts.astype(F), faces
