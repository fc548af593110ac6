"""The arithmetic of csrc/meshtools.hip (ABI 18, include/b3gs_raster.h) restated in numpy and nothing else: connected
components, the cleaning step, the surface lattice, brute-force nearest distances and the score.  Float statements are one
float32 operation each, in the header's order, so the device agrees bit for bit; the means are numpy's fp64 means."""
import numpy as np

F = np.float32
MAX_LATTICE = 1 << 15


def components(V, faces):
    """-> (labels int32 [V], tri_count int32 [V]): label = the smallest vertex index of the component."""
    parent = np.arange(V, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
        for u, v in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    labels = np.array([find(v) for v in range(V)], dtype=np.int32)
    count = np.zeros(V, dtype=np.int32)
    if len(faces):
        np.add.at(count, labels[np.asarray(faces).reshape(-1, 3)[:, 0]], 1)
    return labels, count


def threshold(tri_count, keep_largest=0, min_triangles=0):
    thr = max(int(min_triangles), 1)
    if keep_largest > 0 and len(tri_count):
        thr = max(thr, int(np.sort(tri_count)[::-1][min(keep_largest, len(tri_count)) - 1]))
    return thr


def clean(vertices, colours, faces, keep_largest=0, min_triangles=0):
    vertices, colours, faces = np.asarray(vertices), np.asarray(colours), np.asarray(faces).reshape(-1, 3)
    labels, count = components(len(vertices), faces)
    keep = count[labels] >= threshold(count, keep_largest, min_triangles)
    newid = np.cumsum(keep) - 1
    kept_faces = faces[keep[faces[:, 0]]] if len(faces) else faces
    return vertices[keep], colours[keep], newid[kept_faces].astype(np.int32).reshape(-1, 3)


def _length(e):
    return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2], dtype=F)


def lattice(p0, p1, p2, spacing):
    """The lattice points of one triangle, float32 [n, 3], in (i, j) order."""
    p0, p1, p2, spacing = np.asarray(p0, F), np.asarray(p1, F), np.asarray(p2, F), F(spacing)
    e1, e2 = p1 - p0, p2 - p0
    n1, n2 = int(np.floor(_length(e1) / spacing)), int(np.floor(_length(e2) / spacing))
    assert n1 < MAX_LATTICE and n2 < MAX_LATTICE
    A, B = n1 + 1, n2 + 1
    out = []
    for i in range(A):
        s = F(i) / F(A)
        for j in range(B):
            if (i or j) and i * B + j * A < A * B:
                t = F(j) / F(B)
                out.append((p0 + s * e1) + t * e2)
    return np.array(out, dtype=F).reshape(-1, 3)


def sample_surface(vertices, faces, spacing):
    vertices = np.asarray(vertices, F)
    parts = [vertices.reshape(-1, 3)]
    for f in np.asarray(faces).reshape(-1, 3):
        parts.append(lattice(vertices[f[0]], vertices[f[1]], vertices[f[2]], spacing))
    return np.concatenate(parts, axis=0)


def nearest_distances(a, b, max_dist, chunk=512):
    """min(max_dist, sqrt(min_j d2)), d2 = (dx dx + dy dy) + dz dz in float32: brute force."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    out = np.empty(len(a), dtype=F)
    for s in range(0, len(a), chunk):
        d = a[s:s + chunk, None, :] - b[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        out[s:s + chunk] = np.minimum(F(max_dist), np.sqrt(d2.min(axis=1), dtype=F))
    return out


def score(d_recon, d_gt, tau, mask_recon=None, mask_gt=None):
    """The dict of mesh_tools.score_clouds from the two distance arrays (fp64 means of float32 distances)."""
    dr = np.asarray(d_recon, F)[slice(None) if mask_recon is None else np.asarray(mask_recon, bool)]
    dg = np.asarray(d_gt, F)[slice(None) if mask_gt is None else np.asarray(mask_gt, bool)]
    acc, comp = float(dr.astype(np.float64).mean()), float(dg.astype(np.float64).mean())
    ta, tc = int((dr < F(tau)).sum()), int((dg < F(tau)).sum())
    p, r = ta / len(dr), tc / len(dg)
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "precision": p, "recall": r,
            "fscore": 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0, "n_recon": len(dr), "n_gt": len(dg),
            "n_recon_below_tau": ta, "n_gt_below_tau": tc}
