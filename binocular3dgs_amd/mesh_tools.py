"""Cleaning, scoring and simplifying an extracted mesh, on the device (csrc/meshtools.hip, ABI 18, INTEGRATION.md section 13;
csrc/simplify.hip).

    labels, tri_count = components(vertices, faces)                      # int32 [V] each; no host read
    vertices, colours, faces = clean(vertices, colours, faces, keep_largest=1)
    points = sample_surface(vertices, faces, spacing)                    # the vertices, then a lattice per triangle
    d = nearest_distances(a, b, max_dist)                                # float32 [Na]: the float32 brute force, bit for bit
    score = score_clouds(recon, gt, max_dist, tau)                       # accuracy, completeness, chamfer, precision, recall, fscore
    score = score_mesh(vertices, faces, gt, spacing, max_dist, tau)
    vertices, colours, faces = simplify(vertices, colours, faces, cell, placement="quadric")     # vertex clustering
    vertices, colours, faces, cell = simplify_to(vertices, colours, faces, target_triangles)
    adj = adjacency(vertices, faces)                                     # the vertex adjacency, built once per set of faces
    vertices = smooth(vertices, faces, iterations=10, adjacency=adj)     # Taubin filter (csrc/meshsmooth.hip, section 17)
    normals = vertex_normals(vertices, faces, adjacency=adj)             # float32 [V, 3], area-weighted
    info = topology(vertices, faces, adjacency=adj)                      # edges, boundary, non-manifold, euler, closed

The arithmetic is stated in include/b3gs_raster.h and restated in numpy by tests/meshtools_ref.py, tests/simplify_ref.py and
tests/meshsmooth_ref.py.  Policy that is not hot
lives here in torch: the component threshold of `clean` (a topk of the triangle counts, kept on the device).

The score is the point-to-point measure of the DTU surface benchmark (distances both ways between points on the
reconstruction and a reference cloud).  DTU's own protocol -- thinning both clouds to 0.2 mm, the observation mask, the
ground plane -- stays with the caller, who owns those files: `mask_recon` / `mask_gt` are the hook.  Numbers computed here
without that protocol are not DTU numbers.
"""
from __future__ import annotations

from typing import Optional

import torch

MAX_LATTICE = 1 << 15      # n1, n2 of sample_surface stay below this


def _faces(faces) -> torch.Tensor:
    if faces.dtype != torch.int32:
        raise ValueError("faces are int32 [F, 3]")
    return faces


def components(vertices_or_V, faces: torch.Tensor):
    """-> (labels int32 [V], tri_count int32 [V]) on the device.  labels[v] is the smallest vertex index of v's component
    (two vertices are connected when one triangle names both); tri_count[r] is the number of triangles of the component whose
    label is r and 0 elsewhere.  The first argument is the vertex tensor or V itself.  No host read (capturable)."""
    from . import _C
    V = int(vertices_or_V) if isinstance(vertices_or_V, int) else int(vertices_or_V.shape[0])
    return _C.mesh_components(V, _faces(faces))


def component_threshold(tri_count: torch.Tensor, keep_largest: int = 0, min_triangles: int = 0) -> torch.Tensor:
    """One int32 on the device: max(min_triangles, 1, c_k), c_k the triangle count of the keep_largest-th largest component
    (ties at c_k all survive; keep_largest = 0: no such bound).  No host read."""
    if keep_largest < 0 or min_triangles < 0:
        raise ValueError("keep_largest and min_triangles are not negative")
    thr = torch.full((1,), max(int(min_triangles), 1), dtype=torch.int32, device=tri_count.device)
    if keep_largest > 0 and tri_count.numel() > 0:
        k = min(int(keep_largest), tri_count.numel())
        thr = torch.maximum(thr, torch.topk(tri_count, k).values[k - 1:k])
    return thr


def clean(vertices: torch.Tensor, colours: torch.Tensor, faces: torch.Tensor, keep_largest: int = 0, min_triangles: int = 0,
          return_stats: bool = False):
    """Keeps the components with at least max(min_triangles, 1, c_k) triangles and drops the vertices no kept triangle names
    -> (vertices, colours, faces), order and winding preserved.  One host read: the totals, between count and emit."""
    from . import _C
    labels, tri_count = components(vertices, faces)
    thr = component_threshold(tri_count, keep_largest, min_triangles)
    ws, totals = _C.mesh_clean_count(faces, labels, tri_count, thr)
    if return_stats:                                   # (one read still: the statistics ride along with the totals)
        ncomp = ((tri_count > 0).sum()).reshape(1)
        kept = ((tri_count >= thr) & (tri_count > 0)).sum().reshape(1)
        nverts, ntris, bad, ncomp, kept = torch.cat([totals, ncomp, kept]).tolist()
    else:
        nverts, ntris, bad = totals.tolist()
    if bad:
        raise ValueError(f"clean: {bad} triangles name a vertex outside 0 .. {vertices.shape[0] - 1}")
    out = _C.mesh_clean_emit(vertices, colours, faces, labels, tri_count, thr, ws, nverts, ntris)
    if return_stats:
        return out + ({"components": ncomp, "kept": kept, "vertices_dropped": vertices.shape[0] - nverts,
                       "triangles_dropped": faces.shape[0] - ntris},)
    return out


def sample_surface(vertices: torch.Tensor, faces: torch.Tensor, spacing: float) -> torch.Tensor:
    """float32 [N, 3]: the V vertices in order, then per triangle (p0, p1, p2) the lattice p0 + i/(n1+1) e1 + j/(n2+1) e2,
    n = floor(|e| / spacing), inside the triangle and off its far edge, in (triangle, i, j) order.  Errors, not clamps:
    spacing <= 0, an n at or above 2^15, more than 2^31 - 1 points.  One host read: the total (and the error counts)."""
    from . import _C
    if not spacing > 0.0:
        raise ValueError("sample_surface: the spacing is positive")
    ws, totals = _C.mesh_sample_count(vertices, _faces(faces), float(spacing))
    npoints, over, bad = totals.tolist()
    if bad:
        raise ValueError(f"sample_surface: {bad} triangles name a vertex outside 0 .. {vertices.shape[0] - 1}")
    if over:
        raise ValueError(f"sample_surface: {over} triangles have an edge of {MAX_LATTICE} spacings or more (or not finite): use a larger spacing")
    if vertices.shape[0] + npoints > 2 ** 31 - 1:
        raise ValueError(f"sample_surface: {vertices.shape[0] + npoints} points do not fit int32: use a larger spacing")
    return _C.mesh_sample_emit(vertices, faces, float(spacing), ws, npoints)


class NearestGrid:
    """The search grid over a cloud `b` (float32 [Nb, 3], Nb >= 1) for distances up to max_dist; query(a) -> float32 [Na].
    Built and queried without a host read.  params() reads the grid the device chose (a diagnostic: one host read)."""

    def __init__(self, b: torch.Tensor, max_dist: float):
        from . import _C
        if b.shape[0] < 1:
            raise ValueError("nearest_distances: the cloud searched is empty")
        self.nb, self.max_dist = int(b.shape[0]), float(max_dist)
        self._ws = _C.nearest_grid(b, self.max_dist)

    def query(self, a: torch.Tensor) -> torch.Tensor:
        from . import _C
        return _C.nearest_query(a, self._ws, self.nb, self.max_dist)

    def query_index(self, a: torch.Tensor):
        """-> (distances float32 [Na], index int32 [Na]): the nearest point of `b` as well, among equal squared distances the
        smallest index, -1 where nothing lies within max_dist (edit.register pairs points with it)."""
        from . import _C
        return _C.nearest_query_index(a, self._ws, self.nb, self.max_dist)

    def params(self) -> dict:
        head = self._ws[:32].cpu()
        f, i = head.view(torch.float32), head.view(torch.int32)
        return {"origin": f[:3].tolist(), "cell": float(f[3]), "dims": i[4:7].tolist(), "shells": int(i[7])}


def nearest_distances(a: torch.Tensor, b: torch.Tensor, max_dist: float) -> torch.Tensor:
    """out[i] = min(max_dist, sqrt(min_j |a_i - b_j|^2)) in float32, equal to the brute force bit for bit.  An empty `b` is an
    error.  No host read."""
    return NearestGrid(b, max_dist).query(a)


def _mask(mask, n, device):
    if mask is None:
        return None
    if mask.dtype != torch.bool or mask.shape != (n,):
        raise ValueError("a mask is a bool tensor with one value per point")
    return mask.to(device)


def score_clouds(recon: torch.Tensor, gt: torch.Tensor, max_dist: float, tau: float, mask_recon: Optional[torch.Tensor] = None,
                 mask_gt: Optional[torch.Tensor] = None, return_distances: bool = False) -> dict:
    """accuracy = mean distance recon -> gt, completeness = mean distance gt -> recon (each capped at max_dist), chamfer their
    mean; precision / recall = the share of recon / gt distances below tau, fscore their harmonic mean (0 when both are 0).
    A mask drops points from the means, never from the cloud being searched.  One host read: six fp64 words."""
    from . import _C
    if recon.shape[0] < 1 or gt.shape[0] < 1:
        raise ValueError("score_clouds: both clouds hold at least one point")
    d_recon = nearest_distances(recon, gt, max_dist)
    d_gt = nearest_distances(gt, recon, max_dist)
    sums = torch.empty((2, 3), dtype=torch.float64, device=recon.device)
    _C.cloud_score(d_recon, _mask(mask_recon, recon.shape[0], recon.device), float(tau), sums[0])
    _C.cloud_score(d_gt, _mask(mask_gt, gt.shape[0], gt.device), float(tau), sums[1])
    (sa, na, ta), (sc, nc, tc) = sums.tolist()                    # the one host read
    if na == 0 or nc == 0:
        raise ValueError("score_clouds: a mask leaves no point")
    p, r = ta / na, tc / nc
    out = {"accuracy": sa / na, "completeness": sc / nc, "chamfer": 0.5 * (sa / na + sc / nc), "precision": p, "recall": r,
           "fscore": 2.0 * p * r / (p + r) if p + r > 0.0 else 0.0, "n_recon": int(na), "n_gt": int(nc),
           "n_recon_below_tau": int(ta), "n_gt_below_tau": int(tc), "max_dist": float(max_dist), "tau": float(tau)}
    if return_distances:
        out["d_recon"], out["d_gt"] = d_recon, d_gt
    return out


def score_mesh(vertices: torch.Tensor, faces: torch.Tensor, gt: torch.Tensor, spacing: float, max_dist: float, tau: float,
               mask_gt: Optional[torch.Tensor] = None, return_distances: bool = False) -> dict:
    """sample_surface(vertices, faces, spacing), then score_clouds against gt."""
    return score_clouds(sample_surface(vertices, faces, spacing), gt, max_dist, tau, None, mask_gt, return_distances)


# ---- simplification: vertex clustering with quadric-optimal representatives (csrc/simplify.hip) -------------------------------
PLACEMENTS = {"quadric": 0, "mean": 1}     # B3GS_SIMPLIFY_QUADRIC / _MEAN
MAX_CELLS = 1024                           # cells per axis of the clustering grid
MAX_TRIALS = 12                            # count-only trials of simplify_to


def smallest_cell(extent: float) -> float:
    """The smallest float32 `cell` with floor(extent / cell) <= 1023 in float32, i.e. at most 1024 cells along an edge of
    length `extent` that starts at the grid's origin."""
    import numpy as np
    e = np.float32(extent)
    c = np.float32(e / np.float32(MAX_CELLS))
    while c > 0 and np.floor(e / np.nextafter(c, np.float32(0))) < MAX_CELLS:
        c = np.nextafter(c, np.float32(0))
    while not (c > 0 and np.floor(e / c) < MAX_CELLS):
        c = np.nextafter(c, np.float32(np.inf))
    return float(c)


def _extent_of(word: int) -> float:
    import struct
    return struct.unpack("<f", struct.pack("<I", int(word) & 0xFFFFFFFF))[0]


def _simplify_count(vertices, faces, cell, what):
    """count, the ONE host read, and the errors that ride on it -> (workspace, the nine totals)"""
    from . import _C
    ws, totals = _C.mesh_simplify_count(vertices, _faces(faces), float(cell))
    t = totals.tolist()                                                   # the one host read
    bad, nonfinite, over = t[2], t[3], t[4]
    if bad:
        raise ValueError(f"{what}: {bad} triangles name a vertex outside 0 .. {vertices.shape[0] - 1}")
    if nonfinite:
        raise ValueError(f"{what}: {nonfinite} vertices have a coordinate that is not finite")
    if over:
        raise ValueError(f"{what}: {over} vertices lie beyond {MAX_CELLS} cells of {float(cell):g} along an axis: "
                         f"the smallest admissible cell is {smallest_cell(_extent_of(t[8]))!r}")
    return ws, t


def simplify(vertices: torch.Tensor, colours: torch.Tensor, faces: torch.Tensor, cell: float, placement: str = "quadric",
             return_stats: bool = False):
    """Vertex clustering on a grid of edge `cell` (world units) whose origin is the lower corner of the vertices' box: every
    cluster that a surviving triangle names becomes one vertex, at the minimiser of its faces' quadric ("quadric": pulled to
    the planes of the faces that touch the cluster, never further than `cell` from the mean) or at the mean of its members
    ("mean"); a triangle with two corners in one cluster is dropped, and of the triangles that name the same three clusters
    the first stays -> (vertices, colours, faces), triangles in input order with their winding.  Errors, not clamps: more
    than 1024 cells along an axis, a coordinate that is not finite, a face index outside 0 .. V-1.  One host read: the totals
    (and the error counts and statistics), between count and emit."""
    from . import _C
    if placement not in PLACEMENTS:
        raise ValueError(f"simplify: placement is one of {sorted(PLACEMENTS)}")
    if not cell > 0.0:
        raise ValueError("simplify: the cell is positive")
    ws, t = _simplify_count(vertices, faces, cell, "simplify")
    out = _C.mesh_simplify_emit(vertices, colours, faces, float(cell), PLACEMENTS[placement], ws, t[0], t[1])
    if return_stats:
        return out + ({"clusters": t[5], "vertices_dropped": vertices.shape[0] - t[0], "triangles_degenerate": t[6],
                       "triangles_duplicate": t[7]},)
    return out


def bisect_cell(count_triangles, extent: float, target_triangles: int, trials: int = MAX_TRIALS):
    """The search of simplify_to as host logic over `count_triangles(cell) -> int`: geometric bisection of the cell between
    the smallest admissible one (extent / 1024) and `extent`, at most `trials` calls -> (the smallest tried cell whose count
    is at most the target, its count).  ValueError when even `extent` leaves more than the target."""
    lo = smallest_cell(extent)
    n = count_triangles(lo)
    if n <= target_triangles:
        return lo, n
    hi = float(extent)
    best = count_triangles(hi)
    if best > target_triangles:
        raise ValueError(f"simplify_to: a cell of the whole extent ({hi:g}) still leaves {best} triangles")
    for _ in range(trials - 2):
        mid = (lo * hi) ** 0.5
        if not lo < mid < hi:
            break
        n = count_triangles(mid)
        if n <= target_triangles:
            hi, best = mid, n
        else:
            lo = mid
    return hi, best


def simplify_to(vertices: torch.Tensor, colours: torch.Tensor, faces: torch.Tensor, target_triangles: int, placement: str = "quadric"):
    """simplify() at the smallest cell, of at most 12 tried by geometric bisection between extent / 1024 and extent (the
    longest edge of the vertices' box), that leaves at most `target_triangles` triangles -> (vertices, colours, faces, cell).
    Host reads: the extent, one per count-only trial, and the one of the final simplify()."""
    if target_triangles < 1:
        raise ValueError("simplify_to: target_triangles is at least 1")
    if placement not in PLACEMENTS:
        raise ValueError(f"simplify_to: placement is one of {sorted(PLACEMENTS)}")
    if vertices.shape[0] == 0 or faces.shape[0] == 0:
        raise ValueError("simplify_to: the mesh is empty")
    extent = float((vertices.amax(dim=0) - vertices.amin(dim=0)).max())
    if not (extent > 0.0 and extent < float("inf")):
        raise ValueError("simplify_to: the vertices span no finite, positive extent")
    cell, _ = bisect_cell(lambda c: _simplify_count(vertices, faces, c, "simplify_to")[1][1], extent, int(target_triangles))
    return simplify(vertices, colours, faces, cell, placement) + (cell,)


# ---- smoothing: vertex adjacency, Taubin filter, vertex normals (csrc/meshsmooth.hip) -----------------------------------------
TOTALS = ("bad_faces", "nonfinite_vertices", "edges", "boundary_edges", "non_manifold_edges", "pinned_vertices", "isolated_vertices",
          "good_faces")     # the eight int64 words at the head of the adjacency workspace, in order


def _check_smooth_mesh(vertices, faces, what):
    if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices are float32 [V, 3]")
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces are int32 [F, 3]")
    if vertices.shape[0] > 2 ** 31 - 1 or 6 * faces.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"{what}: V <= 2^31 - 1 and 6 F <= 2^31 - 1")


class Adjacency:
    """The built adjacency workspace of one mesh (opaque; reusable while the faces are unchanged): per vertex its neighbours in
    ascending order and its faces in face-index order, the edge classes and the totals, all on the device.  `totals` is the
    int64 [8] device view of TOTALS; lists() gives views of the lists (what the tests compare).  Nothing here reads the device
    except check()."""

    def __init__(self, vertices: torch.Tensor, faces: torch.Tensor):
        from . import _C
        _check_smooth_mesh(vertices, faces, "adjacency")
        self.V, self.F = int(vertices.shape[0]), int(faces.shape[0])
        self.workspace = _C.mesh_adjacency_build(vertices, faces)
        self.totals = _C.mesh_adjacency_views(self.workspace, self.V, self.F)[0]

    def lists(self) -> dict:
        """Device views: neighbour_offsets int32 [V + 1], neighbour_indices int32 [6 F] (the first offsets[V] are meaningful),
        incidence_ranges int32 [V, 2], incident_faces int32 [3 F], pinned uint8 [V]."""
        from . import _C
        _, off, idx, rng, inc, pinned = _C.mesh_adjacency_views(self.workspace, self.V, self.F)
        return {"neighbour_offsets": off, "neighbour_indices": idx, "incidence_ranges": rng, "incident_faces": inc, "pinned": pinned}

    def matches(self, vertices, faces) -> bool:
        return self.V == int(vertices.shape[0]) and self.F == int(faces.shape[0]) and self.workspace.device == vertices.device

    def check(self, what: str) -> list:
        """The ONE host read: the totals -> the list, ValueError for bad faces or vertices that are not finite."""
        t = self.totals.tolist()
        if t[0]:
            raise ValueError(f"{what}: {t[0]} triangles name a vertex outside 0 .. {self.V - 1}")
        if t[1]:
            raise ValueError(f"{what}: {t[1]} vertices have a coordinate that is not finite")
        return t


def adjacency(vertices: torch.Tensor, faces: torch.Tensor) -> Adjacency:
    """Builds the vertex adjacency of the mesh on the device -> an opaque holder that smooth, vertex_normals and topology take.
    No host read (capturable)."""
    return Adjacency(vertices, faces)


def _adjacency_for(vertices, faces, adj, what) -> Adjacency:
    _check_smooth_mesh(vertices, faces, what)
    if adj is None:
        return Adjacency(vertices, faces)
    if not isinstance(adj, Adjacency) or not adj.matches(vertices, faces):
        raise ValueError(f"{what}: the adjacency was built for another mesh ({getattr(adj, 'V', '?')} vertices, {getattr(adj, 'F', '?')} triangles)")
    return adj


def smooth(vertices: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, pin_boundary: bool = True,
           adjacency: Optional[Adjacency] = None, *, check: bool = True) -> torch.Tensor:
    """Taubin's filter: `iterations` pairs of Jacobi steps x_i += k (mean of the neighbours - x_i), k = lam then k = mu (mu < -lam,
    which keeps the volume; mu = 0 is the plain Laplacian filter of `iterations` steps, which shrinks) -> float32 [V, 3];
    colours and faces are the caller's and unchanged.  pin_boundary keeps the ends of boundary and non-manifold edges where they
    are.  Neighbour sums are fp64 in ascending neighbour order, without atomics: one fixed result.  Errors, not clamps: a face
    index outside 0 .. V-1, a coordinate that is not finite (one host read, after the kernels have run; check=False skips it,
    e.g. under graph capture, and leaves the counts in adjacency.totals)."""
    from . import _C
    if iterations < 0:
        raise ValueError("smooth: iterations is not negative")
    if not (0.0 < lam <= 1.0):
        raise ValueError("smooth: lam is in (0, 1]")
    if mu > 0.0 or mu != mu:
        raise ValueError("smooth: mu is not positive")
    if mu != 0.0 and mu >= -lam:
        raise ValueError("smooth: Taubin's condition is mu < -lam (or mu = 0 for the Laplacian filter)")
    adj = _adjacency_for(vertices, faces, adjacency, "smooth")
    out = _C.mesh_smooth(vertices, adj.F, adj.workspace, int(iterations), float(lam), float(mu), bool(pin_boundary))
    if check:
        adj.check("smooth")
    return out


def vertex_normals(vertices: torch.Tensor, faces: torch.Tensor, adjacency: Optional[Adjacency] = None, *, check: bool = True) -> torch.Tensor:
    """float32 [V, 3]: per vertex the unit sum of its faces' normals (p1 - p0) x (p2 - p0), i.e. area-weighted, summed in fp64 in
    face-index order; (0, 0, 0) for a vertex without faces or with a sum of length 0.  check: as for smooth."""
    from . import _C
    adj = _adjacency_for(vertices, faces, adjacency, "vertex_normals")
    out = _C.mesh_vertex_normals(vertices, faces, adj.workspace)
    if check:
        adj.check("vertex_normals")
    return out


def topology(vertices: torch.Tensor, faces: torch.Tensor, adjacency: Optional[Adjacency] = None) -> dict:
    """The totals of the adjacency (TOTALS) and euler = (V - isolated) - E + good faces, closed = no boundary and no non-manifold
    edge.  One host read.  nonfinite_vertices describes the vertices of the latest call that used the adjacency."""
    adj = _adjacency_for(vertices, faces, adjacency, "topology")
    t = adj.totals.tolist()                                               # the one host read
    out = dict(zip(TOTALS, t))
    out["vertices"], out["triangles"] = adj.V, adj.F
    out["euler"] = (adj.V - out["isolated_vertices"]) - out["edges"] + out["good_faces"]
    out["closed"] = out["boundary_edges"] == 0 and out["non_manifold_edges"] == 0
    return out


def topology_line(info: dict) -> str:
    """The line the command lines print for topology()"""
    return (f"topology: {info['vertices']} vertices ({info['isolated_vertices']} isolated), {info['edges']} edges ({info['boundary_edges']} boundary, "
            f"{info['non_manifold_edges']} non-manifold), {info['good_faces']} triangles, euler {info['euler']}, {'closed' if info['closed'] else 'open'}")
