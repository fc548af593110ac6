"""A numpy restatement of csrc/knn.hip (b3gs_knn_mean_dist2), written from the kernel's header comment: the mean squared
distance of every point to its 3 nearest other points.

  * mean_dist2_exact   float64 brute force over the full P x P matrix, exclusion by index;
  * mean_dist2_f32     the same selection in the kernel's float32 arithmetic.  The library is built with -ffp-contract=off, so
                       every operation has one rounding and a fixed order, and the kernel must return these bits;
  * scene_box, morton_codes, boxes: the intermediates the kernel leaves in its workspace (codes, sorted points, box bounds);
  * scheme             the kernel's whole pruning scheme (Morton order, boxes of 1024, a bound from the +-3 Morton neighbours,
                       the box sweep), which must select the same VALUES as brute force;
  * variants           deliberately wrong restatements: tests/test_knn_ref_cpu.py shows that the clouds below tell each of
                       them from the right one.

The kernel keeps a candidate only `if (best[j] > d)` with best = FLT_MAX at the start, so a distance that is not below
FLT_MAX (NaN, inf) is never kept: a non-finite point is nobody's neighbour, and a point with fewer than three candidates
keeps FLT_MAX terms, whose float32 sum overflows to inf (one term: FLT_MAX / 3).  Selecting values, not indices, makes
ties harmless.  fminf / fmaxf ignore a NaN operand: np.fmin / np.fmax."""
import zlib

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
BOX = 1024                       # knn.hip::KNN_BOX
_PAIRS = 1 << 18                 # distance-matrix entries per block of rows (blocks that stay in the cache)

SIZES = (1, 2, 3, 4, 5, 8, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)
LARGE = 70000                    # above 65536: the scene-box partial kernel is capped at 256 workgroups and strides
SHAPES = ("lattice", "lattice_tenth", "far", "negative", "line", "point", "twins", "clusters", "nonfinite", "seam")
NONFINITE_ROWS = (0, 1024, 2048)
CLOUDS = tuple("uniform_%d" % p for p in SIZES) + ("uniform_%d" % LARGE,) + SHAPES


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def cloud(name):
    """float32 [P, 3], the same bits on every call."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name.startswith("uniform_"):
        return rng.uniform(-3, 5, size=(int(name[8:]), 3)).astype(np.float32)
    if name in ("lattice", "lattice_tenth"):          # 13^3 = 2197 points in shuffled order: ties on every face distance
        g = np.arange(13, dtype=np.float32) - 4
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(13 ** 3)]
        return pts if name == "lattice" else pts * np.float32(0.1)
    if name == "far":                                 # the origin-seeded scene box squeezes it into a few Morton cells
        return rng.uniform(100, 101, size=(2049, 3)).astype(np.float32)
    if name == "negative":
        return rng.uniform(-9, -8, size=(2049, 3)).astype(np.float32)
    if name == "line":                                # only x varies; y has zero extent, z one value off the origin
        pts = np.zeros((2049, 3), np.float32)
        pts[:, 0] = rng.uniform(-3, 5, size=2049).astype(np.float32)
        pts[:, 2] = 0.75
        return pts
    if name == "point":                               # y has zero extent, x sits on the box maximum, z on the minimum
        return np.tile(np.array([[1.25, 0.0, -2.0]], np.float32), (1500, 1))
    if name == "twins":                               # every point twice: the twin is excluded by index only
        half = rng.uniform(-3, 5, size=(1024, 3)).astype(np.float32)
        return np.concatenate([half, half])[rng.permutation(2048)]
    if name == "clusters":                            # 1024-point box seams fall inside clusters
        return (rng.uniform(0, 0.03, size=(4096, 3)) + 7.0 * rng.integers(0, 4, size=(4096, 1))).astype(np.float32)
    if name == "nonfinite":
        pts = rng.uniform(-3, 5, size=(2049, 3)).astype(np.float32)
        for axis, (row, v) in enumerate(zip(NONFINITE_ROWS, (np.nan, np.inf, -np.inf))):
            pts[row, axis] = v
        return pts
    if name == "seam":
        # integers on the x axis in index order, x = 1024 left out.  Morton order is index order (equal codes keep it), so
        # box 0 ends at x = 1023 and box 1 begins at x = 1025: for the point at 1023 (neighbours at 1, 4, 4) the bound from
        # its Morton neighbours is 4 and the nearest face of box 1 is exactly 4 away, and the same mirrored for 1025.
        x = np.arange(2049, dtype=np.float32)
        pts = np.zeros((2048, 3), np.float32)
        pts[:, 0] = x[x != 1024]
        return pts
    raise KeyError(name)


# ---- brute force ----------------------------------------------------------------------------------------------------------
def _dist2(a, x):
    """[n, m]: squared distance of every `x` [n, 3] to every `a` [m, 3] in the arithmetic of their type, as
    knn.hip::dist2 has it: differences a - x per axis, (dx*dx + dy*dy) + dz*dz."""
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = (a[None, :, k] - x[:, None, k] for k in range(3))
        return (dx * dx + dy * dy) + dz * dz


def _smallest(d, k, missing):
    """The k smallest entries of every row of d in ascending order; an entry that is not below `missing` counts as
    `missing`, and so do the entries a row of fewer than k lacks."""
    d = np.where(d < missing, d, missing)
    if d.shape[1] < k:
        d = np.concatenate([d, np.full((d.shape[0], k - d.shape[1]), missing, d.dtype)], axis=1)
    return np.sort(np.partition(d, k - 1, axis=1)[:, :k], axis=1)


def _mean3(b):
    with np.errstate(over="ignore"):
        return ((b[:, 0] + b[:, 1]) + b[:, 2]) / b.dtype.type(3)


def _brute(pts, rows, dtype, missing, pick, exclude):
    pts = np.ascontiguousarray(pts, dtype)
    P = len(pts)
    rows = np.arange(P) if rows is None else np.asarray(rows)
    out = np.empty(len(rows), dtype)
    step = max(1, _PAIRS // max(P, 1))
    for r0 in range(0, len(rows), step):
        r = rows[r0: r0 + step]
        d = _dist2(pts, pts[r])
        if exclude == "index":
            d[np.arange(len(r)), r] = missing
        else:                                          # (wrong on purpose: a duplicate is dropped with the point itself)
            d[~(d > 0)] = missing
        out[r0: r0 + step] = _mean3(_smallest(d, max(pick) + 1, missing)[:, list(pick)])
    return out


def mean_dist2_exact(pts, rows=None):
    """float64 [P] (or one entry per index in `rows`): mean of the three smallest squared distances to the OTHER points,
    a point being excluded by its index; inf where fewer than three are finite."""
    return _brute(pts, rows, np.float64, np.float64(np.inf), (0, 1, 2), "index")


def mean_dist2_f32(pts, rows=None, pick=(0, 1, 2), exclude="index"):
    """float32 [P] (or one entry per index in `rows`): what the kernel must return, bit for bit."""
    return _brute(pts, rows, np.float32, FLT_MAX, pick, exclude)


# ---- the kernel's intermediates -------------------------------------------------------------------------------------------
def scene_box(pts, seed_origin=True):
    """(lo [3], hi [3]) float32: minimum and maximum per axis, both seeded with 0 as upstream does."""
    lo, hi = np.fmin.reduce(pts, axis=0), np.fmax.reduce(pts, axis=0)
    if seed_origin:
        lo, hi = np.fmin(lo, np.float32(0)), np.fmax(hi, np.float32(0))
    return lo.astype(np.float32), hi.astype(np.float32)


def _spread10(x):
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def morton_codes(pts, seed_origin=True, axes=(0, 1, 2)):
    """uint32 [P]: knn.hip::morton_kernel in float32.  t = (p - lo) / ext (a correctly rounded division), t * 1023 clamped
    to [0, 1023] (a NaN becomes 0) and truncated, 10 bits per axis interleaved as x | y << 1 | z << 2; 0 for an axis of
    no extent."""
    pts = np.ascontiguousarray(pts, np.float32)
    lo, hi = scene_box(pts, seed_origin)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ext = hi - lo
        t = np.where(ext > 0, (pts - lo) / ext, np.float32(0))
        q = np.fmin(np.fmax(t * np.float32(1023), np.float32(0)), np.float32(1023))
    c = _spread10(q.astype(np.uint32))
    return c[:, axes[0]] | (c[:, axes[1]] << 1) | (c[:, axes[2]] << 2)


def boxes(sorted_pts):
    """float32 [ceil(P / 1024), 6]: lo[3], hi[3] of every 1024 consecutive points (the last box holds what is left)."""
    n = (len(sorted_pts) + BOX - 1) // BOX
    out = np.empty((n, 6), np.float32)
    for b in range(n):
        chunk = sorted_pts[b * BOX: (b + 1) * BOX]
        out[b, :3], out[b, 3:] = np.fmin.reduce(chunk, axis=0), np.fmax.reduce(chunk, axis=0)
    return out


# ---- the whole scheme -----------------------------------------------------------------------------------------------------
def scheme(pts, prune=">", seed_origin=True, axes=(0, 1, 2), last_box=True):
    """knn.hip restated with its pruning.  Points in the stable order of their Morton codes, boxes of 1024; per point
    `reject` = the third smallest distance to its +-3 neighbours in that order; then box after box: d = squared distance
    to the box, skipped `if (d > reject || d > best[2])`, else every point of the box but the point itself is a
    candidate.  prune=">=" is the wrong comparison, last_box=False forgets the box that is not full.
    -> dict(out, codes, order, sorted, boxes)."""
    pts = np.ascontiguousarray(pts, np.float32)
    P = len(pts)
    codes = morton_codes(pts, seed_origin, axes)
    order = np.argsort(codes, kind="stable")
    s = pts[order]
    bx = boxes(s)
    idx = np.arange(P)
    near = np.full((P, 6), FLT_MAX, np.float32)
    for k, off in enumerate((-3, -2, -1, 1, 2, 3)):
        ok = (idx + off >= 0) & (idx + off < P)
        i, j = idx[ok], idx[ok] + off
        with np.errstate(over="ignore", invalid="ignore"):
            dx, dy, dz = (s[j, a] - s[i, a] for a in range(3))
            near[ok, k] = (dx * dx + dy * dy) + dz * dz
    reject = _smallest(near, 3, FLT_MAX)[:, 2]
    best = np.full((P, 3), FLT_MAX, np.float32)
    for b in range(len(bx) if last_box else P // BOX):
        lo, hi = bx[b, :3], bx[b, 3:]
        with np.errstate(over="ignore", invalid="ignore"):
            t = np.fmin(np.abs(s - lo), np.abs(s - hi))
            tt = np.where((s < lo) | (s > hi), t * t, np.float32(0))
            d = ((np.float32(0) + tt[:, 0]) + tt[:, 1]) + tt[:, 2]
            skip = ((d > reject) | (d > best[:, 2])) if prune == ">" else ((d >= reject) | (d >= best[:, 2]))
        todo = idx[~skip]
        j0, j1 = b * BOX, min(P, (b + 1) * BOX)
        for r0 in range(0, len(todo), _PAIRS // BOX):
            r = todo[r0: r0 + _PAIRS // BOX]
            dist = _dist2(s[j0:j1], s[r])
            own = (r >= j0) & (r < j1)
            dist[np.nonzero(own)[0], r[own] - j0] = FLT_MAX
            best[r] = _smallest(np.concatenate([best[r], dist], axis=1), 3, FLT_MAX)
    out = np.empty(P, np.float32)
    out[order] = _mean3(best)
    return dict(out=out, codes=codes, order=order, sorted=s, boxes=bx)


# Each entry: pts -> dict with some of scheme()'s keys, wrong on purpose.  A cloud "catches" a variant when one of those
# arrays differs from scheme(pts)'s.
variants = {
    "fourth_neighbour": lambda pts: dict(out=mean_dist2_f32(pts, pick=(0, 1, 3))),
    "exclude_by_distance": lambda pts: dict(out=mean_dist2_f32(pts, exclude="d>0")),
    "skip_last_partial_box": lambda pts: scheme(pts, last_box=False),
    "prune_greater_equal": lambda pts: scheme(pts, prune=">="),
    "scene_box_without_origin": lambda pts: scheme(pts, seed_origin=False),
    "morton_axes_swapped": lambda pts: scheme(pts, axes=(2, 1, 0)),
}
