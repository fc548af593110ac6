"""Plain numpy reference of the binning stage (csrc/binning.hip): tile rects, depth order, tile lists, ranges, the two rounds.

Integer work throughout, so every comparison against it is exact.  Rects are recomputed in float32 from what the projection
stored (pixel position, radius, footprint half-extents) with the operations of preprocess.hip -- subtractions, additions, a
division by 16, ceilf, floorf, a clamped cast: each is one correctly rounded float32 operation in numpy as on the device --
and tied to the device by `guard_rects` (area == tiles_touched for every Gaussian).  Depth keys are the float bits of view z,
0xFFFFFFFF for a Gaussian behind the near plane.
"""
import numpy as np

TILE = 16
CULLED = 0xFFFFFFFF
KEY27_BASE = 0x3E4CCCCD          # float bits of the near plane, 0.2f (binning.hip)
KEY27_SPAN = 1 << 27


def grid(W, H):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def _clampi(v, hi):
    """clampi_from_float: (int)fminf(fmaxf(v, 0), hi) -- fmaxf / fminf return the other operand for a NaN"""
    return np.fmin(np.fmax(v, np.float32(0.0)), np.float32(hi)).astype(np.int64)


def rects_reference(mx, my, radii, W, H):
    """The reference's rect of every Gaussian: tiles reached by (mx, my) +- radius -> [P, 4] int64 x0, y0, x1, y1 (exclusive).
    radii == 0 (culled, or no tile): empty."""
    gx, gy = grid(W, H)
    mx, my = np.asarray(mx, np.float32), np.asarray(my, np.float32)
    r = np.asarray(radii).astype(np.float32)
    T, T1 = np.float32(TILE), np.float32(TILE - 1)
    x0 = _clampi((mx - r) / T, gx)
    y0 = _clampi((my - r) / T, gy)
    x1 = _clampi(((mx + r) + T1) / T, gx)
    y1 = _clampi(((my + r) + T1) / T, gy)
    rect = np.stack([x0, y0, x1, y1], 1)
    rect[np.asarray(radii) <= 0] = 0
    return rect


def rects_tight(mx, my, radii, ext_x, ext_y, W, H):
    """The tight rect: the reference's, intersected with the tiles the alpha >= 1/255 footprint (half-extents ext_x, ext_y
    around the centre; negative when the opacity is below 1/255) can reach; empty when the opacity is below 1/255."""
    gx, gy = grid(W, H)
    ref = rects_reference(mx, my, radii, W, H)
    mx, my = np.asarray(mx, np.float32), np.asarray(my, np.float32)
    ex, ey = np.asarray(ext_x, np.float32), np.asarray(ext_y, np.float32)
    T, T1, one = np.float32(TILE), np.float32(TILE - 1), np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        tx0 = _clampi(np.ceil(((mx - ex) - T1) / T), gx)
        tx1 = _clampi(np.floor((mx + ex) / T) + one, gx)
        ty0 = _clampi(np.ceil(((my - ey) - T1) / T), gy)
        ty1 = _clampi(np.floor((my + ey) / T) + one, gy)
    x0 = np.maximum(ref[:, 0], tx0)
    x1 = np.maximum(x0, np.minimum(ref[:, 2], tx1))
    y0 = np.maximum(ref[:, 1], ty0)
    y1 = np.maximum(y0, np.minimum(ref[:, 3], ty1))
    x1 = np.where(ex < 0, x0, x1)
    rect = np.stack([x0, y0, x1, y1], 1)
    rect[np.asarray(radii) <= 0] = 0
    return rect


def rects_from_records(records, radii, W, H, tight):
    """Rects from the device's records ([P, 16] float32: mx, my in words 0, 1; ext_x, ext_y in words 10, 11) and radii."""
    rec = np.asarray(records, np.float32)
    if tight:
        return rects_tight(rec[:, 0], rec[:, 1], radii, rec[:, 10], rec[:, 11], W, H)
    return rects_reference(rec[:, 0], rec[:, 1], radii, W, H)


def area(rect):
    return (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])


def guard_rects(rect, tiles_touched):
    """The recomputed rects are the device's: for EVERY Gaussian the rect area equals the device's tiles_touched."""
    a, t = area(rect), np.asarray(tiles_touched).astype(np.int64) & 0xFFFFFFFF
    bad = np.nonzero(a != t)[0]
    assert len(bad) == 0, f"rect area != tiles_touched at {len(bad)} Gaussians, first {bad[:5]}: {a[bad[:5]]} vs {t[bad[:5]]}"


def depth_order(keys):
    """Stable order of the uint32 depth keys: culled keys (0xFFFFFFFF) sink to the end, ties keep index order."""
    return np.argsort(np.asarray(keys).astype(np.int64) & 0xFFFFFFFF, kind="stable")


def emit(order, rect, gx):
    """(tile, index, rank) of every tile of every rect, Gaussians in depth order."""
    order = np.asarray(order, np.int64)
    r = rect[order]
    a = area(r)
    n = int(a.sum())
    src = np.repeat(np.arange(len(order)), a)                  # rank in the depth order
    first = np.repeat(np.cumsum(a) - a, a)
    k = np.arange(n) - first
    w = np.repeat(r[:, 2] - r[:, 0], a)
    tile = (np.repeat(r[:, 1], a) + k // np.maximum(w, 1)) * gx + np.repeat(r[:, 0], a) + k % np.maximum(w, 1)
    return tile, order[src], src


def ranges_of(tile, tiles, offset=0):
    """[tiles, 2] begin / end of every tile in a tile-sorted array; an empty tile is (0, 0)."""
    b = np.searchsorted(tile, np.arange(tiles), "left")
    e = np.searchsorted(tile, np.arange(tiles), "right")
    out = np.stack([b, e], 1) + offset
    out[b == e] = 0
    return out


class Lists:
    """point_list, tile_ids (tile-major, depth order inside a tile), ranges, N, V and tiles_touched of one round."""

    def __init__(self, keys, rect, W, H, order=None):
        gx, gy = grid(W, H)
        self.order = depth_order(keys) if order is None else np.asarray(order, np.int64)
        self.rect, self.gx, self.tiles = rect, gx, gx * gy
        tile, idx, rank = emit(self.order, rect, gx)
        s = np.argsort(tile, kind="stable")
        self.tile_ids, self.point_list, self.rank = tile[s], idx[s], rank[s]
        self.ranges = ranges_of(self.tile_ids, self.tiles)
        self.tiles_touched = area(rect)
        self.N, self.V = len(tile), int((self.tiles_touched > 0).sum())

    def tile_list(self, t):
        return self.point_list[self.ranges[t, 0]:self.ranges[t, 1]]

    def two_rounds(self, K1, predicted, open_):
        """Segment 1: every entry whose Gaussian has depth rank < K1, and every entry of a predicted-open tile.  Segment 2:
        the entries of rank >= K1 in tiles that are open (after segment 1) and not predicted.  Both tile-major, depth order
        kept; segment 2 sits behind segment 1 in one array, its ranges are absolute.
        -> dict(point_list, tile_ids, ranges, ranges2, N1, N2, V)"""
        pred = np.zeros(self.tiles, bool)
        pred[list(predicted)] = True
        op = np.zeros(self.tiles, bool)
        op[list(open_)] = True
        in1 = (self.rank < K1) | pred[self.tile_ids]
        in2 = ~in1 & op[self.tile_ids]
        t1, t2 = self.tile_ids[in1], self.tile_ids[in2]
        # header word V of a two-round forward: the Gaussians the first round gathers -- rank < K1 with a non-empty rect, and
        # those behind K1 that reach a predicted tile
        v = int((self.tiles_touched[self.order[:K1]] > 0).sum()) + len(np.unique(self.point_list[(self.rank >= K1) & pred[self.tile_ids]]))
        return dict(point_list=np.concatenate([self.point_list[in1], self.point_list[in2]]), tile_ids=np.concatenate([t1, t2]),
                    ranges=ranges_of(t1, self.tiles), ranges2=ranges_of(t2, self.tiles, offset=len(t1)), N1=len(t1), N2=len(t2), V=v)


def is_subsequence(sub, full):
    """sub is an order-preserving sub-list of full (both without duplicates)"""
    sub, full = np.asarray(sub, np.int64), np.asarray(full, np.int64)
    if len(np.unique(sub)) != len(sub) or len(np.unique(full)) != len(full):
        return False
    pos = {int(g): i for i, g in enumerate(full)}
    p = [pos.get(int(g), -1) for g in sub]
    return all(q >= 0 for q in p) and all(a < b for a, b in zip(p, p[1:]))
