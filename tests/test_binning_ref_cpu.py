"""tests/binning_ref.py against oracle/tile_ref.c (its 64-bit key sort) and against brute force; no GPU."""
import numpy as np
import pytest

import binning_ref
from helpers import oracle_kwargs, small_scene


def _keys(st):
    k = np.ascontiguousarray(st.depths, np.float32).view(np.uint32).astype(np.int64)
    return np.where(st.radii > 0, k, binning_ref.CULLED)


@pytest.mark.parametrize("P,W,H,ties", [(257, 33, 17, False), (500, 64, 48, False), (700, 80, 50, True)])
def test_reference_reproduces_the_oracle(P, W, H, ties):
    from oracle import tile_ref
    d, _ = small_scene(P=P, W=W, H=H, seed=P, near_frac=0.05, yaw=0.0 if ties else 5.0)
    if ties:      # view z = stored z under the unrotated camera: a handful of distinct depths
        d["means3D"] = d["means3D"].clone()
        d["means3D"][:, 2] = (d["means3D"][:, 2] * 2).round() / 2
    st = tile_ref.forward(**oracle_kwargs(d))
    vis = st.radii > 0
    assert st.N > P and 0 < vis.sum() < P
    keys = _keys(st)
    n_tied = int(vis.sum()) - len(np.unique(keys[vis]))
    assert (n_tied > 0.9 * vis.sum()) if ties else True, f"{n_tied} tied keys of {int(vis.sum())}"
    rect = binning_ref.rects_reference(st.means2D[:, 0], st.means2D[:, 1], st.radii, W, H)
    binning_ref.guard_rects(rect, st.tiles_touched)
    ref = binning_ref.Lists(keys, rect, W, H)
    assert ref.N == st.N and ref.V == int(vis.sum())
    np.testing.assert_array_equal(ref.tiles_touched, st.tiles_touched)
    np.testing.assert_array_equal(ref.point_list, st.point_list)
    np.testing.assert_array_equal(ref.tile_ids, (st.keys >> np.uint64(32)).astype(np.int64))
    want = st.ranges.astype(np.int64)
    want[want[:, 1] <= want[:, 0]] = 0
    np.testing.assert_array_equal(ref.ranges, want)


def test_tight_rect_is_inside_the_reference_rect_and_empty_below_the_alpha_floor():
    mx = np.array([40.0, 40.0, 40.0, 3.0], np.float32)
    my = np.array([24.0, 24.0, 24.0, 60.0], np.float32)
    radii = np.array([30, 30, 30, 9])
    ext = np.array([4.0, 100.0, -1.0e30, 2.0], np.float32)
    full = binning_ref.rects_reference(mx, my, radii, 96, 64)
    tight = binning_ref.rects_tight(mx, my, radii, ext, ext, 96, 64)
    assert full.tolist() == [[0, 0, 5, 4], [0, 0, 5, 4], [0, 0, 5, 4], [0, 3, 1, 4]]
    assert tight[:2].tolist() == [[2, 1, 3, 2], [0, 0, 5, 4]] and tight[3].tolist() == [0, 3, 1, 4]
    assert binning_ref.area(tight)[2] == 0


def test_two_round_split_against_brute_force():
    """6 tiles (48 x 32), 12 Gaussians, 30 entries; K1 = 5; tile 1 predicted open, tiles 1, 2 and 4 open after segment 1."""
    W, H, K1, predicted, open_ = 48, 32, 5, {1}, {1, 2, 4}
    rect = np.array([[0, 0, 3, 2], [0, 0, 1, 1], [1, 0, 3, 1], [0, 1, 2, 2], [2, 0, 3, 2], [0, 0, 3, 1], [1, 1, 2, 2],
                     [0, 0, 0, 0], [1, 0, 2, 2], [0, 0, 2, 2], [2, 1, 3, 2], [0, 0, 3, 2]])
    keys = np.array([7, 3, 7, 1, 9, 3, 2, binning_ref.CULLED, 6, 5, 7, 4])
    ref = binning_ref.Lists(keys, rect, W, H)
    assert ref.N == 30 and ref.V == 11 and ref.tiles == 6
    order = sorted(range(12), key=lambda i: (keys[i], i))
    assert ref.order.tolist() == order
    rank = {g: r for r, g in enumerate(order)}
    seg1, seg2 = [], []
    for t in range(6):
        ty, tx = divmod(t, 3)
        inside = [g for g in order if rect[g][0] <= tx < rect[g][2] and rect[g][1] <= ty < rect[g][3]]
        assert ref.tile_list(t).tolist() == inside
        for g in inside:
            if rank[g] < K1 or t in predicted:
                seg1.append((t, g))
            elif t in open_:
                seg2.append((t, g))
    two = ref.two_rounds(K1, predicted, open_)
    assert (two["N1"], two["N2"]) == (len(seg1), len(seg2)) and two["N2"] > 0 and two["N1"] + two["N2"] < ref.N
    assert list(zip(two["tile_ids"].tolist(), two["point_list"].tolist())) == seg1 + seg2
    assert two["V"] == len({g for g in order[:K1] if ref.tiles_touched[g]} | {g for t, g in seg1 if rank[g] >= K1}) == 9
    for t in range(6):
        for key, seg, off in (("ranges", seg1, 0), ("ranges2", seg2, len(seg1))):
            where = [off + i for i, e in enumerate(seg) if e[0] == t]
            assert two[key][t].tolist() == ([where[0], where[-1] + 1] if where else [0, 0])
    assert binning_ref.is_subsequence([3, 9], [3, 5, 9]) and not binning_ref.is_subsequence([9, 3], [3, 5, 9])
    assert not binning_ref.is_subsequence([3, 3], [3, 5, 9]) and not binning_ref.is_subsequence([4], [3, 5, 9])
