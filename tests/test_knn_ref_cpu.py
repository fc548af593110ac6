"""tests/knn_ref.py checked on the CPU: its float32 statement against its float64 brute force, its restated pruning scheme
against brute force, hand-computed values, and every deliberately wrong variant told apart by a named cloud; no GPU.

tests/test_gpu_knn_edges.py compares csrc/knn.hip with this module bit for bit on the same clouds."""
import functools

import numpy as np
import pytest

import knn_ref
from knn_ref import FLT_MAX

# 9 ulps, see test_f32_statement_is_the_exact_one_rounded
ULPS = 9
SUBSET = 1024          # rows of the one large cloud that are compared with brute force here


@functools.lru_cache(maxsize=None)
def _facts(name):
    pts = knn_ref.cloud(name)
    rows = None if len(pts) <= 4096 else np.sort(np.random.default_rng(len(pts)).choice(len(pts), SUBSET, replace=False))
    facts = dict(pts=pts, rows=rows, f32=knn_ref.mean_dist2_f32(pts, rows), exact=knn_ref.mean_dist2_exact(pts, rows),
                 scheme=knn_ref.scheme(pts))
    for a in (pts, facts["f32"], facts["exact"], *facts["scheme"].values()):
        a.setflags(write=False)
    return facts


def test_clouds_are_what_their_names_say():
    assert [len(knn_ref.cloud("uniform_%d" % p)) for p in knn_ref.SIZES] == list(knn_ref.SIZES)
    assert {n: len(knn_ref.cloud(n)) for n in knn_ref.SHAPES} == dict(
        lattice=2197, lattice_tenth=2197, far=2049, negative=2049, line=2049, point=1500, twins=2048, clusters=4096,
        nonfinite=2049, seam=2048)
    for n in knn_ref.CLOUDS:
        a, b = knn_ref.cloud(n), knn_ref.cloud(n)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert len(np.unique(knn_ref.cloud("twins"), axis=0)) == 1024 and len(np.unique(knn_ref.cloud("point"), axis=0)) == 1
    nf = knn_ref.cloud("nonfinite")
    assert np.isnan(nf[0, 0]) and nf[1024, 1] == np.inf and nf[2048, 2] == -np.inf and (~np.isfinite(nf)).sum() == 3
    assert np.ptp(knn_ref.cloud("line"), axis=0)[1:].tolist() == [0, 0]


def test_hand_computed_values():
    pts = np.array([[0.0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 3]], np.float32)
    want = [5 / 3, 5 / 3, (1 + 1 + 5) / 3, (4 + 4 + 5) / 3, (9 + 9 + 10) / 3]         # the twin counts, at distance 0
    assert knn_ref.mean_dist2_exact(pts).tolist() == want
    assert knn_ref.mean_dist2_f32(pts).tolist() == np.array(want, np.float32).tolist()
    # fewer than three neighbours: FLT_MAX terms in float32 arithmetic
    assert knn_ref.mean_dist2_f32(pts[:3]).tolist() == [FLT_MAX / np.float32(3)] * 3      # (0 + 1) + FLT_MAX = FLT_MAX
    assert knn_ref.mean_dist2_f32(pts[:2]).tolist() == [np.inf] * 2 == knn_ref.mean_dist2_f32(pts[:1]).tolist() * 2
    assert np.all(np.isinf(knn_ref.mean_dist2_exact(pts[:3])))
    # the scene box contains the origin; a point on its maximum gets 1023, on its minimum 0, an axis of no extent 0
    box = np.array([[2.0, 0, -4], [1, 0, -1]], np.float32)
    lo, hi = knn_ref.scene_box(box)
    assert lo.tolist() == [0, 0, -4] and hi.tolist() == [2, 0, 0]
    # (x = 1 of [0, 2]: 511.5 -> 511; z = -1 of [-4, 0]: 767.25 -> 767)
    assert knn_ref.morton_codes(box).tolist() == [0x09249249, _spread(511) | _spread(767) << 2] and _spread(1023) == 0x09249249
    assert knn_ref.morton_codes(np.array([[3.0, 5, 7]], np.float32)).tolist() == [0x3FFFFFFF]
    assert knn_ref.morton_codes(np.array([[np.nan, -1, np.inf]], np.float32)).tolist() == [0]
    assert knn_ref.boxes(np.arange(3075, dtype=np.float32).reshape(1025, 3)).tolist() == [[0, 1, 2, 3069, 3070, 3071],
                                                                                          [3072, 3073, 3074] * 2]


def _spread(v):
    return sum(((v >> k) & 1) << (3 * k) for k in range(10))


@pytest.mark.parametrize("name", knn_ref.CLOUDS)
def test_f32_statement_is_the_exact_one_rounded(name):
    """|mean_dist2_f32 - mean_dist2_exact| <= 9 ulps of the float32 result.

    With u = 2^-24, one float32 rounding multiplies by (1 + e), |e| <= u.  A distance (dx*dx + dy*dy) + dz*dz: the
    difference dx is rounded once and enters squared (2u), the product is rounded (1u), and the x and y terms pass
    through two sums (2u), the z term through one: five roundings on the longest path, so every term, all of them
    non-negative, is within (1 + u)^5 of its exact value and so is the distance.  A perturbation of every entry by at
    most that factor moves the k-th smallest VALUE by at most that factor, whichever points realise it.  The mean
    ((b0 + b1) + b2) / 3 adds two sums and a division: (1 + u)^8 in all, 8 u to first order.  One ulp of a float32 r
    is more than u * r, so that is below 8 ulps; the ninth covers the second-order terms.  (Inputs are float32, so the
    float64 differences are exact; float64's own roundings are 2^-29 of these.)  No cloud here has a distance small
    enough for a square to be subnormal unless it is exactly 0."""
    f = _facts(name)
    got, exact = f["f32"], f["exact"]
    fin = np.isfinite(exact)
    err = np.abs(got[fin].astype(np.float64) - exact[fin]) / np.spacing(np.maximum(got[fin], np.float32(1e-30))).astype(np.float64)
    print(f"{name}: {int(fin.sum())} rows, max |f32 - exact| = {err.max() if len(err) else 0:.2f} ulp; "
          f"{int((~fin).sum())} rows with fewer than three finite neighbours")
    assert np.all(np.isfinite(got[fin])) and np.all(err <= ULPS)
    assert np.all(got[fin][exact[fin] == 0] == 0)
    # fewer than three neighbours: inf, or FLT_MAX / 3 where two small distances vanish against one FLT_MAX
    assert np.all(np.isin(got[~fin], [np.float32(np.inf), FLT_MAX / np.float32(3)]))
    if name == "nonfinite":
        assert np.nonzero(~fin)[0].tolist() == list(knn_ref.NONFINITE_ROWS) and np.all(np.isinf(got[~fin]))
    elif len(f["pts"]) > 3:
        assert fin.all()


@pytest.mark.parametrize("name", knn_ref.CLOUDS)
def test_scheme_with_strict_pruning_is_brute_force(name):
    f = _facts(name)
    s, rows = f["scheme"], f["rows"]
    out = s["out"] if rows is None else s["out"][rows]
    print(f"{name}: {int((out != f['f32']).sum())} of {len(out)} outputs differ from brute force")
    assert np.array_equal(out, f["f32"])
    assert np.array_equal(s["codes"], knn_ref.morton_codes(f["pts"])) and np.array_equal(s["sorted"], f["pts"][s["order"]], equal_nan=True)
    assert np.array_equal(s["boxes"], knn_ref.boxes(s["sorted"]))
    assert np.all(np.diff(s["codes"][s["order"]].astype(np.int64)) >= 0) and int(s["codes"].max()) <= 0x3FFFFFFF


def test_nonfinite_rows_are_nobodys_neighbours():
    f = _facts("nonfinite")
    keep = np.setdiff1d(np.arange(len(f["pts"])), knn_ref.NONFINITE_ROWS)
    assert np.array_equal(f["f32"][keep], knn_ref.mean_dist2_f32(f["pts"][keep]))


# variant -> (the cloud that catches it, the array that differs)
CAUGHT_BY = {
    "fourth_neighbour": ("uniform_4", "out"),
    "exclude_by_distance": ("twins", "out"),
    "skip_last_partial_box": ("uniform_1025", "out"),
    "prune_greater_equal": ("seam", "out"),
    "scene_box_without_origin": ("far", "codes"),
    "morton_axes_swapped": ("uniform_257", "codes"),
}


def test_every_wrong_variant_is_caught_by_a_named_cloud():
    """(`>=` at the pruning comparison: ties there are everywhere on `lattice`, but a lattice point lies inside the
    bounds of the boxes that hold its nearest neighbours, so dropping the tied boxes loses no value and `lattice` does NOT
    catch it.  `seam` puts a box face exactly at the bound; `point` does too: its own box is at distance 0 = the bound.)"""
    assert set(CAUGHT_BY) == set(knn_ref.variants)
    for variant, (name, key) in CAUGHT_BY.items():
        right, wrong = _facts(name)["scheme"], knn_ref.variants[variant](_facts(name)["pts"])
        n = int((wrong[key] != right[key]).sum())
        print(f"{variant}: caught by `{name}`, {n} of {len(right[key])} entries of `{key}` differ")
        assert n > 0
    wrong = knn_ref.variants["prune_greater_equal"](_facts("point")["pts"])
    assert np.all(wrong["out"] != 0) and np.all(_facts("point")["f32"] == 0)
    # the origin-seeded box squeezes `far` (width 1 of an extent above 100: 10.23 cell widths, so at most 12 of the 1024
    # cells of an axis), the unseeded one spreads it out
    far = _facts("far")
    cells = np.stack([far["scheme"]["codes"] >> a & 0x09249249 for a in range(3)])
    assert all(len(np.unique(c)) <= 12 for c in cells) and len(np.unique(knn_ref.morton_codes(far["pts"], seed_origin=False))) > 2000
