"""GPU: csrc/knn.hip (b3gs_knn_mean_dist2) bit for bit against the numpy restatement tests/knn_ref.py, which
tests/test_knn_ref_cpu.py checks on the CPU: the result AND what the kernel leaves in a caller-owned workspace (Morton
codes, the sorted permutation, the points in Morton order, the bounds of every box of 1024), at the sizes where its
indexing changes and on the clouds that its origin-seeded scene box, its strict pruning comparison and its exclusion by
index treat differently.  The library is built with -ffp-contract=off, so the criterion is equality of bits.

Beside it: b3gs_mark_visible at the near plane and at its launch tail, and create_from_points on clouds of duplicates."""
import numpy as np
import pytest
import torch

import knn_ref
from knn_ref import FLT_MAX

pytestmark = pytest.mark.gpu

SUBSET = 4096          # rows of the one large cloud whose result is compared with brute force; intermediates in full


def _a256(nbytes):
    return (nbytes + 255) & ~255


def _layout(L, n):
    """Byte offsets into the workspace, by knn.hip::carve_ws:
    part [6 * 256 floats] | codes | skey[0] | skey[1] | sval[0] | sval[1] | hist | sorted [3 n floats] | boxes [24 bytes each]."""
    step, nb = _a256(4 * n), (n + knn_ref.BOX - 1) // knn_ref.BOX
    off = dict(part=0, codes=_a256(6 * 256 * 4))
    off["sval0"] = off["codes"] + 3 * step
    off["hist"] = off["codes"] + 5 * step
    off["sorted"] = off["hist"] + _a256(4 * (1280 + 8192 + 4 * 256 * ((n + 4095) // 4096 + 1)))     # b3gs_sort_scratch_words
    off["boxes"] = off["sorted"] + _a256(12 * n)
    assert off["boxes"] + _a256(24 * nb) == L.b3gs_knn_workspace_bytes(n), "knn.hip::carve_ws and this test are out of step"
    return off, nb


def _run(pts):
    """-> dict(out, part, codes, order, sorted, boxes) of a first call on a workspace filled with 0xFF, and `again`: the same
    of a second call on that workspace as the first one left it."""
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    n = len(pts)
    off, nb = _layout(L, n)
    dev = torch.from_numpy(pts).cuda()
    ws = torch.full((L.b3gs_knn_workspace_bytes(n),), 255, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        out = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        _lib.check(L.b3gs_knn_mean_dist2(n, dev.data_ptr(), out.data_ptr(), ws.data_ptr(), stream), "b3gs_knn_mean_dist2")
        torch.cuda.synchronize()
        host = ws.cpu().numpy()
        words = lambda key, count, dtype: host[off[key]: off[key] + 4 * count].view(dtype).copy()      # noqa: E731
        nparts = min((n + 255) // 256, 256)
        return dict(out=out.cpu().numpy(), part=words("part", 6 * nparts, np.float32).reshape(nparts, 6),
                    codes=words("codes", n, np.uint32), order=words("sval0", n, np.uint32),
                    sorted=words("sorted", 3 * n, np.float32).reshape(n, 3), boxes=words("boxes", 6 * nb, np.float32).reshape(nb, 6))

    first = call()
    first["again"] = call()
    return first


def _differ(a, b):
    """Entries that are not the same number (a NaN equals a NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    both_nan = (a != a) & (b != b)
    return int(((a != b) & ~both_nan).sum())


@pytest.mark.parametrize("name", knn_ref.CLOUDS)
def test_result_and_intermediates_equal_the_restatement(name):
    """Differing entries, printed per cloud before anything is asserted; every count must be 0 (and was, on all 27
    clouds, on the first run on an MI355X)."""
    pts = knn_ref.cloud(name)
    n = len(pts)
    got = _run(pts)
    rows = np.arange(n) if n <= SUBSET else np.sort(np.random.default_rng(n).choice(n, SUBSET, replace=False))
    want_out = knn_ref.mean_dist2_f32(pts, rows)
    lo, hi = knn_ref.scene_box(pts)
    codes = knn_ref.morton_codes(pts)
    order = np.argsort(codes, kind="stable")
    count = dict(
        out=_differ(got["out"][rows], want_out),
        scene_box=_differ(np.concatenate([np.fmin(np.fmin.reduce(got["part"][:, :3]), 0), np.fmax(np.fmax.reduce(got["part"][:, 3:]), 0)]),
                          np.concatenate([lo, hi])),
        codes=_differ(got["codes"], codes),
        order=_differ(got["order"], order.astype(np.uint32)),
        sorted=_differ(got["sorted"], pts[order]),
        boxes=_differ(got["boxes"], knn_ref.boxes(got["sorted"])),
        flt_max_in_boxes=int((np.abs(got["boxes"]) == FLT_MAX).sum()),
        second_call=sum(_differ(got[k], got["again"][k]) for k in ("out", "part", "codes", "order", "sorted", "boxes")))
    if name == "nonfinite":
        bad = list(knn_ref.NONFINITE_ROWS)
        keep = np.setdiff1d(np.arange(n), bad)
        count["finite_rows_without_the_others"] = _differ(got["out"][keep], knn_ref.mean_dist2_f32(pts[keep]))
        count["nonfinite_rows_not_inf"] = int((got["out"][bad] != np.inf).sum())
    if name == "point":
        count["nonzero"] = int((got["out"] != 0).sum())
    print(f"{name} (P = {n}, {len(rows)} rows of `out`): differing entries " + ", ".join(f"{k} {v}" for k, v in count.items()))
    assert not any(count.values()), count


def test_twins_are_neighbours_at_distance_zero():
    """Exclusion is by index: the twin counts, at distance 0, so both twins get the same (0 + d1 + d2) / 3, below the
    mean over the three nearest DISTINCT points that exclusion by distance would give."""
    pts = knn_ref.cloud("twins")
    got = _run(pts)["out"]
    _, inverse = np.unique(pts, axis=0, return_inverse=True)
    pair = np.argsort(inverse.ravel(), kind="stable").reshape(-1, 2)
    print(f"twins: {int((got[pair[:, 0]] != got[pair[:, 1]]).sum())} pairs with different results")
    assert np.array_equal(got[pair[:, 0]], got[pair[:, 1]]) and np.all(got > 0) and np.all(np.isfinite(got))
    assert np.all(got < knn_ref.mean_dist2_f32(pts, exclude="d>0"))


@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_mark_visible_at_the_near_plane(P):
    """vz = ((m2*x + m6*y) + m10*z) + m14 > B3GS_NEAR in float32, one rounding per operation.  The last three points (as
    many as P has) land ON the near plane (not visible), one ulp above (visible) and one ulp below; with powers of two in
    the matrix their products and sums are exact: 0.5*1 + (-0.25)*2 = 0, 2*z = (near - 0.125) -+ 2^-26, + 0.125.
    The projection matrix is not read: it is all NaN."""
    from binocular3dgs_amd import _C
    near = np.float32(0.2)                                            # B3GS_NEAR
    rng = np.random.default_rng(P)
    view = rng.normal(size=(4, 4)).astype(np.float32)
    view[:, 2] = [0.5, -0.25, 2.0, 0.125]                             # flat entries 2, 6, 10, 14
    pts = rng.uniform(-1, 1, size=(P, 3)).astype(np.float32)
    pts[:, 2] = pts[:, 2] * np.float32(0.5)                           # vz spread over both sides of the plane
    targets = [near, np.nextafter(near, np.float32(1)), np.nextafter(near, np.float32(0))][:P]
    for k, t in enumerate(targets):
        pts[P - 1 - k] = [1.0, 2.0, (t - np.float32(0.125)) / np.float32(2)]
    m = view.reshape(-1)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    vz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14]
    assert vz.dtype == np.float32 and [vz[P - 1 - k] for k in range(len(targets))] == targets
    want = vz > near
    assert P < 255 or 0.2 < want.mean() < 0.8
    got = _C.mark_visible(torch.from_numpy(pts).cuda(), torch.from_numpy(view).cuda(),
                          torch.full((4, 4), float("nan"), device="cuda"))
    assert got.dtype == torch.bool and got.shape == (P,)
    got = got.cpu().numpy()
    print(f"mark_visible P = {P}: {int((got != want).sum())} differing entries, {int(want.sum())} visible")
    assert np.array_equal(got, want)
    assert got[::-1][:3].tolist() == [False, True, False][:P]           # on the plane, one ulp above, one ulp below


@pytest.mark.parametrize("name", ["twins", "point"])
def test_create_from_points_on_duplicates(name):
    """scale = log(sqrt(max(dist2, 1e-7))): finite on both clouds.  On `point` every dist2 is 0 and the floor decides; on
    `twins` one term of three is 0, so dist2 = (d1 + d2) / 3 stays above the floor and the scale follows the restatement."""
    from binocular3dgs_amd.init_points import create_from_points
    pts = knn_ref.cloud(name)
    m = create_from_points(pts, np.full_like(pts, 0.5), sh_degree=0)
    s = m._scaling.detach().cpu().numpy()
    assert s.shape == (len(pts), 3) and np.all(np.isfinite(s)) and np.array_equal(s[:, 0], s[:, 1]) and np.array_equal(s[:, 0], s[:, 2])
    dist2 = knn_ref.mean_dist2_f32(pts)
    want = np.log(np.sqrt(np.maximum(dist2.astype(np.float64), np.float64(np.float32(1e-7)))))
    err = np.abs(s[:, 0] - want).max()
    print(f"create_from_points on `{name}`: max |scale - log(sqrt(max(dist2, 1e-7)))| = {err:.3g}; floor taken by "
          f"{int((dist2 < 1e-7).sum())} of {len(pts)}")
    assert err <= 4 * np.spacing(np.float32(8.06))                    # |scale| <= 8.06 = -log(sqrt(1e-7)); sqrt and log: a few ulps
    if name == "point":
        assert np.all(dist2 == 0) and len(np.unique(s)) == 1 and abs(float(s[0, 0]) - np.log(np.sqrt(1e-7))) < 1e-5
    else:
        assert np.all(dist2 > 1e-7)
