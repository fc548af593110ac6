"""CPU: the merging rule of include/b3gs_raster.h in its restatement (tests/lod_ref.py) against independent numpy, the two
mutants the parity checks of tests/test_gpu_lod.py must catch, and the argument checks of the entry points, which need no
device.

The sweep count: on 10^5 random and degenerate symmetric 3 x 3 matrices (the families of _matrices() below, 33 times as many)
the restatement's Jacobi against numpy.linalg.eigh, eigenvalues and V diag(lambda) V^T relative to the largest eigenvalue,
measured 8.8e-3 / 6.7e-2 at 2 sweeps, 1.9e-10 / 7.9e-6 at 3 and 1.8e-15 / 1.7e-15 at 4: four is the smallest count within
1e-13."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lod_ref as lr  # noqa: E402

F = np.float32
ERR_ARG = -1


def _cov(scale, quat):
    R = np.array(lr.rotation_of(*(float(x) for x in quat)))
    return R @ np.diag(scale.astype(np.float64) ** 2) @ R.T


def _sym6(S):
    return np.array([[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]])


@pytest.fixture(scope="module")
def cluster():
    pos, sc, quat, alpha, dc, rest = lr.random_gaussians(40, 3, seed=11)
    w = np.random.default_rng(3).uniform(0.0, 2.0, 40)
    return pos, sc, quat, alpha, dc, rest, w


@pytest.mark.parametrize("weighted", [False, True])
def test_moments_are_those_of_the_mixture(cluster, weighted):
    pos, sc, quat, alpha, dc, rest, w = cluster
    w = w if weighted else None
    mo = lr.moments(range(40), pos, sc, quat, alpha, w)
    m = alpha.astype(np.float64) * np.prod(sc.astype(np.float64), axis=1) * (w if weighted else 1.0)
    p = m / m.sum()
    mu = (p[:, None] * pos).sum(0)
    Sigma = sum(p[i] * (_cov(sc[i], quat[i]) + np.outer(pos[i] - mu, pos[i] - mu)) for i in range(40))
    assert np.allclose(mo["mu"], mu, rtol=1e-12, atol=0)
    assert np.abs(_sym6(mo["Sigma"]) - Sigma).max() <= 1e-12 * np.abs(Sigma).max()
    assert mo["sum_a"] == pytest.approx((alpha.astype(np.float64) * np.prod(sc.astype(np.float64), axis=1)).sum(), rel=1e-13)
    cd, cr = lr.colours(mo, dc, rest)
    assert np.allclose(cd, (p[:, None] * dc).sum(0), rtol=1e-11, atol=1e-14) and np.allclose(cr, (p[:, None] * rest).sum(0), rtol=1e-11, atol=1e-14)


def _matrices(n=500, seed=0):
    g = np.random.default_rng(seed)
    q = lambda k: np.linalg.qr(g.normal(size=(k, 3, 3)))[0]                       # noqa: E731
    rot = lambda Q, lam: np.einsum("nij,nj,nkj->nik", Q, lam, Q)                  # noqa: E731
    b, v, u = g.normal(size=(n, 3, 3)), g.normal(size=(n, 3)), g.normal(size=(n, 3))
    two = np.exp(g.uniform(-3, 3, (n, 2)))
    tiny = g.normal(size=(n, 3, 3)) * 1e-14
    diag = np.zeros((n, 3, 3))
    diag[:, [0, 1, 2], [0, 1, 2]] = np.exp(g.uniform(-20, 20, (n, 3)))
    A = np.concatenate([rot(q(n), np.exp(g.uniform(-9, 2, (n, 3)))), b + b.transpose(0, 2, 1), np.einsum("ni,nj->nij", v, v),
                        np.einsum("ni,nj->nij", v, v) + np.einsum("ni,nj->nij", u, u),
                        rot(q(n), np.stack([two[:, 0], two[:, 0], two[:, 1]], 1)),
                        np.eye(3)[None] * np.exp(g.uniform(-5, 5, (n, 1, 1))) * (1 + tiny + tiny.transpose(0, 2, 1)), diag,
                        rot(q(n), np.exp(g.uniform(-30, 5, (n, 3)))), np.zeros((1, 3, 3))])
    return 0.5 * (A + A.transpose(0, 2, 1))


def _jacobi_error(A, sweeps):
    want = np.linalg.eigh(A)[0][:, ::-1]
    worst = 0.0
    for a, w in zip(A, want):
        lam, V = lr.jacobi(*(float(x) for x in (a[0, 0], a[0, 1], a[0, 2], a[1, 1], a[1, 2], a[2, 2])), sweeps=sweeps)
        lam, V = np.array(lam), np.array(V)
        big = max(np.abs(w).max(), np.finfo(np.float64).tiny)
        assert lam[0] >= lam[1] >= lam[2]
        worst = max(worst, np.abs(lam - w).max() / big, np.abs((V * lam) @ V.T - a).max() / big)
        if sweeps == lr.SWEEPS:
            assert abs(np.linalg.det(V) - 1.0) <= 1e-13 and np.abs(V.T @ V - np.eye(3)).max() <= 1e-13
    return worst


def test_jacobi_agrees_with_eigh_at_the_stated_sweep_count_and_not_below():
    A = _matrices()
    assert _jacobi_error(A, lr.SWEEPS) <= 1e-13
    assert _jacobi_error(A, lr.SWEEPS - 1) > 1e-13
    from binocular3dgs_amd import _C
    assert _C.MERGE_JACOBI_SWEEPS == lr.SWEEPS


def test_output_scales_and_rotation_reproduce_the_covariance(cluster):
    pos, sc, quat, alpha, dc, rest, w = cluster
    for idx in (range(40), range(2), range(5, 17)):
        mo = lr.moments(idx, pos, sc, quat, alpha, w)
        mu, s, q, al, vol = lr.merged(mo)
        assert min(s) > mo["smin"]                                              # (the floor is not active here)
        R = np.array(lr.rotation_of(*q))
        Sigma = _sym6(mo["Sigma"])
        assert np.abs(R @ np.diag(np.array(s) ** 2) @ R.T - Sigma).max() <= 1e-12 * np.abs(Sigma).max()
        assert q[0] >= 0.0 and abs(sum(x * x for x in q) - 1.0) <= 1e-15 and s[0] >= s[1] >= s[2]


def test_quaternion_branches_invert_rotation_of():
    g = np.random.default_rng(5)
    qs = list(g.normal(size=(200, 4))) + [np.array(v, float) for v in ((0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1e-9, 1, 0.2, 0.1),
                                                                      (1e-9, 0.1, 1, 0.2), (1e-9, 0.1, 0.2, 1), (0, 1, 1, 1))]
    for q in qs:
        R = lr.rotation_of(*q)
        back = np.array(lr.quaternion_of(R))
        want = q / np.linalg.norm(q)
        want = -want if (want[0] < 0 or (want[0] == 0 and back @ want < 0)) else want
        assert np.abs(back - want).max() <= 1e-7 if abs(want[0]) < 1e-8 else np.abs(back - want).max() <= 1e-12, q


def test_singletons_and_pass_throughs_keep_their_bits():
    arrs, cell, _ = lr.cases()["pass_through"]
    out = lr.merge(*arrs, cell)
    t = out["totals"]
    assert t["pass"] == 53 and t["clusters"] > 0 and t["merged"] > 0
    big = arrs[1].max(axis=1)
    assert big[3] == F(cell) and out["cluster_of"][3] < t["clusters"]           # exactly the cell: mergeable
    assert out["cluster_of"][4] >= t["clusters"]                                # one float32 above it: passes through
    passed = np.flatnonzero(big > F(cell))
    assert list(out["cluster_of"][passed]) == list(range(t["clusters"], t["clusters"] + t["pass"]))   # behind the clusters, in index order
    names = ("positions", "scales", "quaternions", "opacities", "features_dc", "features_rest")
    for i, r in enumerate(out["cluster_of"]):
        if out["members"][r] == 1:
            for name, src in zip(names, arrs):
                assert out[name][r].tobytes() == src[i].tobytes(), (i, name)
    assert (out["members"][t["clusters"]:] == 1).all() and out["members"].sum() == 257
    arrs, cell, _ = lr.cases()["singletons"]
    out = lr.merge(*arrs, cell)
    assert (out["members"] == 1).all() and out["totals"]["clusters"] == 2000
    for name, src in zip(names, arrs):
        back = np.empty_like(src)
        back[:] = out[name][out["cluster_of"]]
        assert back.tobytes() == src.tobytes(), name


@pytest.mark.parametrize("alpha", [0.2, 0.45, 0.6])
def test_two_identical_gaussians_merge_to_themselves_with_twice_the_opacity(alpha):
    a = lr.random_gaussians(1, 8, seed=12)
    arrs = [np.tile(x, (2,) + (1,) * (x.ndim - 1)) for x in a]
    arrs[3] = np.full(2, alpha, F)
    out = lr.merge(*arrs, 8.0)
    assert out["members"].tolist() == [2] and out["cluster_of"].tolist() == [0, 0]
    assert out["positions"][0].tobytes() == arrs[0][0].tobytes()
    assert out["scales"][0].tobytes() == np.sort(arrs[1][0])[::-1].tobytes()
    assert out["features_dc"][0].tobytes() == arrs[4][0].tobytes() and out["features_rest"][0].tobytes() == arrs[5][0].tobytes()
    assert out["opacities"][0] == F(min(0.99, 2.0 * float(F(alpha))))


def test_mass_is_preserved_where_the_clamp_is_inactive(cluster):
    """alpha' = A / V' in fp64: alpha' V' is A up to the rounding of the quotient and of the product, 2 * 2^-53 A; the float32
    outputs carry four more roundings (alpha' and three scales), each 2^-24 relative."""
    pos, sc, quat, alpha, dc, rest, w = cluster
    pos, alpha = (pos * F(0.01)).astype(F), (alpha * F(0.1)).astype(F)        # a compact, faint cluster: the clamp stays out
    for idx in (range(40), range(3), range(7, 9)):
        mo = lr.moments(idx, pos, sc, quat, alpha, w)
        mu, s, q, al, vol = lr.merged(mo)
        assert lr.ALPHA_LO < al < lr.ALPHA_HI
        assert abs(al * vol - mo["sum_a"]) <= 2.0 ** -51 * mo["sum_a"]
    out = lr.merge(pos, sc, quat, alpha, dc, rest, 8.0)
    got = float(out["opacities"][0]) * float(np.prod(out["scales"][0].astype(np.float64)))
    want = float((alpha.astype(np.float64) * np.prod(sc.astype(np.float64), axis=1)).sum())
    assert abs(got - want) <= 5 * 2.0 ** -24 * want


def test_degenerate_clusters_floor_and_clamp():
    cs = lr.cases()
    out = lr.merge(*cs["collinear_flat"][0], 8.0)
    assert out["scales"][0][2] == F(1e-6) and out["scales"][0][0] > F(0.5)     # the floor: the smallest scale of any member
    out = lr.merge(*cs["identical"][0], 8.0)
    assert out["opacities"][0] == F(0.99)                                       # 63 x 0.6: the clamp
    out = lr.merge(*cs["coincident"][0], 8.0)
    assert out["positions"][0].tobytes() == cs["coincident"][0][0][0].tobytes() and np.isfinite(out["scales"]).all()
    arrs, cell, w = cs["weights_zero"]
    plain = lr.merge(*arrs, cell)
    weighted = lr.merge(*arrs, cell, w)
    rows = np.unique(weighted["cluster_of"][w == 0.0])
    all_zero = [r for r in rows if (w[weighted["cluster_of"] == r] == 0.0).all() and weighted["members"][r] >= 2]
    assert all_zero                                                             # all weights 0: the row of the unweighted merge
    for r in all_zero:
        assert all(weighted[k][r].tobytes() == plain[k][r].tobytes() for k in lr.OUTPUTS[:6])
    assert not lr.same_bits(plain, weighted)


@pytest.mark.parametrize("mutant", ["no_ddT", "reverse"])
def test_the_parity_check_catches_the_mutants(mutant):
    """on the CPU data of the GPU test.  fp64 sums in another order differ by 1e-16, which the one rounding to float32 hides:
    the reversed order shows where large terms cancel (the case made for it)."""
    cs = lr.cases()
    names = {"no_ddT": ("P63_deg1", "P257_deg3", "one_cell_weighted", "pass_through", "weights_zero"),
             "reverse": ("cancelling_colours",)}[mutant]
    for name in names:
        arrs, cell, w = cs[name]
        assert not lr.same_bits(lr.merge(*arrs, cell, w), lr.merge(*arrs, cell, w, mutant=mutant)), name


def test_errors_are_counted_not_clamped():
    arrs, cell, _ = lr.cases()["P65_deg1"]
    pos = arrs[0].copy()
    pos[7, 1] = np.nan
    sc = arrs[1].copy()
    sc[9, 0] = np.inf
    sc[7, 2] = np.inf
    assert lr.merge(pos, sc, *arrs[2:], cell)["totals"]["nonfinite"] == 2
    assert lr.merge(*arrs, 4.0 / 1100.0)["totals"]["over"] > 0


def test_library_and_binding_list_the_entry_points():
    from binocular3dgs_amd import _C, _lib
    assert _lib.lib().b3gs_abi_version() == _lib.ABI_VERSION == _C.ABI_VERSION == 18
    for name in ("b3gs_gaussian_merge_workspace_bytes", "b3gs_gaussian_merge_count", "b3gs_gaussian_merge_emit"):
        assert name in _lib.EXPORTS
    assert callable(_C.gaussian_merge_count) and callable(_C.gaussian_merge_emit)


def test_entry_points_refuse_bad_arguments_without_touching_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 255) & ~255                                   # a host address: never dereferenced by a refused call
    count, emit, size = L.b3gs_gaussian_merge_count, L.b3gs_gaussian_merge_emit, L.b3gs_gaussian_merge_workspace_bytes
    ok = (4, 3, p, p, p, p, p, p, None, 1.0, p, None)
    names = ("P", "K", "pos", "scale", "quat", "alpha", "dc", "rest", "w", "cell", "ws", "stream")

    def with_(**kw):
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for kw in ({"P": -1}, {"P": 2 ** 24}, {"K": 4}, {"K": -1}, {"cell": 0.0}, {"cell": -1.0}, {"cell": float("nan")}, {"cell": float("inf")},
               {"ws": None}, {"ws": p + 8}, {"pos": None}, {"scale": None}, {"quat": None}, {"alpha": None}, {"dc": None}, {"rest": None}):
        assert count(*with_(**kw)) == ERR_ARG, kw
    assert count(*with_(cell=0.0)) == ERR_ARG and b"cell" in L.b3gs_last_error()
    totals = (C.c_int64 * 5)(1, 0, 0, 0, 0)
    outs = (p,) * 8
    assert emit(*ok[:11], None, *outs, None) == ERR_ARG                    # no totals
    totals[3] = 3
    assert emit(*ok[:11], totals, *outs, None) == ERR_ARG and b"3 rows hold a value that is not finite" in L.b3gs_last_error()
    totals[3], totals[4] = 0, 2
    assert emit(*ok[:11], totals, *outs, None) == ERR_ARG and b"2 rows lie beyond the 1024 cells" in L.b3gs_last_error()
    totals[4], totals[0] = 0, 5
    assert emit(*ok[:11], totals, *outs, None) == ERR_ARG                  # more rows than Gaussians
    totals[0] = 0
    assert emit(*ok[:11], totals, *outs, None) == ERR_ARG                  # no row for four Gaussians
    totals[0] = 2
    for k in range(8):
        assert emit(*ok[:11], totals, *(outs[:k] + (None,) + outs[k + 1:]), None) == ERR_ARG, k
    assert size(-1, 0) == 0 and size(2 ** 24, 0) == 0 and size(10, 5) == 0
    assert size(0, 0) % 256 == 0 and 0 < size(0, 0) < size(1000, 15) and size(1000, 15) % 256 == 0
