"""The numpy yardstick of the screened Poisson reconstruction (tests/poisson_ref.py) reconstructs: analytic shapes come back as
closed surfaces at the right place, the trim opens what no sample supports, and two mutants -- the operator without its screening
term, a dot product folded in another order -- fail the checks the yardstick passes.  No GPU: the device is held against this
yardstick bit for bit by tests/test_gpu_poisson.py."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402
import poisson_ref as pr  # noqa: E402

F = np.float32
# mean |radius error| of the sphere case below, in voxels, as measured with this yardstick (INTEGRATION.md section 27 records it)
SPHERE_MEAN_ERROR = 0.0171
MARGIN = 0.5
SPREAD, TRIM = 1, 0.5


def _pinned_cloud(n=700, seed=11):
    """Points of a sphere of radius 5 voxels around the middle of a 20 x 17 x 13 grid (18 partials: not a power of two, so
    reversing them is another tree), made with + - * / sqrt only (the digest below
    must not depend on a libm): uniform points of a cube, those inside a shell, pushed onto the sphere."""
    rng = np.random.default_rng(seed)
    q = rng.random((8 * n, 3)) * 2.0 - 1.0
    r = np.sqrt((q * q).sum(axis=1))
    q = q[(r > 0.3) & (r < 1.0)][:n]
    nrm = q / np.sqrt((q * q).sum(axis=1))[:, None]
    return (nrm * 5.0 + np.array([10.0, 8.5, 6.5])).astype(F), nrm.astype(F), (0.5 + 0.5 * rng.random(len(q))).astype(F)


def _digest(sol, trace):
    """of the solution's float32 words and of the float64 sums b.b, per iteration p.Ap and r.r, and sum(D x) (the step scalars are rounded
    to float32 before they reach x, which hides most last-bit changes of a sum: the float64 words show them)"""
    return hashlib.sha256(np.ascontiguousarray(sol["x"], F).tobytes() + np.array([sol["bb"]] + trace, np.float64).tobytes()).hexdigest()[:16]


PINNED_DIGEST = "19388687e29e68a3"


def _sphere_checks(**mutant):
    """-> the named checks of the sphere case and of the pinned cloud, True where one passes"""
    case = pr.sphere_case(3000, 32, 4)
    v, _, f, info = pr.reconstruct(case["points"], case["normals"], case["weights"], case["dims"], case["origin"], case["voxel"],
                                   spread=SPREAD, min_weight=0.0, **mutant)
    _, uses = mr.edge_uses(f)
    err = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).mean() / case["voxel"]) if len(v) else float("inf")
    p, n, w = _pinned_cloud()
    density, vector, dropped = pr.splat(p, n, w, (20, 17, 13), (0.0, 0.0, 0.0), 1.0)
    trace = []
    sol = pr.solve(density, vector, 4.0, 24, 0.0, len(p) - dropped, mutant.get("screening", True), mutant.get("fold_order", "linear"), trace=trace)
    # the numerator of the level, sum(D x): x changes sign, so this sum cancels and shows the order it was made in
    trace.append(float(pr.dot(density, sol["x"], mutant.get("fold_order", "linear"))))
    print(f"sphere: {len(v)} vertices, {len(f)} triangles, {info['iterations']} iterations, residual {np.sqrt(info['rr'] / info['bb']):.3e}, "
          f"mean |radius error| {err:.4f} voxels, pinned digest {_digest(sol, trace)} {mutant}")
    # the issue's own statement about the operator: symmetric positive DEFINITE, i.e. a constant is not in its kernel
    ones = np.ones_like(density)
    definite = float((pr.apply(density, 4.0, ones, mutant.get("screening", True)).astype(np.float64) * ones).sum()) > 0.0
    return {"definite": definite, "closed": len(f) > 0 and bool((uses == 2).all()), "euler": len(f) > 0 and mr.euler_characteristic(len(v), f) == 2,
            "radius": err <= SPHERE_MEAN_ERROR + MARGIN, "converged": bool(info["done"]),
            "bits": _digest(sol, trace) == PINNED_DIGEST}, err


def test_sphere_is_closed_and_at_the_right_radius():
    checks, err = _sphere_checks()
    assert all(checks.values()), checks
    assert abs(err - SPHERE_MEAN_ERROR) < 5e-4, f"the recorded value {SPHERE_MEAN_ERROR} is stale: measured {err:.4f}"


def test_hemisphere_closes_at_zero_and_opens_at_a_positive_trim():
    """The half z >= 0 of a sphere of radius 12 voxels, 8 voxels of room around it: untrimmed, the level set closes under the
    dome; trimmed, only what the samples support remains, no vertex farther than SPREAD + 1 voxels from a sample."""
    case = pr.sphere_case(2000, 24, 8)
    sel = case["points"][:, 2] >= 0
    p, n, w = case["points"][sel], case["normals"][sel], case["weights"][sel]
    v, _, f, _ = pr.reconstruct(p, n, w, case["dims"], case["origin"], case["voxel"], spread=SPREAD, min_weight=0.0)
    _, uses = mr.edge_uses(f)
    assert (uses == 2).all() and mr.euler_characteristic(len(v), f) == 2
    assert v[:, 2].min() < -2 * case["voxel"]                       # (the closing cap lies where no sample is)
    v, _, f, _ = pr.reconstruct(p, n, w, case["dims"], case["origin"], case["voxel"], spread=SPREAD, min_weight=TRIM)
    _, uses = mr.edge_uses(f)
    assert len(f) > 1000 and (uses == 1).any() and uses.max() == 2
    far = 0.0
    for k in range(0, len(v), 512):                                  # brute force, in blocks
        d = np.sqrt(((v[k:k + 512, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)) ** 2).sum(-1)).min(axis=1)
        far = max(far, float(d.max()))
    print(f"hemisphere at trim {TRIM}: {len(v)} vertices, farthest from a sample {far / case['voxel']:.3f} voxels")
    assert far <= (SPREAD + 1) * case["voxel"]


@pytest.mark.parametrize("mutant", [{"screening": False}, {"fold_order": "reversed"}], ids=["no_screening", "other_fold_order"])
def test_mutants_fail_the_checks(mutant):
    """Both mutants still give a closed sphere (the unscreened one at nearly twice the radius error, 0.0305 voxels, far inside
    the issue's margin of one half).  The unscreened operator is caught numerically: 1^T A 1 = 0, it is not definite.  A fold in
    another order is a change of the last bit of a float64 sum by nature: only the bit check can see it."""
    checks, _ = _sphere_checks(**mutant)
    assert not all(checks.values()), checks
    assert not checks["bits"]
    assert checks["definite"] == ("screening" not in mutant)


def test_fold_order_and_partials_are_the_stated_trees():
    rng = np.random.default_rng(0)
    q = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    part = pr.partials(q)
    assert len(part) == 4
    lane = np.zeros(256)
    lane[:232] = q[768:]
    w = [None] * 4
    for k in range(4):                                               # the butterfly of one wave, written out as a tree
        a = lane[64 * k:64 * k + 64].copy()
        for d in (32, 16, 8, 4, 2, 1):
            a = a[:d] + a[d:2 * d]
        w[k] = a[0]
    assert part[3] == (w[0] + w[1]) + (w[2] + w[3])
    many = rng.standard_normal(200)
    want = np.zeros(64)
    for k, value in enumerate(many):
        want[k % 64] = want[k % 64] + value
    for d in (32, 16, 8, 4, 2, 1):
        want = want[:d] + want[d:2 * d]
    assert pr.fold(many) == want[0]
    assert abs(pr.fold(many) - many.sum()) < 1e-12
    order = np.zeros(129)
    order[[0, 64, 128]] = 1.0, 1e16, -1e16                           # one lane: (1 + 1e16) - 1e16 = 0, but (-1e16 + 1e16) + 1 = 1
    assert pr.fold(order) == 0.0 and pr.fold(order, "reversed") == 1.0


def test_operator_is_symmetric_and_positive():
    rng = np.random.default_rng(1)
    dims = (7, 5, 4)
    density = (rng.random(dims[::-1]) * (rng.random(dims[::-1]) < 0.3)).astype(F)
    x, y = rng.standard_normal(dims[::-1]).astype(F), rng.standard_normal(dims[::-1]).astype(F)
    ax, ay = pr.apply(density, 4.0, x).astype(np.float64), pr.apply(density, 4.0, y).astype(np.float64)
    assert abs((ax * y).sum() - (ay * x).sum()) < 1e-3 and (ax * x).sum() > 0
    ones = np.ones(dims[::-1], F)
    assert np.array_equal(pr.apply(density, 4.0, ones), F(4.0) * density)              # Neumann: constants see the screen only
    assert np.array_equal(pr.apply(density, 4.0, ones, screening=False), np.zeros(dims[::-1], F))
