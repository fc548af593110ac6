"""CPU: the input sets of tests/densify_edges.py hold every decision edge and no fragile decision -- tests/densify_ref.py takes
the same keep / clone / child decisions in float32 and in float64 on every set (a condition, not a tolerance: no Gaussian is
left out of the GPU comparison) -- and the float32 noise of the children (xyz' = R(q/|q|)(s * noise) + xyz, scaling' =
log(s / 1.6)) gives the bounds of tests/test_gpu_densify_edges.py."""
import numpy as np
import pytest
import torch

import densify_edges as E


@pytest.mark.parametrize("P,M,size", E.SETS)
def test_no_fragile_decision_and_every_class_is_populated(P, M, size):
    d = E.build(P, M, size)
    r32, r64 = E.run_ref(d, torch.float32), E.run_ref(d, torch.float64)
    for a, b, name in zip(r32[4:], r64[4:], ("keep", "clone", "child")):
        assert np.array_equal(a, b), name
    assert np.array_equal(r32[3], r64[3])
    keep, clone, child = r64[4:]
    pop = E.populations(d, keep, clone, child)
    print(f"P {P} M {M} max_screen_size {size}: kept {int(keep.sum())} clones {int(clone.sum())} split {int(child.sum())} {pop}")
    if P >= 255:
        assert all(n >= 8 for n in pop.values()), pop
    # copies are copies in either precision
    for k in E.NAMES:
        rows = ~E.child_rows(r64[3], keep, clone) if k in ("xyz", "scaling") else np.ones(len(r64[3]), bool)
        assert np.array_equal(r32[0][k][rows], d["params"][k][r32[3]][rows]), k


@pytest.mark.parametrize("kind", ["all_pruned", "unchanged"])
def test_degenerate_sets(kind):
    d = E.degenerate(kind)
    for dt in (torch.float32, torch.float64):
        _, _, _, order, keep, clone, child = E.run_ref(d, dt)
        assert not clone.any() and not child.any()
        assert (len(order) == 0) if kind == "all_pruned" else np.array_equal(order, np.arange(d["P"]))


def test_float32_noise_of_the_children_gives_the_gpu_bounds():
    worst = {"xyz": 0.0, "scaling": 0.0}
    for P, M, size in E.SETS:
        d = E.build(P, M, size)
        r32, r64 = E.run_ref(d, torch.float32), E.run_ref(d, torch.float64)
        rows = E.child_rows(r64[3], r64[4], r64[5])
        if not rows.any():
            continue
        for k in worst:
            e = E.child_err(r32[0][k], r64[0][k], rows)
            print(f"P {P} M {M} size {size} {k}: {e.size} values, p99 {np.percentile(e, 99):.2e} max {e.max():.2e}")
            worst[k] = max(worst[k], float(np.percentile(e, 99)))
    bounds = {k: 10 * x for k, x in worst.items()}
    print("largest 99th percentile:", worst, " GPU bounds (10 x):", bounds, " recorded:", E.GPU_BOUNDS)
    for k, b in bounds.items():      # the recorded figure is the larger of two hosts' measurements (densify_edges.GPU_BOUNDS)
        assert 0.75 * E.GPU_BOUNDS[k] <= b <= 1.1 * E.GPU_BOUNDS[k], (k, b, E.GPU_BOUNDS[k])
