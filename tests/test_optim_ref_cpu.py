"""CPU: the Adam yardstick of tests/optim_ref.py is right, and the bounds of tests/test_gpu_adam_edges.py come from it.

(i) optim_ref.adam_step equals torch.optim.Adam(eps=1e-15) on CPU float64 tensors to 1e-12 relative: several steps, six
groups with their own learning rate, step numbers up to 30 000 (the state's `step` seeded); (ii) both decay orders equal
the torch statements of the reference's train.py:171-173 in float64; (iii) decay_in / decay_out of tests/golden/densify.npz
are reproduced to the fixture's own float32 rounding; (iv) the float32 noise of the formula: optim_ref.adam_step_f32 (one
rounding per operation, the kernel's order) against float64 on the exact inputs of the GPU tests (optim_ref.CASES), per
quantity; 10 x the largest 99th percentile is the GPU bound (optim_ref.GPU_BOUNDS, the convention of
tests/test_gpu_grad_edges.py)."""
import os

import numpy as np
import pytest
import torch

import optim_ref as R

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("t0", [0, 9, 999, 29997])
def test_float64_restatement_equals_torch_adam_in_float64(t0):
    rng = np.random.default_rng(t0)
    shapes = [(50, 3), (50, 1, 3), (50, 15, 3), (50, 3), (50, 4), (50, 1)]
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s))) for s in shapes]
    opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(ps, R.MODEL_LRS)], eps=1e-15)
    mine = []
    for p in ps:
        m, v = R.warm_state(rng, p.numel())
        m, v = m.astype(np.float64).reshape(p.shape), v.astype(np.float64).reshape(p.shape)
        if t0:
            opt.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": torch.from_numpy(m.copy()),
                            "exp_avg_sq": torch.from_numpy(v.copy())}
        else:
            m, v = np.zeros_like(m), np.zeros_like(v)
        mine.append([p.detach().numpy().copy(), m, v])
    for s in range(3):
        for k, p in enumerate(ps):
            g = R.gradients(rng, p.numel()).astype(np.float64).reshape(p.shape)
            # (signs follow the running mean: a relative bound on m' = 0.9 m + 0.1 g means nothing where the two cancel)
            g = np.where(mine[k][1] != 0, np.abs(g) * np.sign(mine[k][1]), g)
            p.grad = torch.from_numpy(g.copy())
            mine[k][0], mine[k][1], mine[k][2], _ = R.adam_step(mine[k][0], g, mine[k][1], mine[k][2], R.MODEL_LRS[k], t0 + s + 1)
        opt.step()
    for k, p in enumerate(ps):
        st = opt.state[p]
        assert float(st["step"]) == t0 + 3
        for got, ref in ((mine[k][0], p.detach().numpy()), (mine[k][1], st["exp_avg"].numpy()), (mine[k][2], st["exp_avg_sq"].numpy())):
            np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("decay_first", [False, True])
def test_both_decay_orders_equal_the_torch_statements(decay_first):
    """train.py:171-173 decays `_opacity.data` before optimizer.step() (decay_first); the other order is the same two
    statements swapped."""
    rng = np.random.default_rng(5)
    n = 512
    o = torch.nn.Parameter(torch.from_numpy(R.opacity_logits(rng, n).astype(np.float64)))
    m, v = (x.astype(np.float64) for x in R.warm_state(rng, n))
    g = R.gradients(rng, n).astype(np.float64)
    opt = torch.optim.Adam([{"params": [o], "lr": 0.05}], eps=1e-15)
    opt.state[o] = {"step": torch.tensor(6.0), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    o.grad = torch.from_numpy(g.copy())
    p0 = o.detach().numpy().copy()

    def decay():
        with torch.no_grad():
            op = torch.sigmoid(o) * 0.995          # gaussians.opacity_decay(factor): get_opacity * factor ...
            o.data = torch.log(op / (1 - op))      # ... through inverse_sigmoid
    if decay_first:
        decay()
        opt.step()
    else:
        opt.step()
        decay()
    got, m2, v2, _ = R.adam_step(p0, g, m, v, 0.05, 7, decay=0.995, decay_sel=np.ones(n, bool), decay_first=decay_first)
    np.testing.assert_allclose(got, o.detach().numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(m2, opt.state[o]["exp_avg"].numpy(), rtol=1e-12)
    # decay = 0 with a selected segment: no decay
    plain, _, _, _ = R.adam_step(p0, g, m, v, 0.05, 7, decay=0.0, decay_sel=np.ones(n, bool))
    np.testing.assert_array_equal(plain, R.adam_step(p0, g, m, v, 0.05, 7)[0])


def test_decay_fixture_of_the_reference_is_reproduced():
    g = np.load(os.path.join(GOLD, "densify.npz"))
    ref = g["decay_out"]
    got = R.logit_decay(g["decay_in"], 0.995)
    # the fixture holds the float32 result of float32 torch statements: its own rounding is what separates it from float64
    f32 = R.logit_decay_f32(g["decay_in"], 0.995)
    own = np.abs(f32.astype(np.float64) - got).max()
    err = np.abs(ref - got)
    print(f"decay fixture: max |fixture - float64| {err.max():.2e}, float32 restatement against float64 {own:.2e}")
    assert err.max() <= 4 * own + np.spacing(np.abs(ref).max())


def test_row_mask_and_float32_restatement_are_consistent():
    c = R.mask_case(63)
    nan_g = np.where(c["live"], c["g"], np.float32("nan"))
    a = R.reference(c, g=nan_g)
    b = R.reference(c, g=np.where(c["live"], c["g"], 0).astype(np.float32))
    for x, y in zip(a, b):
        assert np.array_equal(x, y) and not np.isnan(x).any()
    a32 = R.reference(c, g=nan_g, f32=True)
    assert all(x.dtype == np.float32 and not np.isnan(x).any() for x in a32)


def test_float32_noise_of_the_formula_gives_the_gpu_bounds():
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    rows = []
    for name, build in R.CASES.items():
        e = R.measure(build())
        p99 = {k: float(np.percentile(x, 99)) for k, x in e.items()}
        rows.append((name, e, p99))
        print(f"{name:18s} n {e['p'].size:8d}  p99 / max:  m {p99['m']:.2e} / {e['m'].max():.2e}   v {p99['v']:.2e} / "
              f"{e['v'].max():.2e}   p {p99['p']:.2f} / {e['p'].max():.1f} ulp")
        for k in worst:
            worst[k] = max(worst[k], p99[k])
    bounds = {k: 10.0 * x for k, x in worst.items()}
    print("largest 99th percentile:", {k: f"{x:.3e}" for k, x in worst.items()})
    print("GPU bounds (10 x):      ", {k: f"{x:.3e}" for k, x in bounds.items()}, " recorded:", R.GPU_BOUNDS)
    for k, b in bounds.items():
        # the recorded figure is the measured one rounded up to three digits
        assert b <= R.GPU_BOUNDS[k] <= 1.06 * b, (k, b, R.GPU_BOUNDS[k])
    # the criterion can be met: the float32 restatement itself stays within it on every case
    for name, e, _ in rows:
        for k, x in e.items():
            assert np.isfinite(x).all(), (name, k)
            assert float((x > R.GPU_BOUNDS[k]).mean()) <= R.TAIL, (name, k, float((x > R.GPU_BOUNDS[k]).mean()))
