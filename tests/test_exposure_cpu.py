"""CPU: the exposure yardstick (tests/exposure_ref.py) against independent statements -- torch float64 autograd, numpy lstsq,
torch.optim.Adam --, the trainers' call order with a stand-in term, the rules between the train flags and exposure.json."""
import json
import types

import numpy as np
import pytest
import torch

import exposure_ref as ref
import test_graph_trainer_cpu as g
from binocular3dgs_amd.graph_trainer import GraphTrainer
from binocular3dgs_amd.schedule import IterationSchedule


def _rand(seed, W, H):
    rng = np.random.default_rng(seed)
    return (rng.random((3, H, W), dtype=np.float32), (rng.standard_normal((3, H, W)) * 0.1).astype(np.float32),
            (np.eye(3, 4) + rng.standard_normal((3, 4)) * 0.2).astype(np.float32))


@pytest.mark.parametrize("W,H", [(1, 1), (16, 16), (257, 1), (37, 29), (64, 40)])
def test_backward_of_the_yardstick_is_the_gradient_of_the_plain_statement(W, H):
    """g_in and G against torch float64 autograd of out_c = t_c + sum_k a_ck x_k over TWO planes that share A.  Bound per sum
    of n terms: n 2^-52 sum |terms| (every addition of either order is within 2^-53 of exact, relative to the partial sums,
    which the sum of the magnitudes bounds)."""
    (i0, g0, A), (i1, g1, _) = _rand(W + 1000 * H, W, H), _rand(W + 1000 * H + 1, W, H)
    g_ins, G = ref.backward([i0, i1], [g0, g1], A)
    At = torch.tensor(A, dtype=torch.float64, requires_grad=True)
    xs = [torch.tensor(i, dtype=torch.float64, requires_grad=True) for i in (i0, i1)]
    total = 0.0
    for x, go in zip(xs, (g0, g1)):
        out = At[:, 3, None, None] + torch.einsum("ck,khw->chw", At[:, :3], x)
        total = total + (out * torch.tensor(go, dtype=torch.float64)).sum()
    total.backward()
    for x, gi in zip(xs, g_ins):
        terms = np.abs(A[:, :3].astype(np.float64)).sum(0)[:, None, None] * np.abs(np.stack([g0, g1])).max()
        bound = 3 * 2.0 ** -52 * terms + np.abs(x.grad.numpy()) * 2.0 ** -24          # + the one rounding to float32
        assert (np.abs(gi.astype(np.float64) - x.grad.numpy()) <= bound).all()
    n = 2 * W * H
    mags = np.zeros((3, 4))
    for i, go in ((i0, g0), (i1, g1)):
        x4 = np.concatenate([i.astype(np.float64), np.ones((1, H, W))])
        mags += np.einsum("chw,khw->ck", np.abs(go.astype(np.float64)), np.abs(x4))
    bound = n * 2.0 ** -52 * mags
    assert (np.abs(G - At.grad.numpy()) <= bound).all(), (np.abs(G - At.grad.numpy()) / bound).max()
    _, mut = ref.backward([i0, i1], [g0, g1], A, mutant="no_bias")
    assert not (np.abs(mut - At.grad.numpy()) <= bound).all()
    if W * H > 1:
        (m0, _), _ = ref.backward([i0, i1], [g0, g1], A, mutant="transposed")
        assert not np.array_equal(m0, g_ins[0])


def test_apply_of_the_yardstick_is_the_plain_statement():
    image, _, A = _rand(3, 37, 29)
    want = A[:, 3, None, None].astype(np.float64) + np.einsum("ck,khw->chw", A[:, :3].astype(np.float64), image.astype(np.float64))
    got = ref.apply(image, A)
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 4 * 2.0 ** -52 * 4 + np.abs(want).max() * 2.0 ** -24
    assert np.array_equal(ref.apply(image, ref.IDENTITY), image)


@pytest.mark.parametrize("seed,masked", [(0, False), (1, True)])
def test_fit_of_the_yardstick_against_lstsq(seed, masked):
    """The unrounded Cholesky solution within 64 cond(S) 2^-53 |A| of numpy.linalg.lstsq on the same float64 sums' pixels;
    the inputs are seeded so that cond(S) < 1e4 (asserted)."""
    rng = np.random.default_rng(seed)
    W, H = 64, 40
    render = rng.random((3, H, W), dtype=np.float32)
    A_true = (np.eye(3, 4) * 1.3 + rng.standard_normal((3, 4)) * 0.1).astype(np.float32)
    gt = ref.apply(render, A_true) + (rng.standard_normal((3, H, W)) * 0.02).astype(np.float32)
    mask = (rng.random((H, W)) > 0.3).astype(np.uint8) if masked else None
    A, flag, sums = ref.fit(render, gt, mask)
    S, B = ref.matrix_of_sums(sums)
    cond = np.linalg.cond(S)
    assert cond < 1e4 and flag == 0
    used = np.ones(H * W, bool) if mask is None else mask.reshape(-1) != 0
    X = np.concatenate([render.reshape(3, -1).astype(np.float64), np.ones((1, H * W))]).T[used]
    want = np.linalg.lstsq(X, gt.reshape(3, -1).astype(np.float64).T[used], rcond=None)[0].T          # [3, 4]
    exact = ref.solve(sums, rounded=False)[0]
    bound = 64 * cond * 2.0 ** -53 * np.linalg.norm(want)
    assert np.abs(exact - want).max() <= bound, (np.abs(exact - want).max(), bound)
    assert np.array_equal(A, exact.astype(np.float32))
    assert sums[0] == used.sum() == sums[10]


def test_fit_degeneracy_is_the_identity_and_the_flag():
    c = np.full((3, 29, 37), 0.25, np.float32)
    A, flag, _ = ref.fit(c, c * 2)
    assert flag == 1 and np.array_equal(A, ref.IDENTITY)
    rng = np.random.default_rng(2)
    render = rng.random((3, 40, 64), dtype=np.float32)
    mask = np.zeros((40, 64), np.uint8)
    mask.reshape(-1)[::180] = 1
    assert mask.sum() == 15
    A, flag, sums = ref.fit(render, render * 0.5, mask)
    assert flag == 1 and sums[0] == 15 and np.array_equal(A, ref.IDENTITY)
    mask.reshape(-1)[1] = 1
    A, flag, sums = ref.fit(render, render * 0.5, mask)
    assert flag == 0 and sums[0] == 16 and np.abs(A - 0.5 * ref.IDENTITY).max() < 1e-5


def test_row_sparse_adam_against_torch_adam():
    """One row against torch.optim.Adam on a single 12-vector for 5 steps: 8 * 2^-24 relative (torch works in float32, the
    yardstick rounds once); the other row keeps its bits."""
    rng = np.random.default_rng(4)
    state = ref.new_state(2)
    state["table"][0] = rng.standard_normal((3, 4)).astype(np.float32)
    # (entries of 0.5 .. 1.5: five steps of about 0.01 cancel nothing, so "relative" is relative to the entry itself)
    state["table"][1] = (0.5 + rng.random((3, 4))).astype(np.float32)
    keep = {k: v[0].copy() for k, v in state.items()}
    p = torch.nn.Parameter(torch.tensor(state["table"][1].reshape(-1)))
    opt = torch.optim.Adam([p], lr=0.01, betas=(0.9, 0.999), eps=1e-8)
    for _ in range(5):
        grad = (rng.standard_normal(12) * 0.3).astype(np.float32)
        p.grad = torch.tensor(grad)
        opt.step()
        state = ref.adam(state, 1, grad.astype(np.float64), 0.01, 0.9, 0.999, 1e-8)
        got, want = state["table"][1].reshape(-1).astype(np.float64), p.detach().numpy().astype(np.float64)
        assert (np.abs(got - want) <= 8 * 2.0 ** -24 * np.abs(want)).all(), np.abs(got / want - 1).max()
    assert state["steps"].tolist() == [0, 5] and abs(state["prods"][1, 0] - 0.9 ** 5) < 1e-15
    for k, v in keep.items():
        assert np.array_equal(state[k][0], v), k
    same = ref.adam(state, 1, np.ones(12), 0.01, skip=1)
    assert all(np.array_equal(same[k], state[k]) for k in state)


# ---- the trainers' call order ---------------------------------------------------------------------------------------------
class _Term:
    def __init__(self, log, from_iter=0):
        self.log, self.from_iter = log, from_iter

    def active(self, it):
        return it >= self.from_iter

    def apply(self, view_index, *images):
        self.log.append(f"exposure:{view_index}:{len(images)}")
        out = [x * 0.5 for x in images]
        return out[0] if len(out) == 1 else out

    def step(self, it):
        self.log.append("exposure_adam")


class _LoggedSchedule(IterationSchedule):
    """the term needs the run's log: _schedule_run builds it, the model the run hands over carries it"""
    def __init__(self, model, *a, from_iter=0, **kw):
        super().__init__(model, *a, exposure=_Term(model.log, from_iter), **kw)


def test_without_the_term_both_trainers_do_what_they_did():
    draws = g._draws()
    assert g._schedule_run(draws, exposure=None) == g._schedule_run(draws)
    tr, _, events, got = g._graph_run(draws)
    assert tr.exposure is None and all(len(e["key"]) == 4 for e in events if "key" in e)
    totals = {}
    g._schedule_run(draws, seen=lambda it, s, total: totals.setdefault(it, float(total.detach())))
    assert len(totals) == len(draws)


def test_the_schedule_applies_before_the_loss_and_steps_after_the_optimiser():
    draws = g._draws()
    plain, plain_totals, totals = g._schedule_run(draws), {}, {}
    g._schedule_run(draws, seen=lambda it, s, total: plain_totals.setdefault(it, float(total.detach())))
    got = g._schedule_run(draws, cls=_LoggedSchedule, from_iter=5, seen=lambda it, s, total: totals.setdefault(it, float(total.detach())))
    last = g.CFG["iterations"]
    for it, view, shift in draws:
        ev = got[it]
        assert [e for e in ev if not e.startswith("exposure")] == plain[it], it
        if it < 5:
            assert ev == plain[it] and totals[it] == plain_totals[it]
            continue
        n = 2 if shift is not None else 1
        assert ev.count(f"exposure:{view}:{n}") == 1 and sum(e.startswith("exposure:") for e in ev) == 1
        at = ev.index(f"exposure:{view}:{n}")
        assert at == ev.index("render:shifted") + 1 if n == 2 else at == ev.index(f"render:{view}") + 1
        assert totals[it] != plain_totals[it]                      # the loss read the image the term returned
        if "densify" in ev or it == last:
            assert "exposure_adam" not in ev, (it, ev)
        else:
            assert ev[-1 if "checkpoint" not in ev else -2] == "exposure_adam" and ev.index("adam") < ev.index("exposure_adam"), (it, ev)


def test_the_graph_trainer_grows_its_key_only_while_the_term_is_active():
    log, cams = [], [g._Cam(k) for k in range(3)]
    backend = g._Backend(log, cams)
    backend.has_exposure = True
    events = []
    tr = GraphTrainer(g._Model(log), g._Scene(cams), None, torch.zeros(3), backend=backend, events=events, test_cameras=[],
                      exposure=_Term(log, from_iter=5), **g.CFG)
    for it, view, shift in g._draws():
        tr.run_iteration(it, view, shift)
    tr.settle()
    for e in events:
        if "key" in e:
            assert (e["key"][-1] == "exposure") == (e["it"] >= 5) and len(e["key"]) == (5 if e["it"] >= 5 else 4), e
    caps = [e["key"] for e in events if e["event"] == "capture"]
    assert len(caps) == len(set((k, e["it"]) for e in events if e["event"] == "capture" for k in [e["key"]]))


# ---- flags and files -------------------------------------------------------------------------------------------------------
def test_check_args_rules():
    from binocular3dgs_amd import train
    p = train.parser()
    train.check_args(p.parse_args(["-s", "x"]))
    train.check_args(p.parse_args(["-s", "x", "--exposure", "--exposure_lr_init", "0.02", "--exposure_from", "100"]))
    train.check_args(p.parse_args(["-s", "x", "--exposure", "--step", "graph"]))
    train.check_args(p.parse_args(["-s", "x", "--exposure", "--densify", "mcmc", "--cap_max", "1000"]))
    for bad in (["--exposure_from", "5"], ["--exposure_lr_init", "0.02"], ["--exposure", "--exposure_lr_final", "0"],
                ["--exposure", "--exposure_from", "-1"]):
        with pytest.raises(ValueError, match="exposure"):
            train.check_args(p.parse_args(["-s", "x", *bad]))
    assert train.exposure_sidecar("/m/chkpnt30.pth") == "/m/chkpnt30.exposure.pth"


def test_exposure_json_round_trip_and_term_state(tmp_path):
    from binocular3dgs_amd.exposure import ExposureTerm, read_matrices, write_matrices
    term = ExposureTerm(["a.png", "b.png"], device="cpu", iterations=100)
    assert term.lr(0) == pytest.approx(0.01) and term.lr(100) == pytest.approx(0.001) and term.lr(50) == pytest.approx(10 ** -2.5)
    assert not ExposureTerm(["a"], device="cpu", from_iter=7).active(6)
    term.table[1] = torch.arange(12, dtype=torch.float32).reshape(3, 4) / 7
    term.steps[1] = 3
    path = tmp_path / "exposure.json"
    write_matrices(str(path), term.matrices())
    raw = json.load(open(path))
    assert sorted(raw) == ["a.png", "b.png"] and np.asarray(raw["a.png"]).shape == (3, 4)
    back = read_matrices(str(path))
    assert torch.equal(back["b.png"], term.table[1]) and torch.equal(back["a.png"], torch.eye(3, 4))
    other = ExposureTerm(["c.png", "b.png"], device="cpu")
    other.load_state_dict(term.state_dict())
    assert torch.equal(other.table[1], term.table[1]) and int(other.steps[1]) == 3
    assert torch.equal(other.table[0], torch.eye(3, 4)) and int(other.steps[0]) == 0
