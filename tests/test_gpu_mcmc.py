"""GPU: binocular3dgs_amd/mcmc.py (csrc/mcmc.hip) against tests/mcmc_ref.py.

  * Philox words bit for bit; normals within 4 float32 ulp of the float64 Box-Muller, and standard over 2^20 samples;
  * relocation: src, count, dead ranks and the weight scan bit for bit over the shapes at the wave edges, the seams of the scans
    and the structural cases; copied rows bit for bit, untouched rows untouched, new raw opacities / scales within 1 float32 ulp
    of the float64 value rounded once, moments of written rows zero; both mutants of the yardstick rejected;
  * noise: drawn in registers == handed in, bound against float64, opaque rows do not move;
  * grow: the rule of new_P, the old rows, the optimiser state of optim.Adam and step.FusedAdam;
  * 300 iterations of McmcSchedule on the synthetic scene of the graph-trainer tests."""
import math
import types

import numpy as np
import pytest
import torch

import mcmc_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF1
CASES = {name: (dead, draws) for name, dead, draws in ref.relocation_cases()}
_REF = {}


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _model(rows):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    return GaussianModel.from_tensors(*[torch.from_numpy(np.ascontiguousarray(a)) for a in rows], sh_degree=1, device="cuda")


def _fused_adam(model, seed=5):
    """step.FusedAdam over the six tensors with NONZERO moments"""
    from binocular3dgs_amd.step import FusedAdam
    opt = FusedAdam(model.parameters(), [1e-3] * 6)
    g = torch.Generator(device="cuda").manual_seed(seed)
    opt.exp_avg.copy_(torch.rand(opt.exp_avg.shape, device="cuda", generator=g) + 0.5)
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, device="cuda", generator=g) + 0.5)
    return opt


def _yardstick(name, mutant=None):
    key = (name, mutant)
    if key not in _REF:
        dead, draws = CASES[name]
        rows = ref.make_rows(dead.shape[0], dead, seed=3)
        _REF[key] = (rows, ref.relocate_ref(rows, seed=SEED, offset=150, draws=draws, mutant=mutant))
    return _REF[key]


def _relocate_on_device(name):
    from binocular3dgs_amd import mcmc
    dead, draws = CASES[name]
    rows, _ = _yardstick(name)
    P = dead.shape[0]
    model = _model(rows)
    opt = _fused_adam(model)
    m0, v0 = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    d = None
    if draws is not None:
        full = np.zeros(P, dtype=np.uint64)
        full[:len(draws)] = np.array(draws, dtype=np.uint64)
        d = torch.from_numpy(full.view(np.int64)).cuda()
    src, count, rank, wsum, head = mcmc.relocate(model, opt, iteration=150, seed=SEED, debug=True, draws=d)
    torch.cuda.synchronize()
    got = dict(src=src.cpu().numpy().astype(np.int64), count=count.cpu().numpy().astype(np.int64), rank=rank.cpu().numpy().astype(np.int64),
               wsum=wsum.cpu().numpy().view(np.uint64), head=head.cpu().numpy(),
               params=[p.detach().cpu().numpy() for p in model.parameters()], m=opt.exp_avg.cpu().numpy(), v=opt.exp_avg_sq.cpu().numpy(),
               m0=m0.cpu().numpy(), v0=v0.cpu().numpy())
    return rows, got


def _integers_match(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("src", "count", "rank", "wsum"))


def _ulp_errors(got, want):
    """-> (worst error of the new raw opacities / scales in float32 ulp over the written rows, are the other rows untouched?)"""
    w = want["written"]
    P = w.shape[0]
    worst, untouched = 0.0, True
    for t, key in ((5, "opacity64"), (3, "scaling64")):
        g = got["params"][t].reshape(P, -1).astype(np.float64)
        r64 = want[key].reshape(P, -1)
        if w.any():
            r32 = r64[w].astype(np.float32).astype(np.float64)
            worst = max(worst, float(np.max(np.abs(g[w] - r32) / ref.ulp32(r64[w]))))
        untouched = untouched and _bits_equal(got["params"][t].reshape(P, -1)[~w], want["params"][t].reshape(P, -1)[~w])
    return worst, untouched


@pytest.mark.parametrize("name", list(CASES))
def test_relocate_matches_the_yardstick(name):
    rows, got = _relocate_on_device(name)
    _, want = _yardstick(name)
    P = want["dead"].shape[0]
    # integer outputs, bit for bit
    for k in ("src", "count", "rank", "wsum"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert int(got["head"][0]) == want["total"] and int(got["head"][1]) == int(want["dead"].sum())
    assert int(got["head"][2]) == (1 if want["total"] == 0 else 0)
    if (want["src"] >= 0).any():
        assert not want["dead"][want["src"][want["src"] >= 0]].any()            # never a zero-weight row
    # rows that are copied equal their sources bit for bit, untouched rows are untouched
    for t in (0, 1, 2, 4):
        assert _bits_equal(got["params"][t], want["params"][t]), (name, t)
        moved = want["src"] >= 0
        if moved.any():
            assert _bits_equal(got["params"][t][moved], rows[t][want["src"][moved]])
    if name in ("no_dead", "all_dead"):
        for t in range(6):
            assert _bits_equal(got["params"][t], rows[t]), (name, t)
        assert _bits_equal(got["m"], got["m0"]) and _bits_equal(got["v"], got["v0"])
    # new raw opacities and scales: 1 float32 ulp of the float64 value rounded once (source opacities <= 0.99)
    worst, untouched = _ulp_errors(got, want)
    print(f"{name}: P {P}, dead {int(want['dead'].sum())}, written {int(want['written'].sum())}, worst deviation {worst:.3f} ulp")
    assert untouched and worst <= 1.0, (name, worst)
    if name == "one_alive_200_dead":
        assert want["count"][77] == 200                                             # N clamps at 51
        o_new = 1 / (1 + math.exp(-float(got["params"][5][77, 0])))
        o_old = 1 / (1 + math.exp(-float(rows[5][77, 0])))
        assert abs(1 - (1 - o_new) ** 51 - o_old) < 1e-5
    # the moments of written rows are zero, all others unchanged
    widths = [3, 3, 9, 3, 4, 1]
    off = 0
    for wd in widths:
        for key, key0 in (("m", "m0"), ("v", "v0")):
            a, a0 = got[key][off:off + P * wd].reshape(P, wd), got[key0][off:off + P * wd].reshape(P, wd)
            assert (a[want["written"]] == 0).all() and _bits_equal(a[~want["written"]], a0[~want["written"]]), (name, wd, key)
        off += P * wd


def test_both_mutants_are_rejected():
    """`ge` (first row with W >= t) lands on zero-weight rows where a draw is 0; `count` (N = count) changes every corrected value."""
    _, got = _relocate_on_device("runs_draw_ends")
    assert _integers_match(got, _yardstick("runs_draw_ends")[1])
    assert not _integers_match(got, _yardstick("runs_draw_ends", "ge")[1])
    _, got = _relocate_on_device("P1025")
    good, bad = _yardstick("P1025")[1], _yardstick("P1025", "count")[1]
    assert _integers_match(got, good) and _integers_match(got, bad)
    assert _ulp_errors(got, good)[0] <= 1.0 and _ulp_errors(got, bad)[0] > 1.0
    # both ends of the binary search
    want = _yardstick("runs_draw_ends")[1]
    alive = np.flatnonzero(~want["dead"])
    _, got = _relocate_on_device("runs_draw_ends")
    assert set(got["src"][want["dead"]].tolist()) == {int(alive[0]), int(alive[-1])}


def test_correction_at_opacity_one_minus_1e_6():
    """The alternating sum cancels about half of float64's digits here: relative 1e-5 instead of 1 ulp."""
    from binocular3dgs_amd import mcmc
    P = 64
    dead = np.ones(P, dtype=bool)
    dead[[5, 40]] = False
    rows = ref.make_rows(P, dead, seed=9)
    rows[5][[5, 40], 0] = np.float32(math.log((1 - 1e-6) / 1e-6))
    want = ref.relocate_ref(rows, seed=SEED, offset=3)
    model = _model(rows)
    src, count, _, _, _ = mcmc.relocate(model, None, iteration=3, seed=SEED, debug=True)
    assert np.array_equal(src.cpu().numpy(), want["src"]) and want["count"][[5, 40]].sum() == P - 2
    w = want["written"]
    worst = 0.0
    for t, key in ((5, "opacity64"), (3, "scaling64")):
        g = model.parameters()[t].detach().cpu().numpy().reshape(P, -1).astype(np.float64)[w]
        r = want[key].reshape(P, -1)[w]
        worst = max(worst, float(np.max(np.abs(g - r) / np.abs(r))))
    print(f"opacity 1 - 1e-6: counts {want['count'][[5, 40]].tolist()}, worst relative deviation {worst:.3e}")
    assert worst <= 1e-5


# ---- random numbers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257])
def test_raw_words_bit_for_bit(n):
    from binocular3dgs_amd import mcmc
    for stream_id, offset in ((0, 0), (2, 7)):
        got = _u32(mcmc.random_words(n, SEED, stream_id, offset))
        assert np.array_equal(got, ref.random_u32(n, SEED, stream_id, offset)), (n, stream_id, offset)
    assert mcmc.random_words(0, SEED, 0, 0).numel() == 0


def test_normals_against_float64_box_muller_and_standard():
    from binocular3dgs_amd import mcmc
    n = 1 << 20
    got = mcmc.random_normals(n, SEED, 0, 12).cpu().numpy().astype(np.float64)
    want = ref.random_normal64(n, SEED, 0, 12)
    err = np.abs(got - want) / ref.ulp32(want)
    print(f"normals: worst deviation {err.max():.3f} float32 ulp over {n} samples")
    assert np.isfinite(got).all() and err.max() <= 4.0
    se = 1 / math.sqrt(n)
    lag1 = float(np.mean(got[:-1] * got[1:]))
    print(f"mean {got.mean():+.2e}, variance - 1 {got.var() - 1:+.2e}, lag-1 {lag1:+.2e} (standard error {se:.1e})")
    assert abs(got.mean()) <= 5 * se and abs(got.var() - 1) <= 5 * math.sqrt(2) * se and abs(lag1) <= 5 * se
    short = mcmc.random_normals(5, SEED, 0, 12).cpu().numpy()
    assert _bits_equal(short, got[:5].astype(np.float32))


# ---- the position noise -------------------------------------------------------------------------------------------------------
def _noise_rows(P, seed=4):
    """low opacities (the gate g is open) and, every fifth row, opacity 0.5 (closed)"""
    rng = np.random.default_rng(seed)
    rows = ref.make_rows(P, np.zeros(P, dtype=bool), seed=seed)
    o = rng.uniform(0.001, 0.02, P)
    o[::5] = 0.5
    rows[5] = np.log(o / (1 - o)).reshape(P, 1).astype(np.float32)
    return rows, o


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1025])
def test_noise(P):
    from binocular3dgs_amd import mcmc
    rows, o = _noise_rows(P)
    lr, noise_lr, it = 1.6e-4, 5e5, 37
    zero = [np.zeros_like(rows[0])] + rows[1:]
    # positions zero: the output IS the step
    a = _model(zero)
    mcmc.inject_noise(a, lr, iteration=it, seed=SEED, noise_lr=noise_lr)
    step = a._xyz.detach().cpu().numpy()
    normals = mcmc.random_normals(3 * P, SEED, 0, it).view(P, 3)
    b = _model(zero)
    mcmc.inject_noise(b, lr, iteration=it, seed=SEED, noise_lr=noise_lr, normals=normals)
    assert _bits_equal(step, b._xyz.detach().cpu().numpy())                         # drawn in registers == handed in
    c = _model(zero)
    mcmc.inject_noise(c, torch.tensor([lr], dtype=torch.float32, device="cuda"), iteration=it, seed=SEED, noise_lr=noise_lr)
    assert _bits_equal(step, c._xyz.detach().cpu().numpy())                         # the learning rate from device memory
    d = _model(zero)
    mcmc.inject_noise(d, lr, iteration=it + 1, seed=SEED, noise_lr=noise_lr)
    assert not _bits_equal(step, d._xyz.detach().cpu().numpy())                     # another iteration, other draws
    # against float64: every component within 64 * 2^-24 * (max s)^2 * |n| * g * noise_lr * lr
    n64 = normals.cpu().numpy().astype(np.float64)
    want, g, smax = ref.noise_ref(rows[3], rows[4], rows[5], n64, noise_lr, lr)
    unit = 2.0 ** -24 * smax ** 2 * np.linalg.norm(n64, axis=1) * g * noise_lr * lr
    err = np.abs(step.astype(np.float64) - want)
    open_ = unit > 0
    ratio = float(np.max(err[open_] / unit[open_, None])) if open_.any() else 0.0
    print(f"noise P {P}: worst deviation {ratio:.2f} units of 2^-24 (max s)^2 |n| g noise_lr lr (bound 64)")
    assert (err <= 64 * unit[:, None]).all()
    assert not (o < 0.02).any() or np.abs(step[o < 0.02]).max() > 0
    # nonzero positions: one rounded addition of the same step; a row with opacity 0.5 does not move (g < 1e-21)
    e = _model(rows)
    mcmc.inject_noise(e, lr, iteration=it, seed=SEED, noise_lr=noise_lr)
    moved = e._xyz.detach().cpu().numpy()
    assert _bits_equal(moved, rows[0] + step)
    assert g[::5].max() < 1e-21 and _bits_equal(moved[::5], rows[0][::5])
    for t in range(1, 6):
        assert _bits_equal(e.parameters()[t].detach().cpu().numpy(), rows[t])


# ---- growth --------------------------------------------------------------------------------------------------------------------
def _training_args(iterations=300):
    import ref_schedule as rs
    LR = rs.LR
    return types.SimpleNamespace(percent_dense=0.01, position_lr_init=LR["position_lr_init"], position_lr_final=LR["position_lr_final"],
                                 position_lr_delay_mult=LR["position_lr_delay_mult"], position_lr_max_steps=iterations,
                                 feature_lr=LR["feature_lr"], opacity_lr=LR["opacity_lr"], scaling_lr=LR["scaling_lr"],
                                 rotation_lr=LR["rotation_lr"])


def _set_grads(model):
    for p in model.parameters():
        p.grad = torch.full_like(p, 1e-3)


@pytest.mark.parametrize("kind", ["adam", "fused"])
def test_grow(kind):
    from binocular3dgs_amd import mcmc
    P = 1000
    rows = ref.make_rows(P, ref.random_dead(P, 0.05, 1), seed=6)
    model = _model(rows)
    if kind == "adam":
        model.spatial_lr_scale = 1.0
        model.training_setup(_training_args())
        opt = model.optimizer
        for g in opt.param_groups:
            g["lr"] = 1e-4
        _set_grads(model)
        opt.step()                                             # (the state exists from the first step on)
        before = [p.detach().cpu().numpy().copy() for p in model.parameters()]
    else:
        opt = _fused_adam(model)
        before = [a.copy() for a in rows]
    sizes = []
    for it in (100, 200, 300):
        sizes.append(mcmc.grow(model, opt, 1080, iteration=it, seed=SEED))
    assert sizes == [1050, 1080, 1080]                          # min(cap_max, int(1.05 P)), and it stops at the cap
    now = [p.detach().cpu().numpy() for p in model.parameters()]
    assert all(a.shape[0] == 1080 and np.isfinite(a).all() for a in now)
    for t in (0, 1, 2, 4):                                      # old rows keep their bits ...
        alive = ~ref.classify(before[5], P, 0.005)[0]
        assert _bits_equal(now[t][:P][alive], before[t][alive])
    changed = (now[5][:P] != before[5]).reshape(-1)             # ... except sampled sources (lower opacity) and dead old rows
    alive = ~ref.classify(before[5], P, 0.005)[0]
    assert changed.any() and (now[5][:P][changed & alive] < before[5][changed & alive]).all()
    old_xyz = {tuple(r) for r in before[0].view(np.uint32).tolist()}
    assert all(tuple(r) in old_xyz for r in now[0][P:].view(np.uint32).tolist())   # every appended row copies an old one
    assert model.xyz_gradient_accum.shape[0] == 1080 and model.max_radii2D.shape[0] == 1080
    if kind == "adam":
        for g in opt.param_groups:
            st = opt.state[g["params"][0]]
            assert st["exp_avg"].shape == g["params"][0].shape and st["exp_avg_sq"].shape == g["params"][0].shape
            assert (st["exp_avg"][P:] == 0).all()
    else:
        assert opt.exp_avg.numel() == 1080 * 23 and all(p.shape[0] == 1080 for p in opt.params)
    _set_grads(model)
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert any(not np.array_equal(p.detach().cpu().numpy(), a) for p, a in zip(model.parameters(), now))


# ---- training ------------------------------------------------------------------------------------------------------------------
def _train(scene, strategy, iterations=300):
    import ref_schedule as rs
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.mcmc import McmcSchedule
    from binocular3dgs_amd.render import PipelineParams, render
    from binocular3dgs_amd.scene import Scene
    from binocular3dgs_amd.schedule import IterationSchedule
    i0 = scene["init"]
    W, H, bg = scene["W"], scene["H"], scene["bg"].cuda()
    m = GaussianModel.from_tensors(i0["xyz"], i0["features_dc"], i0["features_rest"], i0["scaling"], i0["rotation"], i0["opacity"],
                                   sh_degree=1, active_sh_degree=0, device="cuda")
    cams = synth.synth_cameras(W, H, yaws=synth.YAWS_6, device="cuda")[:3]
    for cam, gt in zip(cams, scene["gts"]):
        cam.original_image, cam.gt_alpha_mask = gt.cuda(), None
    # held-out views between the input ones, of the scene's own ground-truth Gaussians (ref_schedule.make_scene's model)
    truth = synth.synth_model(4000, seed=31, device="cuda", width=W, height=H, requires_grad=False)
    with torch.no_grad():
        truth._scaling += 0.9
        test_cams = synth.synth_cameras(W, H, yaws=(4.0, -4.0), device="cuda")
        for cam in test_cams:
            cam.original_image, cam.gt_alpha_mask = render(cam, truth, PipelineParams(), bg)["render"].clamp(0, 1).detach(), None
    m.spatial_lr_scale = scene["extent"]
    m.training_setup(_training_args(iterations))
    P0 = m.get_xyz.shape[0]
    cap = int(1.2 * P0)
    kw = dict(iterations=iterations, shift_cam_start=100, binocular=True, opacity_decay_factor=0.995, densify_from_iter=99,
              densify_until_iter=iterations, densification_interval=50, sh_interval=100, test_cameras=test_cams,
              test_iterations=(1, iterations))
    sc = Scene(cams, m, cameras_extent=scene["extent"])
    if strategy == "mcmc":
        sched = McmcSchedule(m, sc, PipelineParams(), bg, cap_max=cap, seed=11, log_relocations=True, **kw)
    else:
        sched = IterationSchedule(m, sc, PipelineParams(), bg, densify_grad_threshold=0.001, **kw)
    rng = np.random.default_rng(5)
    shifts = (rng.random(iterations + 1) * 0.4) * rng.choice([-1.0, 1.0], iterations + 1)
    counts = []
    for it in range(1, iterations + 1):
        sched.run_iteration(it, (it - 1) % 3, float(shifts[it]))
        counts.append(m.get_xyz.shape[0])
    torch.cuda.synchronize()
    log = {it: [t.cpu().numpy() for t in out] for it, out in getattr(sched, "relocation_log", {}).items()}
    return dict(model=m, counts=counts, cap=cap, P0=P0, reports=sched.reports, relocations=log,
                params=[p.detach().cpu().numpy().copy() for p in m.parameters()])


def _same(a, b):
    return all(x.shape == y.shape and _bits_equal(x, y) for x, y in zip(a["params"], b["params"]))


_RUNS = {}


def _run(strategy, k):
    """the k-th run of a strategy from the same seed, trained once per session"""
    import ref_schedule as rs
    if "scene" not in _RUNS:
        _RUNS["scene"] = rs.make_scene()
    if (strategy, k) not in _RUNS:
        _RUNS[(strategy, k)] = _train(_RUNS["scene"], strategy)
    return _RUNS[(strategy, k)]


def test_training_with_a_fixed_budget():
    """300 iterations on the synthetic scene of the graph-trainer tests, relocation and growth at 100, 150, 200, 250, the cap at
    1.2 x the initial points (1.05^4 > 1.2: reached).  The PSNR of the adc run is printed beside, not compared: two strategies
    at 300 iterations."""
    a, adc = _run("mcmc", 0), _run("adc", 0)
    assert max(a["counts"]) <= a["cap"] and a["counts"][-1] == a["cap"] and a["counts"][0] == a["P0"]
    assert a["counts"] == sorted(a["counts"]) and sorted(a["relocations"]) == [100, 150, 200, 250]
    assert all(np.isfinite(p).all() for p in a["params"])
    first, last = a["reports"][1]["test"][1], a["reports"][300]["test"][1]
    print(f"test-view PSNR: mcmc {float(first):.2f} -> {float(last):.2f} dB with {a['counts'][-1]} Gaussians; "
          f"adc {float(adc['reports'][1]['test'][1]):.2f} -> {float(adc['reports'][300]['test'][1]):.2f} dB with {adc['counts'][-1]}")
    assert float(last) > float(first)
    # the relocations never sampled a zero-weight row, and every dead row found a source
    for it, (src, count, rank, wsum, head) in a["relocations"].items():
        assert int(head[2]) == 0 and int((src >= 0).sum()) == int(head[1]) == int(count.sum()), it


def test_a_second_run_from_the_same_seed():
    """A second run with the same seed gives the same parameters bit for bit -- unless the existing adc schedule is not
    bit-reproducible on the same scene either (two adc runs are compared first).  It is not, on the MI355X: the blend backward
    accumulates with float atomics whose order of arrival differs from run to run, two adc runs differ, and so do two mcmc runs
    (largest parameter difference after 300 iterations: 9.0, a relocated Gaussian that went elsewhere).  What is asserted then is
    that the integer DECISIONS of the first relocation (iteration 100) agree: which rows are dead, their ranks, the source of
    every dead row and the count of every source.  The weight scan is not a decision but floor(opacity 2^24) summed, and it does
    differ: measured, 1991 of 2000 rows, totals 15181377248 against 15181377390 (1e-8 relative) -- the last bits of the
    opacities.  At iteration 100 no Gaussian of this scene is dead in either run, so the agreement is that of the dead flags and
    of an empty source list; on ONE state every integer output is one result, which test_relocate_matches_the_yardstick pins bit
    for bit.  The count of Gaussians per iteration, which only the rule of growth decides, is the same in both runs."""
    a, b = _run("mcmc", 0), _run("mcmc", 1)
    adc_same = _same(_run("adc", 0), _run("adc", 1))
    ra, rb = a["relocations"][100], b["relocations"][100]
    decisions_same = all(np.array_equal(ra[k], rb[k]) for k in (0, 1, 2)) and int(ra[4][1]) == int(rb[4][1])
    print(f"same seed twice: adc parameters {'bit for bit' if adc_same else 'differ'}, mcmc parameters "
          f"{'bit for bit' if _same(a, b) else 'differ'}; first relocation: dead rows {int(ra[4][1])} / {int(rb[4][1])}, "
          f"sources that differ {int((ra[0] != rb[0]).sum())}, counts that differ {int((ra[1] != rb[1]).sum())}, "
          f"rows whose weight scan differs {int((ra[3] != rb[3]).sum())} of {ra[3].shape[0]}, totals {int(ra[4][0])} / {int(rb[4][0])}; "
          f"largest parameter difference after 300 iterations "
          f"{max(float(np.max(np.abs(x - y))) for x, y in zip(a['params'], b['params'])):.3e}")
    assert a["counts"] == b["counts"]
    if adc_same:
        assert _same(a, b)
    else:
        assert decisions_same
