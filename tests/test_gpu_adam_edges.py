"""GPU: b3gs_adam_step / b3gs_adam_step_at / b3gs_opacity_decay (csrc/optim.hip, csrc/lossfn.hip) against the float64
restatement of tests/optim_ref.py on p, exp_avg and exp_avg_sq, at the edges no other test reaches: segment seams inside a
float4 group's neighbourhood, a wave and a 256-thread block (empty segments, nseg == 8, the scalar kernel through an odd
count AND through a misaligned pointer), the two-level completion counter at 1 / 63 / 64 / 65 / 128 / 129 workgroups and
behind the grid-stride loop, the bias correction at t = 1 .. 30 000, zero / tiny / huge gradients on cold and warm state,
the opacity decay in both orders on a last and a middle segment, the row mask with first_row > 0, lr_dev and the skip word.

Criterion (optim_ref.GPU_BOUNDS; tests/test_optim_ref_cpu.py measures, prints and checks these figures -- they are the float32
noise of the formula, not the kernel's output): per element, relative error of exp_avg <= 3.37e-6 and of exp_avg_sq
<= 1.30e-4; |p - ref| <= 1.57e3 units, one unit being the larger of one float32 ulp of the parameter and one ulp of the
update (2^-23 |delta|).  Each is 10 x the largest 99th percentile over all cases of the float32 restatement (one rounding per
operation, the kernel's order) against float64: 3.369e-7 (m), 1.295e-5 (v), 156.4 units (p).  At most 0.1 % of a case's
elements may lie above a bound.  Where the figures come from: 1 - 0.999f is 1.29e-5 (relative) away from 0.001, which is
all of the exp_avg_sq figure and 54 of the units of p; the largest p figure belongs to decayed logits of 0 and +-1e-3, whose
result (-0.01) carries the absolute rounding of a sigmoid near 0.5.  Per case (99th percentile m / v / p): seams 3.35e-7 /
1.29e-5 / 56.7; grid sizes 3.3e-7 / 1.29e-5 / 32-33; depth 3.32e-7 / 1.29e-5 / 2.5-10.9; decay 3.1-3.4e-7 / 1.29e-5 /
5.3-156.4; row mask 3.1e-7 / 1.29e-5 / 8.9-46.3; edge rows 3.11e-7 / 1.29e-5 / 3.6.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64            # floats between two segments of a backing buffer
SENTINEL = 12345.0


class Dev:
    """The segments of a case on the device: one backing buffer per quantity, every segment 256-byte aligned (one float
    further for `misalign`) with GUARD untouched floats on either side -- a seam taken one element wrong lands in a guard."""

    def __init__(self, case, misalign=None):
        self.counts = case["counts"]
        self.off, o = [], GUARD
        for k, c in enumerate(self.counts):
            a = o + (1 if k == misalign else 0)
            self.off.append(a)
            o = -(-(a + c + GUARD) // 64) * 64
        self.size = o
        self.buf = {n: torch.full((o,), SENTINEL, dtype=torch.float32, device="cuda") for n in "pgmv"}
        self.inside = np.zeros(o, bool)
        for a, c in zip(self.off, self.counts):
            self.inside[a:a + c] = True
        for n in "pgmv":
            self.put(n, case[n])

    def put(self, name, flat):
        host = np.full(self.size, SENTINEL, np.float32)
        host[self.inside] = np.asarray(flat, np.float32)
        self.buf[name].copy_(torch.from_numpy(host))

    def get(self, name):
        host = self.buf[name].cpu().numpy()
        assert (host[~self.inside] == SENTINEL).all(), f"{name}: a guard float between two segments was written"
        return host[self.inside]

    def segs(self, lrs):
        ptr = lambda n, k: self.buf[n].data_ptr() + 4 * self.off[k] if self.counts[k] else 0  # noqa: E731
        return [(ptr("p", k), ptr("g", k), ptr("m", k), ptr("v", k), c, lr) for k, (c, lr) in enumerate(zip(self.counts, lrs))]


def _words(step=0):
    from binocular3dgs_amd.step import _step_words
    w = _step_words("cuda")
    w[0] = step
    return w


def _launch(dev, case, words, bump=1, skip=None):
    from binocular3dgs_amd.step import _adam_launch
    _adam_launch(dev.segs(case["lrs"]), words, R.BETAS, R.EPS, case["decay"], case["opacity_seg"], case["decay_first"], bump,
                 torch.device("cuda"), None, skip)
    torch.cuda.synchronize()


def _assert_words(words, step):
    w = words.cpu().numpy()
    assert int(w[0]) == step, (int(w[0]), step)
    assert not w[1:].any(), f"completion words left non-zero at {np.nonzero(w[1:])[0][:8] + 1}"


def _check(label, got, ref, p_in, sel=None):
    """got = (p, m, v) of the kernel, ref = (p, m, v, delta) of optim_ref.adam_step.  Figures first, then the assertions."""
    e = {"p": R.p_err(got[0], ref[0], p_in, ref[3]), "m": R.rel_err(got[1], ref[1]), "v": R.rel_err(got[2], ref[2])}
    if sel is not None:
        e = {k: x[sel] for k, x in e.items()}
    for k in ("m", "v", "p"):
        print(f"{label} {k}: p50 {np.percentile(e[k], 50):.2e} p99 {np.percentile(e[k], 99):.2e} max {e[k].max():.2e} "
              f"above the bound {R.GPU_BOUNDS[k]:.2e}: {int((e[k] > R.GPU_BOUNDS[k]).sum())} of {e[k].size}")
    for x in got:
        assert not np.isnan(x).any(), label
    for k, x in e.items():
        assert float((x > R.GPU_BOUNDS[k]).mean()) <= R.TAIL, (label, k, float(x.max()), float((x > R.GPU_BOUNDS[k]).mean()))


def _run(case, misalign=None, step0=None):
    dev = Dev(case, misalign)
    words = _words(case["t"] - 1 if step0 is None else step0)
    _launch(dev, case, words)
    _assert_words(words, case["t"])
    return dev.get("p"), dev.get("m"), dev.get("v")


# ---- segment seams and the kernel choice --------------------------------------------------------------------------------------
def test_segment_seams_in_the_float4_and_both_scalar_kernels():
    """Eight segments, learning rates a factor 10 apart, counts 4, 0, 252, 1020, 0, 4096, 12, 260: seams inside a wave (4, 256)
    and inside a 256-thread block, empty segments second and in the middle.  float4 kernel; the same flat data with a count
    of 253 (scalar kernel by count) and with one tensor a view one float into its storage (scalar kernel by alignment); nseg
    == 8 with a trailing empty segment."""
    vec, odd, tail = R.CASES["seams_vec4"](), R.CASES["seams_odd"](), R.CASES["seams_tail"]()
    assert len(vec["counts"]) == len(tail["counts"]) == 8 and tail["counts"][-1] == 0
    for k in "pgmv":
        assert np.array_equal(vec[k], odd[k]) and np.array_equal(vec[k], tail[k])
    got_vec, got_odd, got_mis, got_tail = _run(vec), _run(odd), _run(vec, misalign=3), _run(tail)
    _check("float4", got_vec, R.reference(vec), vec["p"])
    _check("scalar (count 253)", got_odd, R.reference(odd), odd["p"])
    _check("scalar (misaligned)", got_mis, R.reference(vec), vec["p"])
    _check("trailing empty segment", got_tail, R.reference(tail), tail["p"])
    common = vec["lr"] == odd["lr"]
    assert int((~common).sum()) == 1
    for a, b in zip(got_odd, got_mis):
        assert np.array_equal(a[common], b[common])


# ---- step counter and completion words -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wgs", list(R.GRID_TOTALS))
def test_step_counter_and_completion_words_at_every_grid_branch(wgs):
    """gridDim < 64, == 64, > 64, a second workgroup per slot (128, 129): three steps with bump = 1 -- after each, word 0 is
    the step number and every other word 0 (what makes the launch replayable) -- then one with bump = 0: no word changes."""
    case = R.CASES[f"grid_{wgs}"]()
    assert all(c % 4 == 0 for c in case["counts"]) and (sum(case["counts"]) // 4 + 255) // 256 == wgs
    dev, words = Dev(case), _words(0)
    p, m, v = case["p"], case["m"], case["v"]
    for s in range(4):
        bump = s < 3
        g = R.step_gradient(case, min(s, 2), m)
        dev.put("g", g)
        _launch(dev, case, words, bump=int(bump))
        _assert_words(words, s + 1 if bump else 3)
        got = dev.get("p"), dev.get("m"), dev.get("v")
        _check(f"{wgs} workgroups step {s + 1} bump {int(bump)}", got, R.reference(case, p=p, g=g, m=m, v=v, t=s + 1), p)
        p, m, v = got


def test_grid_stride_loop_beyond_8192_workgroups():
    """8 x 1 050 000 floats: 2 100 000 float4s for 8192 x 256 threads, so every thread of the first 2848 takes a second item
    and the seams fall in either pass.  Three steps; the first is compared in full, all three advance the step once."""
    case = R.CASES["big"]()
    assert sum(case["counts"]) > 8192 * 256 * 4
    dev, words = Dev(case), _words(0)
    for s in range(3):
        _launch(dev, case, words)
        _assert_words(words, s + 1)
        if s == 0:
            _check("grid stride", (dev.get("p"), dev.get("m"), dev.get("v")), R.reference(case), case["p"])


def _model_tensors(case, P=R.MASK_P):
    ps, off = [], 0
    for w in R.ROW_LENS:
        ps.append(torch.nn.Parameter(torch.from_numpy(case["p"][off:off + P * w].reshape(P, w).copy()).cuda()))
        off += P * w
    return ps


def _fused(case, ps, lrs=None, **kw):
    from binocular3dgs_amd.step import FusedAdam
    opt = FusedAdam(ps, case["lrs"] if lrs is None else lrs, betas=R.BETAS, eps=R.EPS, **kw)
    opt.exp_avg.copy_(torch.from_numpy(case["m"]))
    opt.exp_avg_sq.copy_(torch.from_numpy(case["v"]))
    opt.step_count.fill_(case["t"] - 1)
    return opt


def _set_grads(ps, flat, P=R.MASK_P):
    off = 0
    for p, w in zip(ps, R.ROW_LENS):
        p.grad = torch.from_numpy(np.asarray(flat[off:off + P * w], np.float32).reshape(P, w).copy()).cuda()
        off += P * w


def _flat(ps):
    return np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in ps])


def test_three_row_ranges_equal_one_whole_step_bit_for_bit():
    case = R.CASES["depth_10"]()
    res = []
    for ranges in ([(0, R.MASK_P)], [(0, 100), (100, 37), (137, 163)]):
        ps = _model_tensors(case)
        opt = _fused(case, ps)
        _set_grads(ps, case["g"])
        for j, (first, count) in enumerate(ranges):
            ptrs = [p.grad.data_ptr() + 4 * w * first for p, w in zip(ps, R.ROW_LENS)]
            opt.step_rows(first, count, ptrs, last=(j == len(ranges) - 1))
        torch.cuda.synchronize()
        _assert_words(opt._step_words, case["t"])
        res.append((_flat(ps), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()))
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    _check("row ranges", res[1], R.reference(case), case["p"])


# ---- bias correction at depth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", list(R.DEPTH_STEPS))
def test_bias_correction_at_depth_and_the_host_counted_step(t):
    """The device step word preset to t - 1; b3gs_adam_step_at(step = t) on the same data is bit-identical."""
    from binocular3dgs_amd import _lib
    case = R.CASES[f"depth_{t}"]()
    got = _run(case)
    _check(f"t = {t}", got, R.reference(case), case["p"])
    dev = Dev(case)
    py = dev.segs(case["lrs"])
    segs = (_lib.B3gsAdamSegment * len(py))()
    for k, (p, g, m, v, n, lr) in enumerate(py):
        segs[k].param, segs[k].grad, segs[k].exp_avg, segs[k].exp_avg_sq = p or None, g or None, m or None, v or None
        segs[k].count, segs[k].lr, segs[k].row_len, segs[k].first_row, segs[k].lr_dev = n, lr, 0, 0, None
    rc = _lib.lib().b3gs_adam_step_at(len(py), segs, t, R.BETAS[0], R.BETAS[1], R.EPS, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "b3gs_adam_step_at")
    torch.cuda.synchronize()
    for a, n in zip(got, "pmv"):
        assert np.array_equal(a, dev.get(n)), n


# ---- gradient and state edges ------------------------------------------------------------------------------------------------
def test_zero_tiny_and_huge_gradients_on_cold_and_warm_state():
    case = R.CASES["edge_rows"]()
    got = _run(case)
    ref = R.reference(case)
    _check("edge rows", got, ref, case["p"])
    cold, g = case["kind"] == 0, case["g"]
    for mag in (0.0, 1e-12, 1e-6, 1.0, 1e3):
        for kind in (0, 1, -1):
            assert int(((np.abs(g) == np.float32(mag)) & (case["kind"] == kind)).sum()) >= 64
    assert int(((np.sign(g) * np.sign(case["m"])) < 0).sum()) >= 256       # gradients against the running mean
    still = cold & (g == 0)               # nothing to add to nothing: 0 / (0 + eps), the parameter must not move
    assert np.array_equal(got[0][still], case["p"][still]) and not got[1][still].any() and not got[2][still].any()
    # no element of any (state, gradient) class above the bounds: the classes are 64 elements each, the share rule allows none
    e = {"p": R.p_err(got[0], ref[0], case["p"], ref[3]), "m": R.rel_err(got[1], ref[1]), "v": R.rel_err(got[2], ref[2])}
    for k, x in e.items():
        assert float(x.max()) <= R.GPU_BOUNDS[k], (k, float(x.max()), float(g[x.argmax()]), int(case["kind"][x.argmax()]))


# ---- opacity decay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["decay_after_last", "decay_after_middle", "decay_first_last", "decay_first_middle", "no_decay"])
def test_opacity_decay_in_both_orders_on_a_last_and_a_middle_segment(name):
    """Logits at +-10, 0, +-1e-3 and in between.  The reference decays the opacity segment alone: a neighbour the kernel
    decayed as well is 5e-3 or more away.  no_decay: opacity_decay = 0 with a valid opacity_seg."""
    case = R.CASES[name]()
    seg = case["opacity_seg"]
    assert case["counts"][seg] > 0 and (name.endswith("middle")) == (seg < len(case["counts"]) - 1)
    got = _run(case)
    ref = R.reference(case)
    _check(name, got, ref, case["p"])
    # per segment: nothing above the bound outside the opacity segment's special logits is hidden by the share rule
    e = R.p_err(got[0], ref[0], case["p"], ref[3])
    for k in range(len(case["counts"])):
        a, b = case["start"][k], case["start"][k + 1]
        if b > a:
            assert float((e[a:b] > R.GPU_BOUNDS["p"]).mean()) <= R.TAIL, (name, k, float(e[a:b].max()))
    if name == "no_decay":
        plain = dict(case, opacity_seg=-1)
        assert all(np.array_equal(a, b) for a, b in zip(got, _run(plain)))


def test_opacity_decay_alone():
    from binocular3dgs_amd import _lib
    case = R.CASES["decay_only"]()
    o = torch.from_numpy(case["p"]).cuda()
    _lib.check(_lib.lib().b3gs_opacity_decay(o.data_ptr(), o.numel(), 0.995, torch.cuda.current_stream().cuda_stream),
               "b3gs_opacity_decay")
    torch.cuda.synchronize()
    ref = R.reference(case)
    assert not ref[3].any() and np.array_equal(ref[0], R.logit_decay(case["p"], 0.995))
    z = np.zeros_like(case["p"])
    _check("b3gs_opacity_decay", (o.cpu().numpy(), z, z), ref, case["p"])
    # and through the step: the same statement with nothing to add
    _check("decay through the step", _run(case), ref, case["p"])


# ---- row mask with first_row -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", list(R.MASK_FIRSTS))
def test_row_mask_of_a_row_range_starting_past_row_zero(first):
    """step_rows(first, count, row_mask=words) on P = 300, row lengths 3, 3, 45, 3, 4, 1 (first = 1 and 63: scalar kernel;
    64 and 100: float4 groups that straddle rows).  Dead rows hold NaN gradients; the bitmap is addressed by first_row + row."""
    case = R.CASES[f"mask_{first}"]()
    count, live_rows, rows = case["count"], case["live_rows"], case["rows"]
    assert live_rows[first] and not live_rows[first + count - 1] and 0.4 < live_rows[first:first + count].mean() < 0.8
    bits = np.zeros(320, np.uint64)
    bits[:R.MASK_P] = live_rows
    words = (bits.reshape(-1, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    words = torch.from_numpy(words.view(np.int64)).cuda()
    res = []
    for masked in (True, False):
        ps = _model_tensors(case)
        opt = _fused(case, ps, opacity_decay=case["decay"], opacity_index=case["opacity_seg"], decay_first=case["decay_first"])
        _set_grads(ps, np.where(case["live"], case["g"], np.float32("nan") if masked else np.float32(0)))
        ptrs = [p.grad.data_ptr() + 4 * w * first for p, w in zip(ps, R.ROW_LENS)]
        opt.step_rows(first, count, ptrs, last=True, row_mask=words if masked else None)
        torch.cuda.synchronize()
        _assert_words(opt._step_words, case["t"])
        res.append((_flat(ps), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()))
    for a, b, k in zip(res[0], res[1], "pmv"):
        assert not np.isnan(a).any() and np.array_equal(a, b), k
        assert np.array_equal(a[~rows], case[k][~rows]), f"{k}: a row outside [first, first + count) changed"
    _check(f"row mask first {first}", res[0], R.reference(case), case["p"], sel=rows)


# ---- lr_dev and the skip flag -----------------------------------------------------------------------------------------------
def test_device_learning_rates_and_the_skip_word():
    case = R.CASES["lr_dev"]()
    ps = _model_tensors(case)
    opt = _fused(case, ps, lrs=[1.0] * 6)            # ignored once lr_device is set
    opt.lr_device = torch.tensor(case["lrs"], dtype=torch.float32, device="cuda")
    _set_grads(ps, case["g"])
    opt.skip_flag = torch.ones(1, dtype=torch.int32, device="cuda")
    opt.step()
    torch.cuda.synchronize()
    _assert_words(opt._step_words, case["t"] - 1)
    for a, k in zip((_flat(ps), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()), "pmv"):
        assert np.array_equal(a, case[k]), f"{k} changed in a skipped step"
    opt.skip_flag.zero_()
    opt.step()
    torch.cuda.synchronize()
    _assert_words(opt._step_words, case["t"])
    _check("lr_dev", (_flat(ps), opt.exp_avg.cpu().numpy(), opt.exp_avg_sq.cpu().numpy()), R.reference(case), case["p"])
