"""Test infrastructure: plain numpy restatement of ONE b3gs_adam_step (csrc/optim.hip) -- torch.optim.Adam(eps=1e-15) over
up to eight segments with their own learning rate, the optional opacity decay in both orders, the row mask, a step number
given by the caller -- in float64 (`adam_step`, the yardstick) and in float32 with one rounding per operation in the
kernel's order (`adam_step_f32`, which measures the float32 noise of the formula; the library is built with
-ffp-contract=off, so the kernel rounds where the source says).  tests/test_optim_ref_cpu.py pins the float64 form to
torch.optim.Adam on float64 tensors and derives the GPU bounds from the float32 form; tests/test_gpu_adam_edges.py compares
the kernel with the float64 form.  The input builders of both live here (`CASES`).  Never imported by the product."""
import numpy as np

BETAS = (0.9, 0.999)
EPS = 1e-15
F32 = np.float32


def per_element(counts, values):
    """One value per segment -> one per element of the flat (segment-major) arrays."""
    return np.repeat(np.asarray(values), np.asarray(counts, dtype=np.int64))


def logit_decay(p, factor):
    """o <- logit(sigmoid(o) * factor), the reference's opacity_decay (float64)."""
    p = np.asarray(p, np.float64)
    op = factor / (1.0 + np.exp(-p))
    return np.log(op / (1.0 - op))


def adam_step(p, g, m, v, lr, t, betas=BETAS, eps=EPS, decay=0.0, decay_sel=None, decay_first=False, live=None):
    """float64.  p, g, m, v: flat arrays (float32 values are cast, nothing is rounded in between); lr: scalar or one per
    element; t: the 1-based step number; decay_sel: boolean per element, the opacity segment (used when decay > 0);
    live: boolean per element, False = the row mask's bit is clear, the gradient counts as 0 without being looked at.
    Returns (p', m', v', delta)."""
    p, m, v = (np.asarray(x, np.float64) for x in (p, m, v))
    g = np.asarray(g, np.float64)
    if live is not None:
        g = np.where(live, g, 0.0)
    lr = np.asarray(lr, np.float64)
    b1, b2 = float(betas[0]), float(betas[1])
    m2 = b1 * m + (1.0 - b1) * g
    v2 = b2 * v + (1.0 - b2) * g * g
    delta = (lr / (1.0 - b1 ** t)) * m2 / (np.sqrt(v2) / np.sqrt(1.0 - b2 ** t) + eps)
    if decay > 0 and decay_sel is not None:
        sel = np.asarray(decay_sel, bool)
        if decay_first:
            p2 = np.where(sel, logit_decay(p, decay) - delta, p - delta)
        else:
            p2 = np.where(sel, logit_decay(p - delta, decay), p - delta)
    else:
        p2 = p - delta
    return p2, m2, v2, delta


def logit_decay_f32(p, factor):
    p = np.asarray(p, F32)
    op = F32(factor) / (F32(1) + np.exp(-p))
    return np.log(op / (F32(1) - op))


def adam_step_f32(p, g, m, v, lr, t, betas=BETAS, eps=EPS, decay=0.0, decay_sel=None, decay_first=False, live=None):
    """The same statement with every operation rounded to float32, in the order of adam_one / adam_kernel."""
    p, m, v = (np.asarray(x, F32) for x in (p, m, v))
    g = np.asarray(g, F32)
    if live is not None:
        g = np.where(live, g, F32(0))
    lr = np.asarray(lr, np.float64).astype(F32)
    b1, b2, eps = F32(betas[0]), F32(betas[1]), F32(eps)
    tf = float(F32(t))
    bc1 = F32(1) - F32(float(b1) ** tf)                      # 1.0f - powf(beta1, t)
    bc2_sqrt = np.sqrt(F32(1) - F32(float(b2) ** tf))        # sqrtf(1.0f - powf(beta2, t))
    with np.errstate(under="ignore"):
        m2 = b1 * m + (F32(1) - b1) * g
        v2 = b2 * v + ((F32(1) - b2) * g) * g
        denom = np.sqrt(v2) / bc2_sqrt + eps
        delta = (lr / bc1) * (m2 / denom)
    assert m2.dtype == F32 and v2.dtype == F32 and delta.dtype == F32
    if decay > 0 and decay_sel is not None:
        sel = np.asarray(decay_sel, bool)
        if decay_first:
            p2 = np.where(sel, logit_decay_f32(p, decay) - delta, p - delta)
        else:
            p2 = np.where(sel, logit_decay_f32(p - delta, decay), p - delta)
    else:
        p2 = p - delta
    assert p2.dtype == F32
    return p2, m2, v2, delta


# ---- error measures -------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """|got - ref| / |ref| per element; where the reference is exactly 0 the result must be exactly 0 (error 0, else inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ref != 0, d / np.abs(ref), np.where(d == 0, 0.0, np.inf))
    return e


def p_err(got, ref, p_in, delta):
    """|got - ref| in units of the larger of one float32 ulp of the parameter (taken at the larger of its magnitude before
    and after the step: a decayed logit of 0 lands at -0.01) and one ulp of the update, 2^-23 |delta|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    mag = np.maximum(np.abs(np.asarray(p_in, np.float64)), np.abs(ref)).astype(F32)
    unit = np.maximum(np.spacing(mag).astype(np.float64), 2.0 ** -23 * np.abs(np.asarray(delta, np.float64)))
    return np.abs(got - ref) / unit


# The bounds of tests/test_gpu_adam_edges.py: 10 x the largest 99th percentile, over every case of CASES, of the float32
# restatement against the float64 one (measured, printed and checked against these figures by tests/test_optim_ref_cpu.py);
# at most TAIL of the elements of a case may lie above them.
GPU_BOUNDS = {"m": 3.37e-6, "v": 1.30e-4, "p": 1.57e3}
TAIL = 1e-3


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _log_uniform(rng, n, lo, hi):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def gradients(rng, n, zero_share=1.0 / 16):
    """|g| in {0} U [1e-12, 1e3] log-uniform (g^2 stays a normal float32), random sign."""
    g = _log_uniform(rng, n, 1e-12, 1e3) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < zero_share] = 0.0
    return g.astype(F32)


def conditioned(g, m, betas=BETAS):
    """Keeps the inputs where the relative error of m' = b1 m + (1 - b1) g is a property of the arithmetic and not of a
    cancellation: a gradient that opposes the running mean with (1 - b1)|g| within a factor 2 of b1|m| has its sign turned
    (the sum then loses at most a factor 3 against its larger term).  Gradients against m outside that band stay."""
    g, m = np.asarray(g, F32), np.asarray(m, F32)
    a, b = betas[0] * np.abs(m.astype(np.float64)), (1.0 - betas[0]) * np.abs(g.astype(np.float64))
    near = (np.sign(g) * np.sign(m) < 0) & (b >= 0.5 * a) & (b <= 2.0 * a)
    return np.where(near, -g, g).astype(F32)


def warm_state(rng, n, cold_share=1.0 / 16):
    """m, v after two warm-up steps of the reference on gradients of their own, plus elements with m = v = 0."""
    m, v = np.zeros(n), np.zeros(n)
    for t in (1, 2):
        _, m, v, _ = adam_step(np.zeros(n), gradients(rng, n), m, v, 1e-3, t)
    cold = rng.random(n) < cold_share
    m[cold], v[cold] = 0.0, 0.0
    return m.astype(F32), v.astype(F32)


def opacity_logits(rng, n):
    """Logits in [-10, 10]: an eighth each at +10, -10, 0, +1e-3, -1e-3, the rest uniform."""
    o = rng.uniform(-10.0, 10.0, n)
    k = n // 8
    for j, x in enumerate((10.0, -10.0, 0.0, 1e-3, -1e-3)):
        o[j * k:(j + 1) * k] = x
    return o.astype(F32)


def make_case(counts, lrs, seed, t=1, decay=0.0, opacity_seg=-1, decay_first=False, steps=1, row_len=None):
    """A flat (segment-major) input set: float32 p, g, m, v of sum(counts) elements."""
    rng = np.random.default_rng(seed)
    counts = [int(c) for c in counts]
    n = sum(counts)
    p = rng.standard_normal(n).astype(F32)
    m, v = warm_state(rng, n)
    g = conditioned(gradients(rng, n), m)
    extra = [gradients(rng, n) for _ in range(steps - 1)]      # steps 2..: conditioned on the state they meet
    start = np.concatenate([[0], np.cumsum(counts)])
    if opacity_seg >= 0:
        a, b = int(start[opacity_seg]), int(start[opacity_seg + 1])
        p[a:b] = opacity_logits(rng, b - a)
    seg = per_element(counts, np.arange(len(counts)))
    return dict(counts=counts, lrs=[float(x) for x in lrs], start=start, p=p, g=g, m=m, v=v, t=int(t), decay=float(decay),
                opacity_seg=int(opacity_seg), decay_first=bool(decay_first), steps=int(steps),
                lr=per_element(counts, [float(x) for x in lrs]), decay_sel=(seg == opacity_seg), live=None,
                row_len=row_len, extra=extra)


def reference(case, p=None, g=None, m=None, v=None, t=None, f32=False):
    """One step of `case` (state overridable: a chain of steps feeds the previous result back in)."""
    fn = adam_step_f32 if f32 else adam_step
    pick = lambda x, k: case[k] if x is None else x  # noqa: E731
    return fn(pick(p, "p"), pick(g, "g"), pick(m, "m"), pick(v, "v"), case["lr"], case["t"] if t is None else t,
              decay=case["decay"], decay_sel=case["decay_sel"], decay_first=case["decay_first"], live=case["live"])


SEAM_LRS = [10.0 ** (k - 6) for k in range(8)]           # a factor 10 apart: a seam taken one element wrong is a wrong lr
SEAM_COUNTS = (4, 0, 252, 1020, 0, 4096, 12, 260)         # float4 kernel; seams inside a wave and inside a 256-thread block
SEAM_COUNTS_ODD = (4, 0, 253, 1019, 0, 4096, 12, 260)     # one count odd: scalar kernel, the same flat data
SEAM_COUNTS_TAIL = (4, 0, 252, 1020, 0, 4096, 272, 0)     # nseg == 8 with a trailing empty segment
MODEL_LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 0.05]
ROW_LENS = (3, 3, 45, 3, 4, 1)                            # the six tensors at 16 SH coefficients
WG = 256 * 4                                              # floats per workgroup of the float4 kernel
# workgroups -> total floats (ragged ones a few float4s short of the full grid)
GRID_TOTALS = {1: 1 * WG - 12, 63: 63 * WG, 64: 64 * WG - 4, 65: 65 * WG - 8, 128: 128 * WG, 129: 129 * WG - 1020}
BIG_COUNTS = (1050000,) * 8                               # > 8192 * 256 * 4 floats: the grid-stride loop runs twice
DEPTH_STEPS = (1, 2, 10, 1000, 30000)
MASK_FIRSTS = {1: 150, 63: 130, 64: 64, 100: 200}         # first -> count of the masked step_rows calls (P = 300)
MASK_P = 300


def edge_rows():
    """One tensor with a row for every (state, gradient) edge: state cold (m = v = 0), warm with m > 0, warm with m < 0;
    g in {0, +-1e-12, +-1e-6, +-1, +-1e3} (both signs against m); 64 elements of each with their own warm magnitudes."""
    rng = np.random.default_rng(77)
    gs = [0.0] + [s * x for x in (1e-12, 1e-6, 1.0, 1e3) for s in (1.0, -1.0)]
    rep = 64
    p, g, m, v, kind = [], [], [], [], []
    for state in (0, 1, -1):
        for gv in gs:
            mm, vv = warm_state(rng, rep, cold_share=0.0)
            if state == 0:
                mm[:], vv[:] = 0.0, 0.0
            else:
                mm = (np.abs(mm) * state).astype(F32)
            p.append(rng.standard_normal(rep).astype(F32)), g.append(np.full(rep, gv, F32)), m.append(mm), v.append(vv)
            kind.append(np.full(rep, state))
    p, g, m, v, kind = (np.concatenate(x) for x in (p, g, m, v, kind))
    g = conditioned(g, m)
    n = p.size
    return dict(counts=[n], lrs=[1e-3], start=np.array([0, n]), p=p, g=g, m=m, v=v, t=3, decay=0.0, opacity_seg=-1,
                decay_first=False, steps=1, lr=np.full(n, 1e-3), decay_sel=np.zeros(n, bool), live=None, row_len=None,
                kind=kind)


def mask_case(first):
    """Rows [first, first + count) of P = 300 Gaussians with row lengths ROW_LENS, about 60 % of the rows live; the flat
    arrays hold ALL rows (tensor-major), `rows` says which elements the call updates and `live` which of them are live."""
    count = MASK_FIRSTS[first]
    c = make_case([MASK_P * w for w in ROW_LENS], MODEL_LRS, 400 + first, t=4, decay=0.995, opacity_seg=5, decay_first=True)
    rng = np.random.default_rng(900 + first)
    live_rows = rng.random(MASK_P) < 0.6
    live_rows[first], live_rows[first + count - 1] = True, False
    row = np.concatenate([np.repeat(np.arange(MASK_P), w) for w in ROW_LENS])
    c.update(first=first, count=count, live_rows=live_rows, live=live_rows[row], rows=(row >= first) & (row < first + count))
    return c


def _decay_only():
    """b3gs_opacity_decay alone: the Adam statement with nothing to add (g = m = v = 0, delta = 0), an odd length."""
    c = make_case([1003], [0.05], 370, decay=0.995, opacity_seg=0)
    for k in ("g", "m", "v"):
        c[k] = np.zeros_like(c[k])
    return c


def _grid_case(wgs):
    n = GRID_TOTALS[wgs]
    a = (n // 3) // 4 * 4
    return make_case([a, n - a], [1e-3, 2e-2], 100 + wgs, steps=3)


def _decay_case(order, where):
    seg = 5 if where == "last" else 2
    counts = [MASK_P * w for w in ROW_LENS] if where == "last" else [400, 0, 300, 45 * 12, 260, 4]
    return make_case(counts, MODEL_LRS, 300 + seg + 10 * order, t=7, decay=0.995, opacity_seg=seg, decay_first=bool(order))


CASES = {"seams_vec4": lambda: make_case(SEAM_COUNTS, SEAM_LRS, 1),
         "seams_odd": lambda: make_case(SEAM_COUNTS_ODD, SEAM_LRS, 1),
         "seams_tail": lambda: make_case(SEAM_COUNTS_TAIL, SEAM_LRS, 1),
         "edge_rows": edge_rows,
         "no_decay": lambda: make_case([MASK_P * w for w in ROW_LENS], MODEL_LRS, 350, t=7, decay=0.0, opacity_seg=5),
         "lr_dev": lambda: make_case([MASK_P * w for w in ROW_LENS], [3.0 * x for x in MODEL_LRS], 360, t=2),
         "decay_only": _decay_only,
         "big": lambda: make_case(BIG_COUNTS, SEAM_LRS, 2)}
for _w in GRID_TOTALS:
    CASES[f"grid_{_w}"] = (lambda w=_w: _grid_case(w))
for _t in DEPTH_STEPS:
    CASES[f"depth_{_t}"] = (lambda t=_t: make_case([MASK_P * w for w in ROW_LENS], MODEL_LRS, 200, t=t))
for _o in (0, 1):
    for _w in ("last", "middle"):
        CASES[f"decay_{'first' if _o else 'after'}_{_w}"] = (lambda o=_o, w=_w: _decay_case(o, w))
for _f in MASK_FIRSTS:
    CASES[f"mask_{_f}"] = (lambda f=_f: mask_case(f))


def step_gradient(case, s, m):
    """The gradient of step `s` (0-based) of a chain, given the running mean that step starts from."""
    return case["g"] if s == 0 else conditioned(case["extra"][s - 1], m)


def measure(case):
    """float32 restatement against the float64 one on `case`, `steps` steps in a chain (each step's float64 result is
    computed from the float32 state the step started from).  -> dict of per-element error arrays for m, v, p."""
    out = {"m": [], "v": [], "p": []}
    p, m, v = case["p"], case["m"], case["v"]
    sel = case.get("rows")
    for s in range(case["steps"]):
        t = case["t"] + s
        g = step_gradient(case, s, m)
        rp, rm, rv, rd = reference(case, p=p, g=g, m=m, v=v, t=t)
        fp, fm, fv, _ = reference(case, p=p, g=g, m=m, v=v, t=t, f32=True)
        e = {"m": rel_err(fm, rm), "v": rel_err(fv, rv), "p": p_err(fp, rp, p, rd)}
        for k in out:
            out[k].append(e[k] if sel is None else e[k][sel])
        p, m, v = fp, fm, fv
    return {k: np.concatenate(x) for k, x in out.items()}
