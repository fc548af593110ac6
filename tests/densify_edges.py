"""Test infrastructure: input sets for the densify kernels (csrc/densify.hip) that hold every decision edge the code takes
care over, by construction, and no fragile decision: what is compared after an exp (the largest scale against
percent_dense * extent and 0.1 * extent, the sigmoid against min_opacity) sits 6 % or more from its threshold, what is exact
in float32 (accum / denom against the gradient threshold, a power of two) sits exactly on it.  Shared by
tests/test_densify_edges_cpu.py (tests/densify_ref.py in float32 and float64 takes the same decisions; the float32 noise of
the children) and tests/test_gpu_densify_edges.py.  Never imported by the product."""
import numpy as np
import torch

import densify_ref

NAMES = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity")
THR = 2.0 ** -12            # the gradient threshold: exact in float32
MIN_OPACITY = 0.005
EXTENT = 4.0
PERCENT_DENSE = 0.01        # the clone / split limit is 0.04
GRAD = ("eq", "below", "nan", "inf", "neg", "big", "zero")
SCALE = (0.005, 0.005, 0.05, 0.12, 0.15, 0.2, 0.5)      # smax / extent: small twice, large, the world-rule band
QNORM = (1.0, 1e-3, 50.0)
# (P, M, max_screen_size): max_screen_size 20 turns the world-size rule on, None and 0 leave it off
SETS = [(1, 4, 20), (255, 4, 20), (256, 4, 20), (257, 4, 20), (1000, 4, 20), (257, 1, 20), (257, 16, 20), (257, 4, None),
        (257, 4, 0)]
# 10 x the largest 99th percentile, over SETS, of densify_ref in float32 against itself in float64 on the children, relative
# to 1 + |x| (measured, printed and checked by tests/test_densify_edges_cpu.py).  torch's float32 exp and bmm differ in the
# last bit between host CPUs: 1.57e-7 / 5.06e-8 and 1.70e-7 / 5.64e-8 were measured on two of them; the larger pair is kept.
GPU_BOUNDS = {"xyz": 1.70e-6, "scaling": 5.64e-7}


def build(P, M, max_screen_size, seed=None):
    rng = np.random.default_rng(1000 * P + M if seed is None else seed)
    i = rng.permutation(np.arange(P)) if P > 1 else np.zeros(1, np.int64)
    grad, ratio, low = i % 7, np.asarray(SCALE)[(i // 7) % 7], ((i // 49) % 3) == 2
    qn = np.asarray(QNORM)[rng.permutation(np.arange(P)) % 3]
    f = np.float32
    accum, denom = np.zeros(P, f), np.ones(P, f)
    accum[grad == 0] = THR
    accum[grad == 1] = np.nextafter(f(THR), f(0))
    accum[grad == 2], denom[grad == 2] = 0.0, 0.0
    accum[grad == 3], denom[grad == 3] = 1.0, 0.0
    accum[grad == 4] = -2.0 * THR
    accum[grad == 5], denom[grad == 5] = 24.0 * THR, 3.0
    accum[grad == 6], denom[grad == 6] = 0.0, 5.0
    s = ratio[:, None] * EXTENT * rng.uniform(0.3, 0.9, (P, 3))
    s[np.arange(P), rng.integers(0, 3, P)] = ratio * EXTENT
    q = rng.standard_normal((P, 4))
    q *= (qn / np.linalg.norm(q, axis=1))[:, None]
    opacity = np.where(low, np.log(0.002 / 0.998), rng.uniform(-2.0, 3.0, P))
    params = {"xyz": 2.0 * rng.standard_normal((P, 3)), "f_dc": rng.standard_normal((P, 1, 3)),
              "f_rest": rng.standard_normal((P, M - 1, 3)), "scaling": np.log(s), "rotation": q, "opacity": opacity[:, None]}
    params = {k: x.astype(f) for k, x in params.items()}
    m = {k: (1e-3 * rng.standard_normal(x.shape)).astype(f) for k, x in params.items()}
    v = {k: (1e-6 * rng.random(x.shape) + 1e-12).astype(f) for k, x in params.items()}
    return dict(P=P, M=M, params=params, m=m, v=v, accum=accum[:, None], denom=denom[:, None],
                noise=rng.standard_normal((2, P, 3)).astype(f), max_screen_size=max_screen_size,
                grad=np.asarray(GRAD)[grad], ratio=ratio, low=low, qnorm=qn)


def degenerate(kind, P=257, M=4):
    """'all_pruned': every opacity below min_opacity, no gradient.  'unchanged': nothing selected, nothing pruned."""
    d = build(P, M, 20, seed=7 if kind == "unchanged" else 8)
    d["accum"][:], d["denom"][:] = 0.0, 1.0
    d["params"]["scaling"] = (d["params"]["scaling"] - d["params"]["scaling"].max(1, keepdims=True)
                              + np.float32(np.log(0.005 * EXTENT))).astype(np.float32)
    d["params"]["opacity"][:] = -8.0 if kind == "all_pruned" else 1.0
    return d


def run_ref(d, dtype):
    """tests/densify_ref.py on an input set in `dtype`, with a row tag riding along as a seventh 'parameter' (densify_ref
    treats every entry alike).  -> (parameters, exp_avg, exp_avg_sq as numpy dicts, order, keep, clone, child): `order` is
    the original index of every output row, the three masks are the decisions per original Gaussian."""
    P = d["P"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype)  # noqa: E731
    params = {k: t(x) for k, x in d["params"].items()}
    m, v = {k: t(x) for k, x in d["m"].items()}, {k: t(x) for k, x in d["v"].items()}
    params["tag"] = torch.arange(P).reshape(P, 1).to(dtype)
    m["tag"], v["tag"] = torch.ones(P, 1, dtype=dtype), torch.ones(P, 1, dtype=dtype)
    op, om, ov = densify_ref.densify_and_prune(params, m, v, t(d["accum"]), t(d["denom"]), THR, MIN_OPACITY, EXTENT,
                                               d["max_screen_size"], PERCENT_DENSE, t(d["noise"]))
    order = op.pop("tag").reshape(-1).long().numpy()
    n_keep = int(om.pop("tag").sum())
    ov.pop("tag")
    same = (op["scaling"] == params["scaling"][order]).all(dim=1).numpy()   # a child's scaling is log(s / 1.6)
    rest = np.arange(len(order)) >= n_keep
    mask = lambda rows: np.bincount(order[rows], minlength=P) > 0  # noqa: E731
    keep, clone, child = mask(~rest), mask(rest & same), mask(rest & ~same)
    n_clone, n_child = int(clone.sum()), int(child.sum())
    assert len(order) == n_keep + n_clone + 2 * n_child
    # kept | clones | children 0 | children 1, each in index order
    expect = np.concatenate([np.nonzero(keep)[0], np.nonzero(clone)[0], np.nonzero(child)[0], np.nonzero(child)[0]])
    assert np.array_equal(order, expect)
    num = lambda x: {k: y.numpy() for k, y in x.items()}  # noqa: E731
    return num(op), num(om), num(ov), order, keep, clone, child


def child_rows(order, keep, clone):
    return np.arange(len(order)) >= int(keep.sum()) + int(clone.sum())


def child_err(got, ref, rows):
    """|got - ref| / (1 + |ref|) over the children's rows."""
    g, r = np.asarray(got, np.float64)[rows], np.asarray(ref, np.float64)[rows]
    return (np.abs(g - r) / (1.0 + np.abs(r))).reshape(-1)


def populations(d, keep, clone, child):
    """How many Gaussians of every class the issue names the set holds (asserted >= 8 each at P >= 255)."""
    g, r, low, world = d["grad"], d["ratio"], d["low"], bool(d["max_screen_size"])
    small, hot = r < PERCENT_DENSE, np.isin(g, ("eq", "inf", "big"))
    out = {"g == thr, cloned or split": (g == "eq") & ~low & (r < 0.16) & (clone | child),
           "just below thr, neither": (g == "below") & ~clone & ~child,
           "0/0, neither": (g == "nan") & ~clone & ~child,
           "x/0, cloned or split": (g == "inf") & ~low & (r < 0.16) & (clone | child),
           "negative g, small: cloned": (g == "neg") & small & ~low & clone,
           "negative g, large: not split": (g == "neg") & ~small & ~child & ~clone,
           "low opacity, large gradient: gone": hot & low & ~keep & ~clone & ~child,
           "norm 1e-3 among the split": child & (d["qnorm"] == 1e-3), "norm 50 among the split": child & (d["qnorm"] == 50.0)}
    band, wide = hot & ~low & ((r == 0.12) | (r == 0.15)), hot & ~low & ((r == 0.2) | (r == 0.5))
    if world:
        out["world rule: children of 0.12 / 0.15 survive"] = band & child
        out["world rule: children of 0.2 / 0.5 dropped"] = wide & ~child & ~keep
        out["world rule: unselected parent of 0.12+ dropped"] = ~hot & ~low & (r > 0.1) & ~keep
    else:
        out["world rule off: every wide one split"] = (band | wide) & child
        out["world rule off: unselected wide parent kept"] = ~hot & ~low & (r > 0.1) & keep
    return {k: int(x.sum()) for k, x in out.items()}
