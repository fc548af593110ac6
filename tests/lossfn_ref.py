"""A float64 restatement of the drop-in loss functions (binocular3dgs_amd/csrc/lossfn.hip: l1_loss, ssim, SmoothLoss,
inverse_warp_images, opacity_decay, add_densification_stats, apply_staged_densify_stats) on the CPU, the table of cases
that tests/test_lossfn_ref_cpu.py and tests/test_gpu_lossfn_parity.py share, the per-element "flip budget", the bound
both files apply, and the mutants that show the bound has teeth.  Imports nothing from the package: the PyTorch statement
(binocular3dgs_amd/loss.py) is handed in where it is needed.

    l1      mean |x m - y m| (m absent, [B,1,H,W] or of x's shape); gradients for x, y and m
    ssim    11x11 window of loss_ref.make_window(), zero padding, every plane by itself; one mean, or one per batch element
            (then the scalar that is differentiated is sum_b gw[b] * value[b], gw distinct per element)
    smooth  mean over the interior of |exp(-0.33 |sum_c dx(image_c)|) dx(disparity)|, plus the same along y
    warp    out = (x0+1-d) img[c+x0] + (d-x0) img[c+x0+1], x0 = floor(d); zero where a tap leaves the row, and -- the kernel's
            documented guard, where the reference's cast is undefined -- wherever not |d| < 1e6 (inf, NaN): output and both
            gradients are zero there.  The scalar that is differentiated is sum(out * up).
    opacity logit(sigmoid(o) * factor)
    densify accum[f] += ||grad[f, :2]||, denom[f] += 1 on the rows the filter selects
    staged  agreed == 0: accum += st_accum, denom += st_denom, maxrad = max(maxrad, st_maxrad); else nothing, and the local
            flag is raised; staging zero afterwards either way

Kinks and the flip budget.  |.| at 0 (l1, smooth), sgn of the summed image derivative (smooth) and floor(d) at integers
(warp) are where float32 may legitimately land on the other side.  The inputs are built away from them -- l1 residuals
are at least 0.05 * 0.25 or exactly 0, every disparity of a warp case is an exact integer or at least 0.05 from one -- and
whatever remains (random ties of the smoothness term) gets a per-element budget: twice the magnitude of the term whose
sign could flip, for 0 < |u| < TAU * max|u|.  Exact zeros are not fragile: float32 and float64 agree on them bit for bit.

Bound (check()), element-wise:  |got - ref64| <= F * max(E32, 1e-7 * max|ref64|) + budget      gradients and images
                                |got - ref64| <= F * max(E32, 1e-6 * |ref64|)                   scalar values
E32 = max |statement in float32 on the CPU - ref64| of that case and tensor (element-wise for the values); an element
that is exactly zero in the reference and in the float32 statement, and has no budget, must be exactly zero.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from loss_ref import CAP, FLOOR_MARGIN, TAU, make_window, window2d  # noqa: F401

F_MAX = 16.0
GUARD = 1.0e6
D = torch.float64
SCALARS = ("value",)


def _fragile(u):
    a = u.detach().abs()
    top = float(a.max()) if a.numel() else 0.0
    return ((a > 0) & (a < TAU * top)).to(D)


def _leaf(t):
    return t.detach().clone().to(D).requires_grad_(True)


def _np(t):
    return t.detach().double().numpy().copy()


# ------------------------------------------------------------------------------------------------------------- ssim
def _ssim_map(x, y, w2d, drop_tap=False):
    C = x.shape[1]
    w = w2d.to(x.dtype).expand(C, 1, 11, 11).contiguous()

    def conv(t):
        out = F.conv2d(t, w, padding=5, groups=C)
        # mutant: the workgroup that ends at column 32k+31 loads a halo one column short on its far side, so the last
        # output column of the tile loses the tap at +5 (input column c+5 reaches output column c through that tap only)
        cols = [c for c in range(31, t.shape[-1] - 5, 32)] if drop_tap else []
        if cols:
            out = out.clone()
            for c in cols:
                t2 = t.clone()
                t2[..., c + 5] = 0
                out[..., c] = F.conv2d(t2, w, padding=5, groups=C)[..., c]
        return out
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def ssim_workgroups(case):
    B, C, H, W = case["x"].shape
    return B * C * ((H + 31) // 32) * ((W + 31) // 32)


def _ref_ssim(case, mut, w2d):
    x, y = _leaf(case["x"]), _leaf(case["y"])
    S = _ssim_map(x, y, window2d() if w2d is None else w2d, drop_tap=mut == "drop_tap")
    B, C, H, W = S.shape
    if case["size_average"]:
        v, gw = S.mean(), None
        L = v
    else:
        v, gw = S.mean((1, 2, 3)), case["gw"].to(D)
        L = (v * (gw[0].expand(B) if mut == "shared_weight" else gw)).sum()
    g1, g2 = torch.autograd.grad(L, [x, y])
    v = v.detach().clone()
    if mut == "skip_partial":       # the fold stops one partial short: the last workgroup (last plane, last tile) is left out
        r0, c0 = ((H - 1) // 32) * 32, ((W - 1) // 32) * 32
        lost = S.detach()[B - 1, C - 1, r0:, c0:].sum()
        if case["size_average"]:
            v -= lost / (B * C * H * W)
        else:
            v[B - 1] -= lost / (C * H * W)
    z = np.zeros((B, C, H, W))
    return dict(value=_np(v), g_img1=_np(g1), g_img2=_np(g2), budget=dict(g_img1=z, g_img2=z))


def _stmt_ssim(stmt, case, dtype):
    x, y = (case[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "y"))
    v = stmt.ssim(x, y, size_average=case["size_average"])
    L = v if case["size_average"] else (v * case["gw"].to(dtype)).sum()
    g1, g2 = torch.autograd.grad(L, [x, y])
    return dict(value=_np(v), g_img1=_np(g1), g_img2=_np(g2))


# --------------------------------------------------------------------------------------------------------------- l1
def _ref_l1(case, mut, w2d):
    x, y = _leaf(case["x"]), _leaf(case["y"])
    m = None if case["mask"] is None else _leaf(case["mask"])
    u = (x - y) if m is None else (x * m - y * m)
    a = u.abs()
    if mut == "sgn0":               # mutant: sgn(0) = 1 -- the same value, a gradient where the reference has none
        a = a + (u.detach() == 0).to(D) * u
    v = a.mean()
    ins = [x, y] + ([] if m is None else [m])
    gr = torch.autograd.grad(v, ins)
    n = float(u.numel())
    fr = _fragile(u)
    mm = torch.ones_like(u) if m is None else m.detach().abs().expand_as(u)
    out = dict(value=_np(v), g_x=_np(gr[0]), g_y=_np(gr[1]), budget=dict(g_x=_np(2.0 * mm / n * fr), g_y=_np(2.0 * mm / n * fr)))
    if m is not None:
        b = 2.0 * (x - y).detach().abs() / n * fr
        out["g_mask"] = _np(gr[2])
        out["budget"]["g_mask"] = _np(b if m.shape == u.shape else b.sum(1, keepdim=True))
    return out


def _stmt_l1(stmt, case, dtype):
    x, y = (case[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "y"))
    m = None if case["mask"] is None else case["mask"].detach().clone().to(dtype).requires_grad_(True)
    v = stmt.l1_loss(x, y, mask=m)
    gr = torch.autograd.grad(v, [x, y] + ([] if m is None else [m]))
    out = dict(value=_np(v), g_x=_np(gr[0]), g_y=_np(gr[1]))
    if m is not None:
        out["g_mask"] = _np(gr[2])
    return out


# ------------------------------------------------------------------------------------------------------------- warp
def guarded(d):
    """Where the kernel's `|d| < 1e6` guard refuses the pixel (inf and NaN included)."""
    return ~(d.abs() < GUARD)


def _ref_warp(case, mut, w2d):
    img, d = _leaf(case["image"]), _leaf(case["disp"])
    up = case["up"].to(D)
    B, C, H, W = img.shape
    ok = ~guarded(d.detach())
    dd = torch.where(ok, d, torch.zeros((), dtype=D))           # (no gradient, and no NaN, through a refused pixel)
    x0 = torch.floor(dd.detach())
    c0 = torch.arange(W).view(1, 1, 1, W) + x0.long()
    c1 = c0 + 1
    valid = ok & (c0 >= 0) & (c0 < W) & (c1 >= 0) & (c1 < W)
    if mut == "clamp":              # mutant: the taps are clamped to the row instead of the pixel being zeroed
        valid = ok
    w0, w1 = (x0 + 1.0) - dd, dd - x0
    if mut == "swap":               # mutant: the two interpolation weights change places
        w0, w1 = w1, w0
    i0, i1 = c0.clamp(0, W - 1).expand(B, C, H, W), c1.clamp(0, W - 1).expand(B, C, H, W)
    out = torch.where(valid, w0 * torch.gather(img, 3, i0) + w1 * torch.gather(img, 3, i1), torch.zeros((), dtype=D))
    g_img, g_d = torch.autograd.grad((out * up).sum(), [img, d])
    z = np.zeros
    return dict(out=_np(out), g_image=_np(g_img), g_disp=_np(g_d), valid=valid.numpy(), c0=c0.numpy(),
                budget=dict(out=z((B, C, H, W)), g_image=z((B, C, H, W)), g_disp=z((B, 1, H, W))))


def statement_disparity(case):
    """The disparity the PyTorch statement is handed: a refused pixel (where the statement's cast is undefined and its
    gradient NaN) is replaced by a finite disparity of the same sign that leaves the row -- zeros by the statement's own
    rule, which is what the kernel documents for them."""
    d = case["disp"].clone()
    W = d.shape[-1]
    bad = guarded(d)
    d[bad] = torch.where(d[bad] < 0, torch.tensor(-(3.0 * W + 0.5)), torch.tensor(3.0 * W + 0.5))
    return d


def _stmt_warp(stmt, case, dtype):
    img = case["image"].detach().clone().to(dtype).requires_grad_(True)
    d = statement_disparity(case).to(dtype).requires_grad_(True)
    out = stmt.inverse_warp_images(img, d)
    g_img, g_d = torch.autograd.grad((out * case["up"].to(dtype)).sum(), [img, d])
    return dict(out=_np(out), g_image=_np(g_img), g_disp=_np(g_d))


# ----------------------------------------------------------------------------------------------------------- smooth
def _dx(t):
    return 0.5 * (t[..., 1:-1, 2:] - t[..., 1:-1, :-2])


def _dy(t):
    return 0.5 * (t[..., 2:, 1:-1] - t[..., :-2, 1:-1])


def _ref_smooth(case, mut, w2d):
    disp, img = _leaf(case["disp"]), _leaf(case["image"])
    B, C, H, W = img.shape
    ax, ay = _dx(img).sum(1, keepdim=True), _dy(img).sum(1, keepdim=True)
    ex, ey = torch.exp(ax.abs() * -0.33), torch.exp(ay.abs() * -0.33)
    ddx, ddy = _dx(disp), _dy(disp)
    vx, vy = ex * ddx, ey * ddy
    v = vx.abs().mean() + vy.abs().mean()
    g_d, g_i = torch.autograd.grad(v, [disp, img])
    c = 1.0 / float(B * (H - 2) * (W - 2))
    bd, bi = torch.zeros(B, 1, H, W, dtype=D), torch.zeros(B, 1, H, W, dtype=D)
    tx, ty = ex.detach() * c * _fragile(ddx), ey.detach() * c * _fragile(ddy)            # 2 * 0.5 * ex / count
    sx, sy = 0.33 * vx.detach().abs() * c * _fragile(ax), 0.33 * vy.detach().abs() * c * _fragile(ay)
    for b_, px, py in ((bd, tx, ty), (bi, sx, sy)):
        b_[..., 1:-1, 2:] += px
        b_[..., 1:-1, :-2] += px
        b_[..., 2:, 1:-1] += py
        b_[..., :-2, 1:-1] += py
    return dict(value=_np(v), g_disp=_np(g_d), g_image=_np(g_i), ax=_np(ax), ay=_np(ay), ddx=_np(ddx), ddy=_np(ddy),
                budget=dict(g_disp=_np(bd), g_image=_np(bi.expand(B, C, H, W))))


def _stmt_smooth(stmt, case, dtype):
    disp, img = (case[k].detach().clone().to(dtype).requires_grad_(True) for k in ("disp", "image"))
    v = stmt.smooth_loss(disp, img)
    g_d, g_i = torch.autograd.grad(v, [disp, img])
    return dict(value=_np(v), g_disp=_np(g_d), g_image=_np(g_i))


# ------------------------------------------------------------------------------------------- the model's statements
def _ref_opacity(case, mut, w2d):
    s = torch.sigmoid(case["o"].to(D)) * float(case["factor"])
    return dict(out=_np(torch.log(s / (1.0 - s))), budget=dict(out=np.zeros(tuple(case["o"].shape))))


def _stmt_opacity(stmt, case, dtype):
    # (`factor` is the Python float the method is handed: torch multiplies a float32 tensor by it in float32)
    return dict(out=_np(stmt.inverse_sigmoid(torch.sigmoid(case["o"].to(dtype)) * float(case["factor"]))))


def densify_grads(case):
    """The [P,2+] views with row stride case['stride'] that the calls are handed (views of the case's own buffers)."""
    return [buf[:, :2] for buf in case["bufs"]]


def _densify(case, dtype):
    acc, den = case["accum"].to(dtype).clone(), case["denom"].to(dtype).clone()
    f = case["filter"]
    for g in densify_grads(case):
        acc[f] += torch.norm(g.to(dtype)[f, :2], dim=-1, keepdim=True)
        den[f] += 1
    return dict(accum=_np(acc), denom=_np(den))


def _ref_densify(case, mut, w2d):
    out = _densify(case, D)
    out["budget"] = dict(accum=np.zeros_like(out["accum"]), denom=np.zeros_like(out["denom"]))
    return out


def _stmt_densify(stmt, case, dtype):
    return _densify(case, dtype)


def _staged(case, dtype):
    acc, den, rad = (case[k].to(dtype).clone() for k in ("accum", "denom", "maxrad"))
    if case["agreed"] == 0:
        acc, den = acc + case["st_accum"].to(dtype), den + case["st_denom"].to(dtype)
        rad = torch.maximum(rad, case["st_maxrad"].to(dtype))
    return dict(accum=_np(acc), denom=_np(den), maxrad=_np(rad))


def _ref_staged(case, mut, w2d):
    out = _staged(case, D)
    out["flag"] = int(case["flag"]) | int(case["agreed"] != 0)
    out["budget"] = {k: np.zeros_like(out[k]) for k in ("accum", "denom", "maxrad")}
    return out


def _stmt_staged(stmt, case, dtype):
    return _staged(case, dtype)


_REF = dict(ssim=_ref_ssim, l1=_ref_l1, warp=_ref_warp, smooth=_ref_smooth, opacity=_ref_opacity, densify=_ref_densify,
            staged=_ref_staged)
_STMT = dict(ssim=_stmt_ssim, l1=_stmt_l1, warp=_stmt_warp, smooth=_stmt_smooth, opacity=_stmt_opacity, densify=_stmt_densify,
             staged=_stmt_staged)
KEYS = dict(ssim=("value", "g_img1", "g_img2"), l1=("value", "g_x", "g_y", "g_mask"), warp=("out", "g_image", "g_disp"),
            smooth=("value", "g_disp", "g_image"), opacity=("out",), densify=("accum", "denom"), staged=("accum", "denom", "maxrad"))


def keys_of(case):
    return tuple(k for k in KEYS[case["kind"]] if not (k == "g_mask" and case["mask"] is None))


def reference(case, mut=None, w2d=None):
    """Results of a case in float64 (numpy), with `budget` per tensor.  mut: one of MUTANTS' mutations; w2d: another 2-D
    window (the comparison with the statement in float64 hands in the statement's own)."""
    return _REF[case["kind"]](case, mut, w2d)


def statement(stmt, case, dtype):
    """The PyTorch statement (`stmt`: an object with l1_loss, ssim, smooth_loss, inverse_warp_images, inverse_sigmoid) on the
    CPU in `dtype`; results as float64 numpy."""
    return _STMT[case["kind"]](stmt, case, dtype)


# ------------------------------------------------------------------------------------------------------------ bound
def e32_of(stmt, name):
    """(E32 per result, the float32 statement's results).  E32 of an opacity case is taken over the elements whose float32
    statement is finite: the others are compared as a pattern, not as numbers."""
    case, ref = get_case(name), ref_of(name)
    st = statement(stmt, case, torch.float32)
    out = {}
    for k in keys_of(case):
        err = np.abs(st[k] - ref[k])
        if k in SCALARS:
            out[k] = err
        else:
            err = err[np.isfinite(st[k])]
            out[k] = float(err.max()) if err.size else 0.0
    return out, st


def ratio_of(key, got, ref, e32, budget):
    """Largest error of `got` over the floor of the bound (the budget taken off first), over the elements that are finite
    in `got`; 0 for an empty tensor."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (key, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    if key in SCALARS:
        floor = np.maximum(e32, 1e-6 * np.abs(ref))
        err = np.abs(got - ref)
    else:
        floor = np.full(ref.shape, max(e32, 1e-7 * float(np.abs(ref).max())))
        err = np.maximum(np.abs(got - ref) - budget, 0.0)
    fin = np.isfinite(got)
    err, floor = err[fin], floor[fin]
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, np.where(floor > 0, err / floor, np.inf))
    return float(r.max())


def exact_zeros_hold(key, got, ref, st32, budget=None):
    """An element that is exactly zero in the reference and in the float32 statement (and has no budget) is exactly zero."""
    z = (ref == 0) & (st32 == 0)
    if budget is not None:
        z &= budget == 0
    return bool(np.all(np.asarray(got)[z] == 0))


def check(stmt, name, got, f_of, keys=None):
    """Asserts the bound on every key of `got` (or `keys`); returns {key: ratio}.  f_of: key -> F."""
    case, ref = get_case(name), ref_of(name)
    e32, st = e32_of(stmt, name)
    rat = {}
    for k in (keys or [k for k in keys_of(case) if k in got]):
        g = np.asarray(got[k], dtype=np.float64)
        bud = None if k in SCALARS else ref["budget"][k]
        if case["kind"] == "opacity":       # the pattern of infinities (and NaN) is the float32 statement's
            assert np.array_equal(np.isposinf(g), np.isposinf(st[k])) and np.array_equal(np.isneginf(g), np.isneginf(st[k])) \
                and np.array_equal(np.isnan(g), np.isnan(st[k])), (name, k, g[~np.isfinite(g) | ~np.isfinite(st[k])])
        else:
            assert np.all(np.isfinite(g)), (name, k)
        rat[k] = ratio_of(k, g, ref[k], e32[k], bud)
        assert exact_zeros_hold(k, g, ref[k], st[k], bud), (name, k, "a non-zero where the reference has an exact zero")
    print(name, {k: round(v, 3) for k, v in rat.items()})
    assert all(v <= f_of(k) for k, v in rat.items()), (name, rat)
    return rat


def old_criterion(key, got, ref32):
    """The criterion of tests/test_gpu_lossfn.py and test_gpu_lossfn_edges.py: max|a-b| / max|b| against the float32 statement,
    at most 2e-4 per tensor and 3e-5 per value.  Returns (passes, the figure)."""
    top = max(float(np.abs(ref32).max()), 1e-30)
    rel = float(np.abs(np.asarray(got) - ref32).max()) / top
    return rel <= (3e-5 if key in SCALARS else 2e-4), rel


# ------------------------------------------------------------------------------------------------------------ cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pair(gen, *shape):
    """Two images at least 0.05 apart everywhere."""
    r = lambda: torch.rand(*shape, generator=gen)  # noqa: E731
    x = r()
    return x, x + ((r() > 0.5).float() * 2 - 1) * (0.05 + 0.15 * r())


def _ssim_case(seed, B, C, H, W, size_average=True, content="random"):
    gen = _gen(seed)
    x, y = torch.rand(B, C, H, W, generator=gen), torch.rand(B, C, H, W, generator=gen)
    if content == "same":
        y = x.clone()
    elif content == "const":
        x, y = torch.full((B, C, H, W), 0.25), torch.full((B, C, H, W), 0.625)
    elif content == "zeros":
        x, y = torch.zeros(B, C, H, W), torch.zeros(B, C, H, W)
    gw = 0.5 + 0.25 * torch.arange(B, dtype=torch.float32)          # distinct per batch element, exact in float32
    return dict(kind="ssim", x=x, y=y, size_average=size_average, gw=gw)


def _l1_case(seed, B, C, H, W, mask=None, equal=False):
    """mask: None | 'chan' ([B,1,H,W]) | 'full'.  equal: blocks where x == y exactly.  A mask holds exact zeros and negative
    values, and is at least 0.25 in magnitude elsewhere."""
    gen = _gen(seed)
    x, y = _pair(gen, B, C, H, W)
    n = H * W
    if equal:
        flat_x, flat_y = x.view(B, C, n), y.view(B, C, n)
        flat_y[:, :, : max(1, n // 7)] = flat_x[:, :, : max(1, n // 7)]                # a run from the first pixel on
        flat_y[:, 0, n // 2: n // 2 + max(1, n // 9)] = flat_x[:, 0, n // 2: n // 2 + max(1, n // 9)]     # one channel only
    m = None
    if mask is not None:
        shp = (B, 1, H, W) if mask == "chan" else (B, C, H, W)
        u, s = torch.rand(*shp, generator=gen), torch.rand(*shp, generator=gen)
        m = (0.25 + 0.75 * u) * ((s > 0.3).float() * 2 - 1)
        m[torch.rand(*shp, generator=gen) < 0.2] = 0.0
    return dict(kind="l1", x=x, y=y, mask=m)


WARP_ROWS = ("edges", "ints", "guard", "random", "collect", "random", "edges")
GUARD_VALUES = (999999.9375, 1.0e6, -1.0e6, float("inf"), float("-inf"), float("nan"))


def _warp_case(seed, B, C, W):
    """One row per entry of WARP_ROWS in every batch element:
    edges    c + floor(d) lands on -1, 0, W-2, W-1 in turn, d fractional
    ints     d = 0, 1, -1, W-1, -(W-1) in turn
    guard    GUARD_VALUES in turn
    random   floor in [-1.2 W, 1.2 W], fraction in [0.05, 0.95]
    collect  d falls by 1 per column over runs of twelve: c + floor(d) stays put, one column collects the run
    The upstream gradient has exact-zero blocks."""
    gen = _gen(seed)
    H = len(WARP_ROWS)
    r = lambda *s: torch.rand(*s, generator=gen, dtype=D)  # noqa: E731
    cols = torch.arange(W, dtype=D)
    d = torch.zeros(B, 1, H, W, dtype=D)
    for b in range(B):
        for h, kind in enumerate(WARP_ROWS):
            frac = 0.3 + 0.4 * r(W)
            if kind == "edges":
                tgt = torch.tensor([(-1, 0, W - 2, W - 1)[(c + b + h) % 4] for c in range(W)], dtype=D)
                row = tgt - cols + frac
            elif kind == "ints":
                row = torch.tensor([(0, 1, -1, W - 1, -(W - 1))[(c + b) % 5] for c in range(W)], dtype=D)
            elif kind == "guard":
                row = torch.tensor([GUARD_VALUES[(c + b + 3) % 6] for c in range(W)], dtype=D)
            elif kind == "random":
                row = torch.floor((r(W) * 2 - 1) * 1.2 * W) + 0.05 + 0.9 * r(W)
            else:
                row = 12.0 - (cols % 12) + frac
            d[b, 0, h] = row
    up = torch.rand(B, C, H, W, generator=gen) - 0.3
    up[:, :, 1::3, : max(1, W // 3)] = 0.0
    if C > 1:
        up[:, C // 2, :, W // 2:] = 0.0
    return dict(kind="warp", image=torch.rand(B, C, H, W, generator=gen), disp=d.float(), up=up)


def _smooth_case(seed, B, C, H, W, blocks=False):
    """blocks (17x33): rows 2..7 x columns 3..12 flat disparity; rows 9..15 x columns 3..12 flat image; rows 2..15 x columns
    18..30 an image whose channel derivatives cancel exactly (multiples of 1/256: ch0 = q, ch1 = 1 - q, ...; C = 1: flat)."""
    gen = _gen(seed)
    disp, img = torch.rand(B, 1, H, W, generator=gen) * 3.0, torch.rand(B, C, H, W, generator=gen)
    if blocks:
        disp[:, :, 2:8, 3:13] = 1.375
        img[:, :, 9:16, 3:13] = 0.5
        q = torch.randint(0, 257, (B, 1, 14, 13), generator=gen).float() / 256.0
        for ch in range(C):
            img[:, ch:ch + 1, 2:16, 18:31] = 0.5 if (C % 2 and ch == C - 1) else (q if ch % 2 == 0 else 1.0 - q)
    return dict(kind="smooth", disp=disp, image=img)


def _opacity_case(seed, n=None, values=None, factor=0.995):
    o = torch.tensor(values, dtype=torch.float32) if values is not None else torch.rand(n, generator=_gen(seed)) * 40.0 - 20.0
    return dict(kind="opacity", o=o.view(-1, 1), factor=factor)


def _densify_case(seed, P, stride, filt):
    gen = _gen(seed)
    f = dict(none=torch.zeros(P, dtype=torch.bool), all=torch.ones(P, dtype=torch.bool), alt=torch.arange(P) % 2 == 0)[filt]
    return dict(kind="densify", stride=stride, filter=f, bufs=[torch.randn(P, stride, generator=gen) for _ in range(2)],
                accum=torch.rand(P, 1, generator=gen), denom=torch.randint(0, 5, (P, 1), generator=gen).float())


def _staged_case(seed, P, agreed, flag=0):
    """Every third row has nothing staged (all three values zero) and holds -0.0 / odd values in the model's arrays, which
    an `x += 0` would not leave bit for bit."""
    gen = _gen(seed)
    r = lambda: torch.rand(P, generator=gen)  # noqa: E731
    c = dict(kind="staged", agreed=agreed, flag=flag, st_accum=r(), st_denom=torch.randint(1, 4, (P,), generator=gen).float(),
             st_maxrad=r() * 50, accum=r(), denom=torch.randint(0, 9, (P,), generator=gen).float(), maxrad=r() * 50)
    idle = torch.arange(P) % 3 == 1
    for k in ("st_accum", "st_denom", "st_maxrad"):
        c[k][idle] = 0.0
    c["st_accum"][torch.arange(P) % 3 == 2] = 0.0         # (a row with only some of the three staged is still applied)
    c["accum"][idle] = -0.0
    c["idle"] = idle
    return c


_B = {
    # ssim: sizes, B = 1, C = 3, two different random images
    "ssim_1x1": lambda: _ssim_case(1, 1, 3, 1, 1),
    "ssim_5x4": lambda: _ssim_case(2, 1, 3, 5, 4),
    "ssim_11x11": lambda: _ssim_case(3, 1, 3, 11, 11),
    "ssim_32x32": lambda: _ssim_case(4, 1, 3, 32, 32),
    "ssim_33x32": lambda: _ssim_case(5, 1, 3, 33, 32),
    "ssim_31x33": lambda: _ssim_case(6, 1, 3, 31, 33),
    "ssim_37x37": lambda: _ssim_case(7, 1, 3, 37, 37),
    "ssim_64x65": lambda: _ssim_case(8, 1, 3, 64, 65),
    "ssim_6x70": lambda: _ssim_case(9, 1, 3, 6, 70),
    "ssim_same_33x32": lambda: _ssim_case(10, 1, 3, 33, 32, content="same"),
    "ssim_const_33x32": lambda: _ssim_case(11, 1, 3, 33, 32, content="const"),
    "ssim_zeros_33x32": lambda: _ssim_case(12, 1, 3, 33, 32, content="zeros"),
    # ssim: workgroup counts across the edges of the 64 arrival slots
    "ssim_nb1": lambda: _ssim_case(21, 1, 1, 8, 8),
    "ssim_nb2": lambda: _ssim_case(22, 1, 2, 8, 8),
    "ssim_nb63_avg": lambda: _ssim_case(23, 21, 3, 8, 8),
    "ssim_nb63_per": lambda: _ssim_case(23, 21, 3, 8, 8, size_average=False),
    "ssim_nb64_avg": lambda: _ssim_case(24, 16, 4, 8, 8),
    "ssim_nb64_per": lambda: _ssim_case(24, 16, 4, 8, 8, size_average=False),
    "ssim_nb65_avg": lambda: _ssim_case(25, 13, 5, 8, 8),
    "ssim_nb65_per": lambda: _ssim_case(25, 13, 5, 8, 8, size_average=False),
    "ssim_nb129_avg": lambda: _ssim_case(26, 43, 3, 8, 8),
    "ssim_nb129_per": lambda: _ssim_case(26, 43, 3, 8, 8, size_average=False),
    "ssim_nb128_avg": lambda: _ssim_case(27, 16, 2, 33, 33),
    "ssim_nb128_per": lambda: _ssim_case(27, 16, 2, 33, 33, size_average=False),
    # l1: 1, 63, 64, 65 workgroups, above the 512-block cap, the three mask forms, x == y
    "l1_1x1": lambda: _l1_case(101, 1, 1, 1, 1),
    "l1_1x1_chan": lambda: _l1_case(102, 1, 3, 1, 1, mask="chan"),
    "l1_126x128": lambda: _l1_case(103, 1, 1, 126, 128),
    "l1_128x128_eq": lambda: _l1_case(104, 1, 1, 128, 128, equal=True),
    "l1_128x128_chan_eq": lambda: _l1_case(105, 1, 3, 128, 128, mask="chan", equal=True),
    "l1_1x16385": lambda: _l1_case(106, 1, 1, 1, 16385),
    "l1_1x16385_full": lambda: _l1_case(107, 2, 1, 1, 16385, mask="full"),
    "l1_cap_300x450_eq": lambda: _l1_case(108, 1, 3, 300, 450, equal=True),
    "l1_cap_300x450_chan": lambda: _l1_case(109, 1, 3, 300, 450, mask="chan"),
    "l1_3x4x17x19": lambda: _l1_case(110, 3, 4, 17, 19),
    "l1_3x4x17x19_chan": lambda: _l1_case(111, 3, 4, 17, 19, mask="chan"),
    "l1_3x4x17x19_full_eq": lambda: _l1_case(112, 3, 4, 17, 19, mask="full", equal=True),
    "l1_2x1x9x5_full": lambda: _l1_case(113, 2, 1, 9, 5, mask="full"),
    # warp
    "warp_w1": lambda: _warp_case(201, 1, 1, 1),
    "warp_w2": lambda: _warp_case(202, 3, 3, 2),
    "warp_w3": lambda: _warp_case(203, 1, 5, 3),
    "warp_w17": lambda: _warp_case(204, 3, 1, 17),
    "warp_w40": lambda: _warp_case(205, 1, 3, 40),
    "warp_w40_b3c5": lambda: _warp_case(206, 3, 5, 40),
    # smooth
    "smooth_3x3": lambda: _smooth_case(301, 1, 1, 3, 3),
    "smooth_3x40": lambda: _smooth_case(302, 2, 3, 3, 40),
    "smooth_40x3": lambda: _smooth_case(303, 1, 4, 40, 3),
    "smooth_4x4": lambda: _smooth_case(304, 2, 1, 4, 4),
    "smooth_17x33_c1": lambda: _smooth_case(305, 1, 1, 17, 33, blocks=True),
    "smooth_17x33_c3": lambda: _smooth_case(306, 2, 3, 17, 33, blocks=True),
    "smooth_17x33_c4": lambda: _smooth_case(307, 1, 4, 17, 33, blocks=True),
    "smooth_cap_513x512": lambda: _smooth_case(308, 1, 1, 513, 512),
    # opacity_decay
    "opacity_n0": lambda: _opacity_case(401, n=0),
    "opacity_n1": lambda: _opacity_case(402, n=1),
    "opacity_n255": lambda: _opacity_case(403, n=255),
    "opacity_n256": lambda: _opacity_case(404, n=256),
    "opacity_n257": lambda: _opacity_case(405, n=257),
    "opacity_extreme": lambda: _opacity_case(0, values=[-104.0, -88.0, 17.0, 30.0, 89.0]),
    "opacity_factor1_at_17": lambda: _opacity_case(0, values=[17.0], factor=1.0),
    # add_densification_stats
    "densify_p0": lambda: _densify_case(501, 0, 3, "all"),
    "densify_p1_s2": lambda: _densify_case(502, 1, 2, "all"),
    "densify_p257_s2_alt": lambda: _densify_case(503, 257, 2, "alt"),
    "densify_p257_s3_all": lambda: _densify_case(504, 257, 3, "all"),
    "densify_p257_s4_alt": lambda: _densify_case(505, 257, 4, "alt"),
    "densify_p257_s4_none": lambda: _densify_case(506, 257, 4, "none"),
    # apply_staged_densify_stats
    "staged_keep_p257": lambda: _staged_case(601, 257, 0),
    "staged_drop_p257": lambda: _staged_case(602, 257, 5),
    "staged_keep_sticky_p257": lambda: _staged_case(603, 257, 0, flag=1),
    "staged_keep_p1": lambda: _staged_case(604, 1, 0),
    "staged_drop_p0": lambda: _staged_case(605, 0, -1),
    "staged_keep_p0": lambda: _staged_case(606, 0, 0),
}
CASES = tuple(_B)


def names(kind):
    return tuple(n for n in CASES if n.split("_")[0] == kind)


@functools.lru_cache(maxsize=None)
def get_case(name):
    c = _B[name]()
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """The reference of a case: computed once, shared, never written to."""
    out = reference(get_case(name))
    for v in list(out.values()) + list(out["budget"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------- mutants
# (mutation, the case it must break, the result it must break it on): the reference is mutated, rounded to float32, and
# must miss the bound with F at its ceiling F_MAX
MUTANTS = (
    ("drop_tap", "ssim_64x65", "g_img1"),            # the outermost tap on the far side of a 32 seam
    ("drop_tap", "ssim_37x37", "g_img2"),
    ("drop_tap", "ssim_64x65", "value"),
    ("swap", "warp_w40", "out"),
    ("swap", "warp_w40", "g_disp"),
    ("clamp", "warp_w3", "out"),
    ("clamp", "warp_w17", "g_image"),
    ("skip_partial", "ssim_nb129_avg", "value"),
    ("skip_partial", "ssim_nb128_per", "value"),
    ("shared_weight", "ssim_nb65_per", "g_img1"),
    ("sgn0", "l1_128x128_eq", "g_x"),
    ("sgn0", "l1_3x4x17x19_full_eq", "g_mask"),
)
