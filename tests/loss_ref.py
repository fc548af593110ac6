"""A float64 restatement of the fused loss block (binocular3dgs_amd/csrc/loss.hip) on the CPU, the table of edge cases
that tests/test_loss_ref_cpu.py and tests/test_gpu_loss_edges.py share, and the per-element "flip budget" that says where
a float32 implementation may legitimately take the other sign of an absolute value.  Imports nothing from the package.

    total = (1-l)*L1(image, gt) + l*(1 - SSIM(image, gt))
          + L1(warp(shifted, d)*m, gt*m) + lambda_smooth * smooth(d*m, gt)
          + mean(|alpha| * alpha_weight)
    d = k_disp / (depth + 1e-5),  k_disp = float32(focal_x) * float32(-trans_dist)   (the float32 product the host forms)
    warp: linear interpolation between columns c+floor(d) and c+floor(d)+1, zero where either leaves the image;
    m = (x1-d)+(d-x0) there, 0 elsewhere;  smooth: central differences on the interior, weighted by exp(-0.33|d gt|),
    defined as 0 where H <= 2 or W <= 2 (the kernel's `inner > 0.f`; PyTorch's mean over nothing would be NaN).
The SSIM window is make_window()'s: double exp, rounded to float32, summed and normalised in float32 in index order; the 2-D
window is the exact product of two such weights (the kernel is separable).  Gradients: float64 autograd.

Sensitivity (a case that cannot pass if the item is wrong by one pixel or one lane):
  SSIM halo (LR = 5, zero padding)      ssim_11x11, ssim_32x32, ssim_33x33: every window crosses the image border and, at 33,
                                        the tile seam; one tap less or more moves every output by about w[0] = 1e-3 relative
  16-seam guard of take / given         seam_alias_48x19: floor(d) of (row+1, tile column 0) is floor(d) of (row, tile column 15)
                                        plus 16, so without `tx < LT-1` / `tx > 0` the last lane of a row would take the first
                                        lane of the NEXT row (n_c0 == c1 holds); d_merge_48x19: the run crosses 15|16|17 and
                                        31|32 with has == false blocks on the seam, a guard one lane early drops a tap there
  |d| >= 1e6 guard                      f_uncov_k16_40x24 (d = 1.6e6, refused by the guard) next to f_uncov_k4_40x24 (d = 4e5,
                                        refused by the range test): identical observable outcome is what is pinned -- m = 0,
                                        D' = 0, gradient finite and 0.  At these widths the guard can only change pixels whose
                                        taps are outside the image anyway; it is there for the int conversion, not the value
  border test of gx_at / gy_at          smooth_3x3 (one interior location), smooth_3x40 / smooth_40x3 (one interior row /
                                        column), smooth_4x4: a location more or less is a whole term of the mean
  per-pair early return                 the mixed batch (BATCH): 1x1, 3x40 and 16x16 pairs in a grid sized for 65x34; a return
                                        one tile early loses the one-column tiles of 33x17 and 65x34.  (One tile late is
                                        harmless by construction: every access behind it is bounds-checked.)
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
TAU = 1e-5           # fragile: 0 < |u| < TAU * max|u| of that argument in the case
FLOOR_MARGIN = 1e-3  # no disparity closer than this to an integer where a tap could be inside
CAP = 0.005          # largest share of elements with a budget, per case and gradient tensor


def make_window():
    g = [np.float32(math.exp(-float((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5))) for k in range(11)]
    tot = np.float32(0.0)
    for v in g:
        tot = np.float32(tot + v)
    return np.array([np.float32(v / tot) for v in g], dtype=np.float32)


def window2d():
    w = torch.from_numpy(make_window()).double()
    return w[:, None] * w[None, :]


def k_disp_of(case):
    return float(np.float32(case["focal_x"]) * np.float32(-np.float32(case["trans_dist"])))


def alpha_weight_of(case):
    """The float32 weight image the kernel is handed (fused_loss.binocular_loss_fused forms it the same way)."""
    if case.get("gt_alpha_mask") is not None:
        return 1.0 - case["gt_alpha_mask"]
    return case.get("bg_mask")


def _ssim(x, y, w2d):
    w = w2d.to(x.dtype).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t.unsqueeze(0), w, padding=5, groups=3)[0]  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()


def _fragile(u, live=None):
    a = u.detach().abs()
    if live is not None:
        a = a * live
    top = float(a.max()) if a.numel() else 0.0
    return (a > 0) & (a < TAU * top)


def reference(case, w2d=None, lambda_smooth=None):
    """dict(parts [8], g_image, g_depth, g_alpha, g_shifted, budget {same four keys}, aux {...}); numpy float64.
    The two lambdas are the float32 values the ABI carries.  w2d / lambda_smooth: the comparison with the PyTorch statement
    hands in the statement's own window and its unrounded 0.05, so that the formulas can be held to 1e-12."""
    D = torch.float64
    H, W = case["H"], case["W"]
    hw = float(H * W)
    lam, lsm = float(np.float32(case["lambda_dssim"])), float(np.float32(case["lambda_smooth"]))
    lsm = lsm if lambda_smooth is None else float(lambda_smooth)
    image, depth, alpha = (case[k].detach().to(D).requires_grad_(True) for k in ("image", "depth", "alpha"))
    gt = case["gt"].to(D)
    shifted = None if case["shifted"] is None else case["shifted"].detach().to(D).requires_grad_(True)
    aw = alpha_weight_of(case)
    aw = None if aw is None else aw.to(D)
    z = lambda *s: torch.zeros(*s, dtype=D)  # noqa: E731
    budget = dict(g_image=z(3, H, W), g_depth=z(1, H, W), g_alpha=z(1, H, W), g_shifted=z(3, H, W))
    aux = {}

    res1 = image - gt
    Ll1 = res1.abs().mean()
    ssim = _ssim(image, gt, window2d() if w2d is None else w2d)
    budget["g_image"] += 2.0 * (1.0 - lam) / (3.0 * hw) * _fragile(res1)

    l1m, smooth = z(()), z(())
    if shifted is not None:
        k = k_disp_of(case)
        d = k / (depth + EPS)
        x0 = torch.floor(d).detach()
        cols = torch.arange(W).view(1, 1, W)
        c0 = cols + x0.long()
        c1 = c0 + 1
        valid = (c0 >= 0) & (c0 < W) & (c1 >= 0) & (c1 < W)
        w0, w1 = (x0 + 1.0) - d, d - x0
        m = torch.where(valid, w0 + w1, z(()))
        i0, i1 = c0.clamp(0, W - 1).expand(3, H, W), c1.clamp(0, W - 1).expand(3, H, W)
        s0, s1 = torch.gather(shifted, 2, i0), torch.gather(shifted, 2, i1)
        warped = torch.where(valid, w0 * s0 + w1 * s1, z(()))
        resw = warped * m - gt * m
        l1m = resw.abs().mean()
        Dp = d * m
        gs = gt.sum(0, keepdim=True)
        dd_ddepth = (d / (depth + EPS)).detach().abs()       # |d d / d depth|
        md = m.detach()
        # flip budget of the warp residual: g_shifted at both taps, g_depth at the pixel
        fr = _fragile(resw, valid) & valid                      # (an invalid pixel's residual is exactly 0 anyway)
        gmag = md / (3.0 * hw)
        budget["g_shifted"].scatter_add_(2, i0, 2.0 * w0.detach().abs() * gmag * fr)
        budget["g_shifted"].scatter_add_(2, i1, 2.0 * w1.detach().abs() * gmag * fr)
        budget["g_depth"] += (2.0 * gmag * (s1 - s0).detach().abs() * fr).sum(0, keepdim=True) * dd_ddepth
        if H > 2 and W > 2:
            ex = torch.exp((0.5 * (gs[:, 1:-1, 2:] - gs[:, 1:-1, :-2])).abs() * -0.33)
            ey = torch.exp((0.5 * (gs[:, 2:, 1:-1] - gs[:, :-2, 1:-1])).abs() * -0.33)
            vx = ex * (0.5 * (Dp[:, 1:-1, 2:] - Dp[:, 1:-1, :-2]))
            vy = ey * (0.5 * (Dp[:, 2:, 1:-1] - Dp[:, :-2, 1:-1]))
            smooth = vx.abs().mean() + vy.abs().mean()
            c_smooth = lsm / float((H - 2) * (W - 2))
            tap = md * dd_ddepth                                # |d D' / d depth| at a tap
            bx, by = 2.0 * 0.5 * ex * c_smooth * _fragile(vx), 2.0 * 0.5 * ey * c_smooth * _fragile(vy)
            bd = budget["g_depth"]
            bd[:, 1:-1, 2:] += bx * tap[:, 1:-1, 2:]
            bd[:, 1:-1, :-2] += bx * tap[:, 1:-1, :-2]
            bd[:, 2:, 1:-1] += by * tap[:, 2:, 1:-1]
            bd[:, :-2, 1:-1] += by * tap[:, :-2, 1:-1]
        has = valid & (resw.detach() != 0)                      # the kernel's `has`, per channel
        aux = dict(d=d.detach()[0].numpy(), floor=x0[0].long().numpy(), c0=c0[0].numpy(), valid=valid[0].numpy(),
                   has=has.numpy(), fragile_warp=int(fr.sum()))

    al = z(())
    if aw is not None:
        al = (alpha.abs() * aw).mean()
        budget["g_alpha"] += 2.0 * aw / hw * (_fragile(alpha, (aw != 0).to(D)) & (aw != 0))

    total = ((1.0 - lam) * Ll1 + lam * (1.0 - ssim)) + (l1m + lsm * smooth) + al
    ins = [image, depth, alpha] + ([] if shifted is None else [shifted])
    gr = list(torch.autograd.grad(total, ins, allow_unused=True)) + ([None] if shifted is None else [])
    shapes = ((3, H, W), (1, H, W), (1, H, W), (3, H, W))
    out = dict(parts=np.array([float(v.detach()) for v in (total, Ll1, ssim, l1m, smooth, al)] + [0.0, 0.0]),
               budget={k: v.numpy() for k, v in budget.items()}, aux=aux)
    for key, g, shp in zip(("g_image", "g_depth", "g_alpha", "g_shifted"), gr, shapes):
        out[key] = np.zeros(shp) if g is None else g.numpy().copy()
    return out


def statement_outputs(binocular_loss, case, dtype):
    """The package's PyTorch statement (handed in: this file imports nothing from the package) on `case` in `dtype` on the
    CPU: same keys as reference() without budget / aux.  Where the statement and the kernel deliberately differ -- its
    hard-coded 0.05 and its NaN mean over an empty interior -- the total is put together from the statement's own parts."""
    H, W = case["H"], case["W"]
    # (clones: .to() of a tensor that already has the dtype is the case's own tensor, which stays untouched)
    t = {k: case[k].detach().clone().to(dtype).requires_grad_(True) for k in ("image", "depth", "alpha")}
    sh = None if case["shifted"] is None else case["shifted"].detach().clone().to(dtype).requires_grad_(True)
    kw = dict(lambda_dssim=float(np.float32(case["lambda_dssim"])))
    if sh is not None:
        kw.update(shifted_image=sh, focal_x=float(np.float32(case["focal_x"])), trans_dist=float(np.float32(case["trans_dist"])))
    for key in ("gt_alpha_mask", "bg_mask"):
        if case.get(key) is not None:
            kw[key] = case[key].to(dtype)
            break
    total, p = binocular_loss(t["image"], t["depth"], t["alpha"], case["gt"].to(dtype), **kw)
    zero = total.new_zeros(())
    thin = H <= 2 or W <= 2
    l1m = p.get("l1_masked", zero)
    smooth = zero if (thin or sh is None) else p["smooth"]
    if sh is not None and (thin or float(np.float32(case["lambda_smooth"])) != float(np.float32(0.05))):
        total = p["loss"] + (l1m + float(np.float32(case["lambda_smooth"])) * smooth) + p["alpha_loss"]
    ins = [t["image"], t["depth"], t["alpha"]] + ([] if sh is None else [sh])
    gr = list(torch.autograd.grad(total, ins, allow_unused=True)) + ([None] if sh is None else [])
    out = dict(parts=np.array([float(v.detach()) for v in (total, p["Ll1"], p["ssim"], l1m, smooth, p["alpha_loss"])] + [0.0, 0.0]))
    for key, g, shp in zip(("g_image", "g_depth", "g_alpha", "g_shifted"), gr, ((3, H, W), (1, H, W), (1, H, W), (3, H, W))):
        out[key] = np.zeros(shp) if g is None else g.double().numpy().copy()
    return out


def deviates_from_statement(case):
    """The cases the comparison with the statement leaves out (see statement_outputs)."""
    return case["shifted"] is not None and (case["H"] <= 2 or case["W"] <= 2 or
                                             float(np.float32(case["lambda_smooth"])) != float(np.float32(0.05)))


# ------------------------------------------------------------------------------------------------------------------ inputs
def floor_fragile(depth, k, W):
    """Mask of pixels whose disparity is within FLOOR_MARGIN of an integer while a tap could be inside the image for
    either choice of the floor.  k == 0 (d exactly 0 in both precisions) and zero depth (outside for any floor) are exempt."""
    if k == 0.0:
        return torch.zeros_like(depth, dtype=torch.bool)
    d = k / (depth.double() + EPS)
    n = torch.round(d)
    cols = torch.arange(W).view(1, 1, W).double()
    could = (cols + n + 1 >= 0) & (cols + n - 1 <= W - 1)
    return ((d - n).abs() < FLOOR_MARGIN) & could & (depth != 0)


def nudge(depth, k, W):
    depth = depth.clone()
    for _ in range(64):
        bad = floor_fragile(depth, k, W)
        if not bool(bad.any()):
            return depth
        depth[bad] = depth[bad] * 1.01
    raise AssertionError("depth stays floor-fragile")


def _case(name, W, H, seed, *, shift=None, weight=None, lambda_dssim=0.2, lambda_smooth=0.05, depth_range=(2.0, 8.0)):
    """shift: None or (focal_x, trans_dist).  weight: None | 'bg' | 'gam'.  image = gt +- [0.05, 0.2]."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    gt = r(3, H, W)
    image = gt + ((r(3, H, W) > 0.5).float() * 2 - 1) * (0.05 + 0.15 * r(3, H, W))
    depth = depth_range[0] + (depth_range[1] - depth_range[0]) * r(1, H, W)
    alpha = 0.05 + 0.9 * r(1, H, W)
    shifted = r(3, H, W)
    mask = r(1, H, W)
    c = dict(name=name, W=W, H=H, image=image, gt=gt, depth=depth, alpha=alpha, shifted=shifted if shift else None,
             focal_x=shift[0] if shift else 0.0, trans_dist=shift[1] if shift else 0.0, lambda_dssim=lambda_dssim,
             lambda_smooth=lambda_smooth, bg_mask=None, gt_alpha_mask=None)
    if weight == "bg":
        c["bg_mask"] = (mask > 0.5).float()
    elif weight == "gam":
        c["gt_alpha_mask"] = torch.round(mask * 16) / 16      # 1 - mask is exact in float32
    return c


def _finish(c):
    if c["shifted"] is not None:
        c["depth"] = nudge(c["depth"], k_disp_of(c), c["W"])
    return c


def _depth_from_d(d, k):
    return (k / d.double() - EPS).float()


def _d_merge():
    """(d) k = 16; rows share floor(d) = 2 (a slow ramp), every sixth row is random instead; blocks with shifted == 0 and
    gt == 0 aligned through the warp (residual exactly 0: has == false) at the row start, in mid-run, across 15|16|17 and
    31|32, and at the end of the valid run (columns 45..47 have a tap outside)."""
    c = _case("d_merge_48x19", 48, 19, 401, shift=(64.0, -0.25), weight="bg")
    W, H = 48, 19
    rr, cc = torch.arange(H).view(H, 1).double(), torch.arange(W).view(1, W).double()
    ramp = _depth_from_d(2.15 + 0.012 * cc + 0.005 * rr, 16.0)
    rows = torch.arange(H)
    rnd = rows % 6 == 5
    c["depth"][0, ~rnd] = ramp[~rnd]
    blk = (rows % 3 != 0) & ~rnd
    for a, b in ((0, 2), (7, 10), (14, 18), (30, 33), (42, 44)):
        c["gt"][:, blk, a:b + 1] = 0.0
        c["shifted"][:, blk, a + 2:b + 4] = 0.0
    return _finish(c)


def _e_many():
    """(e) k = 16; rows 0..9: d falls by 1 per column over runs of 12 (c + floor(d) stays put: one target column collects the
    run); rows 10..18: d rises by 1 per column (c0 jumps by 2: nothing merges)."""
    c = _case("e_many_48x19", 48, 19, 402, shift=(64.0, -0.25), weight=None)
    W, H = 48, 19
    gen = torch.Generator().manual_seed(4021)
    frac = 0.3 + 0.4 * torch.rand(H, W, generator=gen, dtype=torch.float64)
    j = (torch.arange(W) % 12).view(1, W).double()
    d = torch.where(torch.arange(H).view(H, 1) < 10, 12.0 - j + frac, 1.0 + j + frac)
    c["depth"][0] = _depth_from_d(d, 16.0)
    return _finish(c)


def _f_uncov(name, focal):
    """(f) depth == 0 blocks: interior, on each border, straddling column 16."""
    c = _case(name, 40, 24, 403, shift=(focal, -0.25), weight="gam")
    for r0, r1, c0, c1 in F_BLOCKS:   # (row range, column range), half open
        c["depth"][0, r0:r1, c0:c1] = 0.0
    return _finish(c)


F_BLOCKS = ((8, 13, 22, 28), (0, 3, 5, 10), (21, 24, 30, 35), (10, 15, 0, 3), (4, 9, 37, 40), (15, 20, 14, 19))


def _seam_alias():
    """k = 35; even rows floor(d) = 1, odd rows floor(d) = 17: the left tap of (odd row, tile column 0) is the column of the
    right tap of (even row above, tile column 15) -- the lane pair a 16-wide row ends and the next one begins with."""
    c = _case("seam_alias_48x19", 48, 19, 404, shift=(140.0, -0.25), weight=None)
    W, H = 48, 19
    gen = torch.Generator().manual_seed(4041)
    frac = 0.3 + 0.4 * torch.rand(H, W, generator=gen, dtype=torch.float64)
    d = torch.where(torch.arange(H).view(H, 1) % 2 == 0, 1.0 + frac, 17.0 + frac)
    c["depth"][0] = _depth_from_d(d, 35.0)
    return _finish(c)


def _ssim_variant(name, kind):
    c = _case(name, 33, 33, 105, weight=None)
    if kind == "same":
        c["image"] = c["gt"].clone()
    elif kind == "same_l0":
        c["image"] = c["gt"].clone()
        c["lambda_dssim"] = 0.0
    elif kind == "black":
        c["image"], c["gt"] = torch.zeros(3, 33, 33), torch.zeros(3, 33, 33)
    return c


def _alpha_neg():
    c = _case("alpha_neg_bg_33x17", 33, 17, 701, weight="bg")
    c["alpha"] = c["alpha"] * ((torch.arange(33 * 17).view(1, 17, 33) % 3 != 0).float() * 2 - 1)
    return c


def _alpha_zero():
    c = _case("alpha_zero_gam_33x17", 33, 17, 702, shift=(64.0, 0.25), weight="gam")
    c["alpha"][0, ::2, ::3] = 0.0
    c["alpha"][0, 5, :] *= -1.0
    return _finish(c)


def _noshift_of(name):
    c = dict(get_case(name))
    c.update(name="noshift_48x19", shifted=None, focal_x=0.0, trans_dist=0.0)
    return c


SMALL = (2.0, -0.25)   # k = 0.5 with depth in [1, 2]: d in [0.25, 0.5]
_B = {
    "ssim_1x1": lambda n: _case(n, 1, 1, 101),
    "ssim_5x4": lambda n: _case(n, 5, 4, 102, weight="bg"),
    "ssim_11x11": lambda n: _case(n, 11, 11, 103),
    "ssim_32x32": lambda n: _case(n, 32, 32, 104, weight="gam"),
    "ssim_33x33": lambda n: _case(n, 33, 33, 105),
    "ssim_37x5": lambda n: _case(n, 37, 5, 106),
    "ssim_65x34": lambda n: _case(n, 65, 34, 107),
    "ssim_same_33x33": lambda n: _ssim_variant(n, "same"),
    "ssim_same_l0_33x33": lambda n: _ssim_variant(n, "same_l0"),
    "ssim_black_33x33": lambda n: _ssim_variant(n, "black"),
    "ssim_lam0_37x5": lambda n: _case(n, 37, 5, 106, lambda_dssim=0.0),
    "ssim_lam1_37x5": lambda n: _case(n, 37, 5, 106, lambda_dssim=1.0),
    "shift_neg_50x37": lambda n: _finish(_case(n, 50, 37, 201, shift=(64.0, -0.25), weight="gam")),
    "shift_pos_50x37": lambda n: _finish(_case(n, 50, 37, 202, shift=(64.0, 0.25), weight="bg")),
    "tzero_35x20": lambda n: _finish(_case(n, 35, 20, 203, shift=(64.0, 0.0))),
    "d_merge_48x19": lambda n: _d_merge(),
    "e_many_48x19": lambda n: _e_many(),
    "f_uncov_k4_40x24": lambda n: _f_uncov(n, 16.0),
    "f_uncov_k16_40x24": lambda n: _f_uncov(n, 64.0),
    "g_outside_20x20": lambda n: _finish(_case(n, 20, 20, 405, shift=(640.0, -0.25), depth_range=(0.95, 1.05))),
    "seam_alias_48x19": lambda n: _seam_alias(),
    "smooth_3x3": lambda n: _finish(_case(n, 3, 3, 501, shift=SMALL, depth_range=(1.0, 2.0))),
    "smooth_3x40": lambda n: _finish(_case(n, 3, 40, 502, shift=SMALL, depth_range=(1.0, 2.0), weight="gam")),
    "smooth_40x3": lambda n: _finish(_case(n, 40, 3, 503, shift=SMALL, depth_range=(1.0, 2.0))),
    "smooth_4x4": lambda n: _finish(_case(n, 4, 4, 504, shift=SMALL, depth_range=(1.0, 2.0))),
    "smooth_17x17": lambda n: _finish(_case(n, 17, 17, 505, shift=SMALL, depth_range=(1.0, 2.0))),
    "smooth_18x18": lambda n: _finish(_case(n, 18, 18, 506, shift=SMALL, depth_range=(1.0, 2.0))),
    "smooth_ls0_17x17": lambda n: _finish(_case(n, 17, 17, 505, shift=SMALL, depth_range=(1.0, 2.0), lambda_smooth=0.0)),
    "smooth_ls02_18x18": lambda n: _finish(_case(n, 18, 18, 506, shift=SMALL, depth_range=(1.0, 2.0), lambda_smooth=0.2)),
    "thin_2x9": lambda n: _finish(_case(n, 2, 9, 601, shift=SMALL, depth_range=(1.0, 2.0))),
    "thin_9x2": lambda n: _finish(_case(n, 9, 2, 602, shift=SMALL, depth_range=(1.0, 2.0), weight="bg")),
    "thin_1x1": lambda n: _finish(_case(n, 1, 1, 603, shift=SMALL, depth_range=(1.0, 2.0), weight="gam")),
    "alpha_neg_bg_33x17": lambda n: _alpha_neg(),
    "alpha_zero_gam_33x17": lambda n: _alpha_zero(),
    "b_16x16": lambda n: _finish(_case(n, 16, 16, 801, shift=(16.0, 0.25), weight="bg")),
    "noshift_48x19": lambda n: _noshift_of("d_merge_48x19"),
}
CASES = tuple(_B)
# the mixed batch: sizes 16x16, 65x34, 1x1, 33x17, 50x37, 3x40, 48x19, 20x20; no shift image in 65x34 and 33x17, no alpha
# weight in 65x34 and 20x20; the largest pair is the second
BATCH = ("b_16x16", "ssim_65x34", "thin_1x1", "alpha_neg_bg_33x17", "shift_pos_50x37", "smooth_3x40", "d_merge_48x19",
         "g_outside_20x20")
REUSE = ("d_merge_48x19", "noshift_48x19", "e_many_48x19")   # one size, one slot: with, without, another with


@functools.lru_cache(maxsize=None)
def get_case(name):
    c = _B[name](name)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """The reference of a case: computed once, shared, never written to."""
    out = reference(get_case(name))
    for k in ("parts", "g_image", "g_depth", "g_alpha", "g_shifted"):
        out[k].setflags(write=False)
    return out


def e32_of(binocular_loss, name):
    """E32 per result of a case: max |statement in float32 on the CPU - reference|; parts element-wise."""
    ref, st = ref_of(name), statement_outputs(binocular_loss, get_case(name), torch.float32)
    out = {k: float(np.abs(st[k] - ref[k]).max()) for k in ("g_image", "g_depth", "g_alpha", "g_shifted")}
    out["parts"] = np.abs(st["parts"] - ref["parts"])
    return out
