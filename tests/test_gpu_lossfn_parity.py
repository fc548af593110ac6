"""GPU: the drop-in loss functions (binocular3dgs_amd/csrc/lossfn.hip behind loss_utils / graphics_utils / GaussianModel)
against the float64 reference of tests/lossfn_ref.py, on that file's table of cases.

Bound, element-wise:  |got - ref64| <= F * max(E32, 1e-7 * max|ref64|) + budget      (gradients and images)
                      |got - ref64| <= F * max(E32, 1e-6 * |ref64|)                   (scalar values)
E32 = max|statement in float32 on the CPU - ref64| of that case and tensor, computed at run time; budget = the reference's
flip budget (tests/test_lossfn_ref_cpu.py holds it under 0.5 % of every tensor).  An element that is exactly zero in the
reference and in the float32 statement must be exactly zero here.

F, measured on an MI355X as the issue of this test sets it: per kind of result the largest ratio of the kernel's error to the
floor above over all cases (the case that set it in brackets), doubled and rounded up to a power of two.
    ssim     value 0.171 (ssim_nb1) -> 0.5        g_img1, g_img2 1.233 (ssim_same_33x32) -> 4
    l1       value 0.208 (l1_1x1_chan) -> 0.5     g_x, g_y 1.000 (l1_3x4x17x19_chan) -> 2     g_mask 1.000 (l1_1x16385_full) -> 2
    warp     out 0.659 -> 2     g_image 1.089 -> 4     g_disp 0.448 -> 1                      (all three: warp_w40)
    smooth   value 0.031 (smooth_17x33_c3) -> 1/16      g_disp 1.040 (smooth_17x33_c3) -> 4    g_image 1.290 (smooth_40x3) -> 4
    opacity  out 1.031 (opacity_n257) -> 4
    densify  accum 0.850 (densify_p257_s4_alt) -> 2     denom 0: counts are exact and asserted equal
    staged   accum 0.374 (staged_keep_p1) -> 1          denom, maxrad 0: sums of small integers and a maximum, asserted equal
A ratio of exactly 1.000 (l1) says the kernel rounds where the statement rounds.  Nothing comes near the ceiling of 16, no term
had to be singled out, and the kernels are unchanged.  The pattern of infinities of opacity_decay (-inf at a logit of -104,
+inf at 17 with factor 1.0, where float32's sigmoid is 1) equals the float32 statement's; the denormal sigmoid at -88 stays
finite, and 17, 30 and 89 all land on logit(0.995).
"""
import ctypes
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lossfn_ref as lf  # noqa: E402

pytestmark = pytest.mark.gpu
F_TOL = {
    ("ssim", "value"): 0.5, ("ssim", "g_img1"): 4.0, ("ssim", "g_img2"): 4.0,
    ("l1", "value"): 0.5, ("l1", "g_x"): 2.0, ("l1", "g_y"): 2.0, ("l1", "g_mask"): 2.0,
    ("warp", "out"): 2.0, ("warp", "g_image"): 4.0, ("warp", "g_disp"): 1.0,
    ("smooth", "value"): 0.0625, ("smooth", "g_disp"): 4.0, ("smooth", "g_image"): 4.0,
    ("opacity", "out"): 4.0, ("densify", "accum"): 2.0, ("densify", "denom"): 1.0,
    ("staged", "accum"): 1.0, ("staged", "denom"): 1.0, ("staged", "maxrad"): 1.0,
}
assert max(F_TOL.values()) <= lf.F_MAX
_OPT = types.SimpleNamespace(percent_dense=0.01, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                             position_lr_max_steps=30000, feature_lr=2.5e-3, opacity_lr=0.05, scaling_lr=5e-3, rotation_lr=1e-3)


@functools.lru_cache(maxsize=None)
def _stmt():
    from binocular3dgs_amd import loss
    from binocular3dgs_amd.gaussian_model import inverse_sigmoid
    return types.SimpleNamespace(l1_loss=loss.l1_loss, ssim=loss.ssim, smooth_loss=loss.smooth_loss,
                                 inverse_warp_images=loss.inverse_warp_images, inverse_sigmoid=inverse_sigmoid)


def check(name, got):
    kind = lf.get_case(name)["kind"]
    return lf.check(_stmt(), name, got, lambda k: F_TOL[(kind, k)])


def _dev(t, grad=False):
    t = t.detach().clone().cuda()
    return t.requires_grad_(True) if grad else t


def _out(t):
    return t.detach().double().cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- runners
def run_ssim(name, want="12"):
    from binocular3dgs_amd.loss_utils import ssim
    case = lf.get_case(name)
    x, y = _dev(case["x"], "1" in want), _dev(case["y"], "2" in want)
    v = ssim(x, y, size_average=case["size_average"])
    L = v if case["size_average"] else (v * case["gw"].cuda()).sum()
    L.backward()
    raw = dict(value=v.detach(), g_img1=x.grad, g_img2=y.grad)
    return {k: t for k, t in raw.items() if t is not None}


def run_l1(name):
    from binocular3dgs_amd.loss_utils import l1_loss
    case = lf.get_case(name)
    x, y = _dev(case["x"], True), _dev(case["y"], True)
    m = None if case["mask"] is None else _dev(case["mask"], True)
    v = l1_loss(x, y, mask=m)
    v.backward()
    raw = dict(value=v.detach(), g_x=x.grad, g_y=y.grad)
    if m is not None:
        raw["g_mask"] = m.grad
    return raw


def run_warp(name, want="id"):
    from binocular3dgs_amd.graphics_utils import inverse_warp_images
    case = lf.get_case(name)
    img, d = _dev(case["image"], "i" in want), _dev(case["disp"], "d" in want)
    out = inverse_warp_images(img, d)
    (out * case["up"].cuda()).sum().backward()
    raw = dict(out=out.detach(), g_image=img.grad, g_disp=d.grad)
    return {k: t for k, t in raw.items() if t is not None}


def run_smooth(name):
    from binocular3dgs_amd.loss_utils import SmoothLoss
    case = lf.get_case(name)
    disp, img = _dev(case["disp"], True), _dev(case["image"], True)
    v = SmoothLoss()(disp, img)
    v.backward()
    return dict(value=v.detach(), g_disp=disp.grad, g_image=img.grad)


def _model(P, opacity=None):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    m = GaussianModel.from_tensors(torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, 3, 3), torch.zeros(P, 3),
                                   torch.zeros(P, 4), torch.zeros(P, 1) if opacity is None else opacity, sh_degree=1, device="cuda")
    m.spatial_lr_scale = 1.0
    return m


RUN = dict(ssim=run_ssim, l1=run_l1, warp=run_warp, smooth=run_smooth)


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", lf.names("ssim"))
def test_ssim_against_the_float64_reference(name):
    both, one, two = run_ssim(name, "12"), run_ssim(name, "1"), run_ssim(name, "2")
    check(name, {k: _out(v) for k, v in both.items()})
    # a gradient for img1 only takes three maps, for img2 (or both) five: the same bits whichever inputs ask
    assert set(one) == {"value", "g_img1"} and set(two) == {"value", "g_img2"}
    assert torch.equal(one["value"], both["value"]) and torch.equal(two["value"], both["value"])
    assert torch.equal(one["g_img1"], both["g_img1"]) and torch.equal(two["g_img2"], both["g_img2"])
    if name == "ssim_zeros_33x32":
        assert float(both["value"]) == 1.0 and not both["g_img1"].any() and not both["g_img2"].any()


@pytest.mark.parametrize("name", lf.names("l1"))
def test_l1_against_the_float64_reference(name):
    got = run_l1(name)
    check(name, {k: _out(v) for k, v in got.items()})
    case = lf.get_case(name)
    eq = (case["x"] == case["y"]).cuda()
    assert not got["g_x"][eq].any() and not got["g_y"][eq].any()                 # sgn(0) = 0 where x == y
    if case["mask"] is not None:
        z = (case["mask"] == 0).cuda()
        assert not got["g_mask"][z].any() and not got["g_x"][z.expand_as(eq)].any()


@pytest.mark.parametrize("name", lf.names("warp"))
def test_warp_against_the_float64_reference(name):
    both, img_only, disp_only = run_warp(name, "id"), run_warp(name, "i"), run_warp(name, "d")
    check(name, {k: _out(v) for k, v in both.items()})
    assert set(img_only) == {"out", "g_image"} and set(disp_only) == {"out", "g_disp"}
    check(name, {k: _out(v) for k, v in img_only.items()})
    assert torch.equal(img_only["out"], both["out"]) and torch.equal(disp_only["out"], both["out"])
    assert torch.equal(disp_only["g_disp"], both["g_disp"])
    # the refused disparities (|d| >= 1e6, inf, NaN): zeros in the output and in both gradients, nothing non-finite anywhere
    bad = lf.guarded(lf.get_case(name)["disp"]).cuda()
    assert bool(bad.any()) and not both["g_disp"][bad].any() and not both["out"][bad.expand_as(both["out"])].any()
    assert bool(torch.isfinite(both["g_image"]).all())


@pytest.mark.parametrize("name", lf.names("smooth"))
def test_smooth_against_the_float64_reference(name):
    got = run_smooth(name)
    check(name, {k: _out(v) for k, v in got.items()})


@pytest.mark.parametrize("name", lf.names("opacity"))
def test_opacity_decay_against_the_float64_reference(name):
    case = lf.get_case(name)
    m = _model(case["o"].shape[0], case["o"])
    before = m._opacity._version
    m.opacity_decay(factor=case["factor"])
    assert m._opacity.shape == case["o"].shape and (m._opacity._version > before or case["o"].numel() == 0)
    check(name, dict(out=_out(m._opacity)))


@pytest.mark.parametrize("name", lf.names("densify"))
def test_add_densification_stats_against_the_float64_reference(name):
    case = lf.get_case(name)
    P = case["filter"].shape[0]
    m = _model(P)
    m.training_setup(_OPT)
    m.xyz_gradient_accum, m.denom = case["accum"].clone().cuda(), case["denom"].clone().cuda()
    filt = case["filter"].cuda()
    for buf in case["bufs"]:                                        # two calls in a row
        leaf = torch.zeros(P, 2, device="cuda", requires_grad=True)
        leaf.grad = buf.cuda()[:, :2]
        assert P == 0 or leaf.grad.stride(0) == case["stride"]
        m.add_densification_stats(leaf, filt)
    got = dict(accum=_out(m.xyz_gradient_accum), denom=_out(m.denom))
    check(name, got)
    assert np.array_equal(got["denom"], lf.ref_of(name)["denom"])                                     # counts are exact
    off = ~case["filter"].numpy()
    assert np.array_equal(got["accum"][off], case["accum"].double().numpy()[off])                     # unselected rows: untouched


@pytest.mark.parametrize("name", lf.names("staged"))
def test_apply_staged_densify_stats_raw_abi(name):
    from binocular3dgs_amd import _lib
    case, ref = lf.get_case(name), lf.ref_of(name)
    P = case["accum"].shape[0]
    t = {k: case[k].clone().cuda().contiguous() for k in ("st_accum", "st_denom", "st_maxrad", "accum", "denom", "maxrad")}
    agreed = torch.tensor([case["agreed"]], dtype=torch.int32, device="cuda")
    flag = torch.tensor([case["flag"]], dtype=torch.int32, device="cuda")
    ptr = lambda x: ctypes.c_void_p(x.data_ptr() if x.numel() else None)  # noqa: E731
    rc = _lib.lib().b3gs_apply_staged_densify_stats(P, ptr(t["st_accum"]), ptr(t["st_denom"]), ptr(t["st_maxrad"]), ptr(t["accum"]),
                                                    ptr(t["denom"]), ptr(t["maxrad"]), ptr(agreed), ptr(flag),
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "b3gs_apply_staged_densify_stats")
    torch.cuda.synchronize()
    assert int(flag) == ref["flag"] and int(agreed) == case["agreed"]
    for k in ("st_accum", "st_denom", "st_maxrad"):
        assert not t[k].any(), k                                                                      # staging zero either way
    got = {k: _out(t[k]) for k in ("accum", "denom", "maxrad")}
    check(name, got)
    assert np.array_equal(got["maxrad"], ref["maxrad"]) and np.array_equal(got["denom"], ref["denom"])   # max and counts: exact
    # nothing staged on a row (or a dropped step): the model's row is left as it was, bit for bit (-0.0 stays -0.0)
    same = case["idle"] if case["agreed"] == 0 else torch.ones(P, dtype=torch.bool)
    for k in ("accum", "denom", "maxrad"):
        assert torch.equal(t[k].cpu().view(torch.int32)[same], case[k].view(torch.int32)[same]), k


# ------------------------------------------------------------------- determinism and the self-cleaning workspace
SEQUENCE = ("ssim_nb65_avg", "ssim_nb1", "l1_128x128_eq", "smooth_3x3", "ssim_nb129_per", "l1_1x1")


def _run(name):
    return RUN[lf.get_case(name)["kind"]](name)


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_workspace_cleans_itself_across_launch_sizes_and_repeats_are_bit_identical():
    """65 workgroups, then 1, 64, 1 (two partials each), 129 with per-batch folds, 1: a counter left non-zero by one launch
    would make the next fold early (a value from stale partials) or never (`out` unwritten)."""
    alone = {}
    for name in SEQUENCE:
        torch.cuda.synchronize()
        alone[name] = _run(name)
        torch.cuda.synchronize()
        check(name, {k: _out(v) for k, v in alone[name].items()})
    rounds = [[_run(name) for name in SEQUENCE] for _ in range(2)]           # back to back, nothing waits in between
    torch.cuda.synchronize()
    for rnd in rounds:
        for name, got in zip(SEQUENCE, rnd):
            assert _same_bits(got, alone[name]), name
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = [_run(name) for name in SEQUENCE]
    side.synchronize()
    for name, got in zip(SEQUENCE, third):
        assert _same_bits(got, alone[name]), name
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ warp zero-fill
def _two_source_warp():
    """Every row has one floor: a column collects at most two sources, so the atomic sums do not depend on their order."""
    gen = torch.Generator().manual_seed(77)
    img = torch.rand(2, 3, 6, 40, generator=gen)
    d = torch.tensor([-2.0, 0.0, 3.0, -7.0, 1.0, 0.0]).view(1, 1, 6, 1) + 0.2 + 0.6 * torch.rand(2, 1, 6, 40, generator=gen)
    return img, d, torch.rand(2, 3, 6, 40, generator=gen) - 0.4


def test_warp_backward_twice_through_one_forward():
    from binocular3dgs_amd.graphics_utils import inverse_warp_images
    img0, d0, up = _two_source_warp()
    img, d = _dev(img0, True), _dev(d0, True)
    L = (inverse_warp_images(img, d) * up.cuda()).sum()
    g1 = torch.autograd.grad(L, [img, d], retain_graph=True)
    g2 = torch.autograd.grad(L, [img, d], retain_graph=True)
    g3 = torch.autograd.grad(L, [img])
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1]) and torch.equal(g1[0], g3[0])
    assert g1[0].data_ptr() != g2[0].data_ptr() and bool(g1[0].any())
    # the case with twelve sources on one column: each of the two backwards is within the bound by itself
    name = "warp_w40"
    case = lf.get_case(name)
    img, d = _dev(case["image"], True), _dev(case["disp"], True)
    L = (inverse_warp_images(img, d) * case["up"].cuda()).sum()
    for k in range(2):
        gi, gd = torch.autograd.grad(L, [img, d], retain_graph=True)
        check(name, dict(g_image=_out(gi), g_disp=_out(gd)))


def test_warp_forward_under_no_grad_then_a_differentiated_one():
    from binocular3dgs_amd.graphics_utils import inverse_warp_images
    img0, d0, up = _two_source_warp()
    img, d = _dev(img0, True), _dev(d0, True)
    L = (inverse_warp_images(img, d) * up.cuda()).sum()
    want = torch.autograd.grad(L, [img, d])
    img, d = _dev(img0, True), _dev(d0, True)
    with torch.no_grad():
        plain = inverse_warp_images(img, d)
    assert not plain.requires_grad
    out = inverse_warp_images(img, d)
    assert torch.equal(out, plain)
    got = torch.autograd.grad((out * up.cuda()).sum(), [img, d])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    name = "warp_w40_b3c5"
    case = lf.get_case(name)
    img, d = _dev(case["image"], True), _dev(case["disp"], True)
    with torch.no_grad():
        inverse_warp_images(img, d)
    out = inverse_warp_images(img, d)
    (out * case["up"].cuda()).sum().backward()
    check(name, dict(out=_out(out), g_image=_out(img.grad), g_disp=_out(d.grad)))
