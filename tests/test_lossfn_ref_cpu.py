"""CPU: the float64 yardstick of the drop-in loss functions (tests/lossfn_ref.py) is itself checked here -- against the
package's PyTorch statement run in float64, for the share of elements with a flip budget, for what each constructed case
claims to construct, and for the teeth of the bound that tests/test_gpu_lossfn_parity.py applies: mutants of the reference,
rounded to float32, must miss that bound with F at its ceiling of 16 while the float32 statement passes it.

Agreement with the statement leaves no case out.  Two are compared on changed terms, because the statement is undefined
on them as they stand: the warp cases hold disparities the kernel refuses (|d| >= 1e6, inf, NaN -- the statement casts
them to int64 and multiplies a zero gradient by inf); the statement is handed lossfn_ref.statement_disparity() instead,
which moves exactly those pixels to a finite disparity that leaves the row, and must then produce the zeros the kernel
documents.  The SSIM statement builds its window in float64 and rounds the 2-D product to float32: the reference is
handed that window for this comparison (the GPU test uses loss_ref.make_window(), the one the kernel is handed).

Mutants: every one misses the new bound at F = 16 (ratio of its error to the floor of the bound; `zeros` = it also puts a
non-zero where the reference has an exact zero).  `old` = max|a-b| / max|b| of the same mutant on the same case, which the
criterion of test_gpu_lossfn*.py allows up to 2e-4 per tensor and 3e-5 per value:
    drop_tap       ssim_64x65 g_img1 926, ssim_37x37 g_img2 894, ssim_64x65 value 113      old 1.9e-3, 1.3e-3, 7.6e-4
    swap           warp_w40 out 9e6, g_disp 1.5e7                                          old 0.90, 2.0
    clamp          warp_w3 out 1e7 + zeros, warp_w17 g_image 1.6e7 + zeros                 old 0.98, 1.6
    skip_partial   ssim_nb129_avg value 7.6e3, ssim_nb128_per value 358                    old 7.6e-3, 1.0e-3
    shared_weight  ssim_nb65_per g_img1 1.3e6                                              old 0.85
    sgn0           l1_128x128_eq g_x 1e7 + zeros, l1_3x4x17x19_full_eq g_mask 2e6 + zeros  old 1.0, 1.0
The old criterion misses NONE of them on these cases: a lost outer tap moves SSIM's variance terms, not only its means,
and costs 1e-3 of the gradient's maximum, seven times the old tolerance (it was expected below 2e-4).  What the old files
lack is the cases -- no x == y, no non-finite disparity, no 65 / 128 / 129 workgroups, no `size_average=False` above one
workgroup per plane -- and the margin: the new bound leaves a tap error a factor of 50 or more, the old one a factor of 7.
Largest share of elements with a flip budget: 0.0061 % (g_image of smooth_cap_513x512); the cap is 0.5 %.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lossfn_ref as lf  # noqa: E402
from binocular3dgs_amd import loss as _loss  # noqa: E402
from binocular3dgs_amd.gaussian_model import inverse_sigmoid  # noqa: E402

STMT = types.SimpleNamespace(l1_loss=_loss.l1_loss, ssim=_loss.ssim, smooth_loss=_loss.smooth_loss,
                             inverse_warp_images=_loss.inverse_warp_images, inverse_sigmoid=inverse_sigmoid)
# the mutants the old criterion misses: none (asserted below, so that the docstring cannot go stale)
OLD_MISSES = set()


@pytest.mark.parametrize("name", lf.CASES)
def test_agrees_with_the_statement_in_float64(name):
    case = lf.get_case(name)
    w2d = None
    if case["kind"] == "ssim":
        w2d = _loss._gaussian_window(11, 1.5, case["x"].shape[1], torch.zeros(1, dtype=torch.float64))[0, 0]
    ref, st = lf.reference(case, w2d=w2d), lf.statement(STMT, case, torch.float64)
    for k in lf.keys_of(case):
        assert ref[k].shape == st[k].shape, k
        if ref[k].size == 0:
            continue
        if case["kind"] == "ssim" and k != "value":
            unit = 1.0 / case["x"][0].numel()          # one pixel's weight in a mean: what the gradient is made of
            # (identical images: the gradient is rounding noise around zero on both sides)
            assert np.abs(ref[k] - st[k]).max() <= 1e-12 * max(np.abs(st[k]).max(), unit), k
        else:
            assert np.abs(ref[k] - st[k]).max() <= 1e-12 * np.abs(st[k]).max(), k


def test_budget_cap_on_every_case_and_tensor():
    worst = (0.0, "", "")
    for name in lf.CASES:
        ref = lf.ref_of(name)
        for k, b in ref["budget"].items():
            assert np.all(b >= 0) and np.all(np.isfinite(b)) and np.all(np.isfinite(ref[k]))
            share = float((b > 0).mean()) if b.size else 0.0
            worst = max(worst, (share, name, k))
            assert share <= lf.CAP, (name, k, share)
    print("largest share of elements with a flip budget: %.6f (%s, %s)" % worst)
    assert worst[0] > 0          # (the budget is not vacuous: the large smoothness case does hold near-ties)


def test_inputs_are_float32_and_stay_inputs():
    for name in lf.CASES:
        for k, v in lf.get_case(name).items():
            for t in (v if isinstance(v, list) else [v]):
                if isinstance(t, torch.Tensor):
                    assert not t.requires_grad and t.dtype in (torch.float32, torch.bool), (name, k)


@pytest.mark.parametrize("name,nb", [("ssim_nb1", 1), ("ssim_nb2", 2), ("ssim_nb63_per", 63), ("ssim_nb64_avg", 64), ("ssim_nb65_per", 65),
                                     ("ssim_nb129_per", 129), ("ssim_nb128_per", 128), ("ssim_37x37", 12), ("ssim_64x65", 18)])
def test_ssim_cases_launch_the_workgroup_counts_they_name(name, nb):
    case = lf.get_case(name)
    assert lf.ssim_workgroups(case) == nb
    if not case["size_average"]:
        gw = case["gw"]
        assert len(set(gw.tolist())) == case["x"].shape[0] > 1 and lf.ref_of(name)["value"].shape == (case["x"].shape[0],)


def test_ssim_contents():
    same, const, zeros = (lf.ref_of(n) for n in ("ssim_same_33x32", "ssim_const_33x32", "ssim_zeros_33x32"))
    assert abs(float(same["value"]) - 1.0) < 1e-12 and np.abs(same["g_img1"]).max() < 1e-12
    assert 0 < float(const["value"]) < 1 and np.abs(const["g_img1"]).max() > 0
    assert float(zeros["value"]) == 1.0 and not zeros["g_img1"].any() and not zeros["g_img2"].any()


@pytest.mark.parametrize("name,blocks", [("l1_1x1", 1), ("l1_1x1_chan", 1), ("l1_126x128", 63), ("l1_128x128_eq", 64),
                                         ("l1_128x128_chan_eq", 64), ("l1_1x16385", 65), ("l1_1x16385_full", 129),
                                         ("l1_cap_300x450_eq", 1583), ("l1_cap_300x450_chan", 528)])
def test_l1_cases_have_the_item_counts_they_name(name, blocks):
    case = lf.get_case(name)
    x, m = case["x"], case["mask"]
    items = x.numel() if (m is None or m.shape == x.shape) else x.numel() // x.shape[1]
    assert (items + 255) // 256 == blocks
    if name.startswith("l1_cap"):
        assert blocks > 512 and items % 256 != 0          # above the forward's cap, with a ragged tail


def test_l1_exact_paths():
    for name in lf.names("l1"):
        case, ref = lf.get_case(name), lf.ref_of(name)
        x, y, m = case["x"], case["y"], case["mask"]
        eq = (x == y).numpy()
        assert eq.any() == name.endswith("_eq")
        u = (x - y).abs()
        assert float(u[~(x == y)].min()) >= 0.049
        if eq.any():
            assert not ref["g_x"][eq].any() and not ref["g_y"][eq].any() and 0.05 < eq.mean() < 0.5
        if m is not None:
            z = (m == 0)
            assert float(m[~z].abs().min()) >= 0.25
            assert m.numel() < 100 or (bool(z.any()) and bool((m < 0).any()))
            zz = z.expand_as(x).numpy()
            assert not ref["g_x"][zz].any() and not ref["g_mask"][z.numpy()].any()
        assert not any(b.any() for b in ref["budget"].values())


def test_warp_rows_construct_what_they_claim():
    for name in lf.names("warp"):
        case, ref = lf.get_case(name), lf.ref_of(name)
        d = case["disp"]
        B, _, H, W = d.shape
        rows = {k: [h for h, r in enumerate(lf.WARP_ROWS) if r == k] for k in set(lf.WARP_ROWS)}
        c0, valid = ref["c0"][:, 0], ref["valid"][:, 0]
        # no kink: every finite disparity is an integer or at least 0.05 away from one
        fin = d[~lf.guarded(d)].double()
        frac = fin - torch.floor(fin)
        assert bool(((frac == 0) | ((frac >= 0.05 - 1e-6) & (frac <= 0.95 + 1e-6))).all())
        assert lf.FLOOR_MARGIN < 0.05
        for h in rows["edges"]:
            assert set(np.unique(c0[:, h])) <= {-1, 0, W - 2, W - 1} and bool((d[:, 0, h] != torch.floor(d[:, 0, h])).all())
            if W >= 4:
                assert set(np.unique(c0[:, h])) == {-1, 0, W - 2, W - 1}
            assert np.array_equal(valid[:, h], (c0[:, h] >= 0) & (c0[:, h] <= W - 2))
        for h in rows["ints"]:
            assert set(d[:, 0, h].unique().tolist()) <= {0.0, 1.0, -1.0, float(W - 1), float(-(W - 1))}
        for h in rows["guard"]:
            g = d[:, 0, h]
            assert not valid[:, h].any() and not ref["out"][:, :, h].any() and not ref["g_disp"][:, :, h].any()
            if W >= 6:
                assert bool(torch.isnan(g).any()) and bool(torch.isposinf(g).any()) and bool(torch.isneginf(g).any())
                assert bool((g == 1e6).any()) and bool((g == -1e6).any()) and bool((g == 999999.9375).any())
        assert float(np.float32(999999.9375)) == 999999.9375 and np.nextafter(np.float32(999999.9375), np.float32(2e6)) == np.float32(1e6)
        # guarded pixels of the `guard` row that the range test alone would ALSO refuse are the rule; only the guard keeps
        # inf / NaN from reaching the int conversion
        if W >= 17:
            h = rows["collect"][0]
            most = max(int(np.bincount(c0[b, h][valid[b, h]], minlength=W).max()) for b in range(B))
            assert most == 12
        if W == 1:
            assert not valid.any() and not ref["out"].any() and not ref["g_image"].any()
        else:
            assert valid.any() and np.abs(ref["g_image"]).max() > 0 and np.abs(ref["g_disp"]).max() > 0
        up = case["up"]
        assert bool((up == 0).any()) and bool((up > 0).any()) and bool((up < 0).any())
    assert {lf.get_case(n)["disp"].shape[-1] for n in lf.names("warp")} == {1, 2, 3, 17, 40}
    assert {lf.get_case(n)["image"].shape[0] for n in lf.names("warp")} == {1, 3}
    assert {lf.get_case(n)["image"].shape[1] for n in lf.names("warp")} == {1, 3, 5}


def test_smooth_blocks_are_exact():
    for name in ("smooth_17x33_c1", "smooth_17x33_c3", "smooth_17x33_c4"):
        case, ref = lf.get_case(name), lf.ref_of(name)
        # (arrays of the interior: index [r-1, c-1] is location (r, c))
        assert not ref["ddx"][:, :, 2:6, 3:10].any() and not ref["ddy"][:, :, 2:5, 2:12].any()       # flat disparity
        assert not ref["ax"][:, :, 8:15, 3:10].any() and not ref["ay"][:, :, 9:14, 2:12].any()        # flat image
        assert not ref["ax"][:, :, 1:15, 18:28].any() and not ref["ay"][:, :, 2:14, 17:30].any()      # channels cancel
        img = case["image"]
        if img.shape[1] > 1:
            assert bool((img[:, 0, 2:16, 19:30] != img[:, 0, 2:16, 18:29]).any())                      # (not flat there)
        # the float32 sum the kernel forms cancels exactly too: multiples of 1/256
        assert bool((img[:, :, 2:16, 18:31] * 256 == torch.round(img[:, :, 2:16, 18:31] * 256)).all())
        assert not ref["g_image"][:, :, 4:14, 20:28].any() and not ref["g_image"][:, :, 11:14, 5:10].any()
        assert np.abs(ref["g_disp"]).max() > 0 and float(ref["value"]) > 0
    case = lf.get_case("smooth_cap_513x512")
    assert (case["disp"].numel() + 255) // 256 > 1024
    assert {tuple(lf.get_case(n)["disp"].shape[-2:]) for n in lf.names("smooth")} == {(3, 3), (3, 40), (40, 3), (4, 4), (17, 33), (513, 512)}


def test_model_statement_cases():
    ex = lf.get_case("opacity_extreme")
    assert ex["o"].flatten().tolist() == [-104.0, -88.0, 17.0, 30.0, 89.0] and np.all(np.isfinite(lf.ref_of("opacity_extreme")["out"]))
    assert [lf.get_case(n)["o"].numel() for n in lf.names("opacity")[:5]] == [0, 1, 255, 256, 257]
    assert abs(float(lf.ref_of("opacity_factor1_at_17")["out"][0, 0]) - 17.0) < 1e-7
    for n in lf.names("densify"):
        case = lf.get_case(n)
        for g in lf.densify_grads(case):
            assert g.shape[1] == 2 and (g.shape[0] == 0 or g.stride(0) == case["stride"])
            assert case["stride"] == 2 or g.shape[0] <= 1 or not g.is_contiguous()
    assert {lf.get_case(n)["stride"] for n in lf.names("densify")} == {2, 3, 4}
    keep, drop = lf.ref_of("staged_keep_p257"), lf.ref_of("staged_drop_p257")
    ck, cd = lf.get_case("staged_keep_p257"), lf.get_case("staged_drop_p257")
    assert keep["flag"] == 0 and drop["flag"] == 1 and lf.ref_of("staged_keep_sticky_p257")["flag"] == 1
    assert lf.ref_of("staged_drop_p0")["flag"] == 1 and lf.ref_of("staged_keep_p0")["flag"] == 0
    assert np.array_equal(drop["accum"], cd["accum"].double().numpy()) and (keep["accum"] != ck["accum"].double().numpy()).any()
    assert bool(ck["idle"].any()) and np.all(keep["maxrad"] >= ck["maxrad"].double().numpy())


def _round32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("name", lf.CASES)
def test_the_float32_statement_passes_the_bound_with_f_1(name):
    """(By construction of E32 -- this pins that the construction, the budget and the exact-zero rule hold together.)"""
    case = lf.get_case(name)
    st = lf.statement(STMT, case, torch.float32)
    lf.check(STMT, name, {k: st[k] for k in lf.keys_of(case)}, lambda k: 1.0)


@pytest.mark.parametrize("mut,name,key", lf.MUTANTS)
def test_mutant_misses_the_bound_at_the_ceiling(mut, name, key):
    case, ref = lf.get_case(name), lf.ref_of(name)
    e32, st = lf.e32_of(STMT, name)
    got = _round32(lf.reference(case, mut=mut)[key])
    bud = None if key in lf.SCALARS else ref["budget"][key]
    rat = lf.ratio_of(key, got, ref[key], e32[key], bud)
    zeros_ok = lf.exact_zeros_hold(key, got, ref[key], st[key], bud)
    old, fig = lf.old_criterion(key, got, st[key])
    print(mut, name, key, "ratio %.3g" % rat, "exact zeros hold:", zeros_ok, "old criterion passes it:", old, "at %.3g" % fig)
    assert rat > lf.F_MAX or not zeros_ok
    assert old == ((mut, name, key) in OLD_MISSES)
    # the unmutated reference, rounded the same way, is far inside
    assert lf.ratio_of(key, _round32(ref[key]), ref[key], e32[key], bud) <= 1.0
