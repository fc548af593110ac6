"""CPU: the float64 yardstick of the fused loss block (tests/loss_ref.py) is itself checked here -- against the golden
fixture recorded from the reference's own Python, against the package's PyTorch statement run in float64, and for the
conditions on its inputs that the GPU test (tests/test_gpu_loss_edges.py) relies on: the share of elements with a flip
budget stays under the cap, no disparity is floor-fragile, and every constructed case constructs what it claims."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as lr  # noqa: E402
from binocular3dgs_amd import loss as stmt  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GRADS = ("g_image", "g_depth", "g_alpha", "g_shifted")


def test_window_is_the_statements_up_to_its_float32_roundings():
    # make_window() sums in index order, torch in another: the normaliser may differ by an ulp (2^-23 relative at worst),
    # each quotient is rounded on either side (2 * 2^-24), and the statement rounds the 2-D product to float32 (2^-24):
    # 2 * (2^-23 + 2 * 2^-24) + 2^-24 = 9 * 2^-24 relative at most
    w = lr.make_window()
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1.0) < 2e-7 and np.array_equal(w, w[::-1])
    mine = lr.window2d().numpy()
    theirs = stmt._gaussian_window(11, 1.5, 3, torch.zeros(1, dtype=torch.float64))[0, 0].numpy()
    assert np.all(np.abs(mine / theirs - 1.0) <= 9 * 2.0 ** -24)


def test_golden_fixture_values_and_gradients():
    g = np.load(os.path.join(GOLD, "loss_block.npz"))
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    focal_x, trans, lam = [float(x) for x in g["scalars"]]
    H, W = g["image"].shape[-2:]
    case = dict(name="golden", W=W, H=H, image=t("image"), gt=t("gt"), depth=t("depth"), alpha=t("alpha"), shifted=t("shifted"),
                focal_x=focal_x, trans_dist=trans, lambda_dssim=lam, lambda_smooth=0.05, bg_mask=None,
                gt_alpha_mask=t("gt_alpha_mask"))
    ref = lr.reference(case)
    for i, k in ((0, "total"), (1, "Ll1"), (2, "ssim"), (3, "l1_masked"), (4, "smooth"), (5, "alpha_loss")):
        np.testing.assert_allclose(ref["parts"][i], g[k], rtol=3e-5, atol=0, err_msg=k)
    assert np.array_equal(ref["aux"]["valid"], g["shift_mask"][0, 0] != 0)
    for key in GRADS:
        rec = g[key].astype(np.float64)
        over = np.abs(rec - ref[key]) - (2e-6 * np.abs(ref[key]).max() + ref["budget"][key])
        print(key, "worst excess over the bound, in units of max|ref|:", over.max() / np.abs(ref[key]).max(),
              "share with a budget:", (ref["budget"][key] > 0).mean())
        assert np.abs(ref[key]).max() > 0 and over.max() <= 0, key


@pytest.mark.parametrize("name", [n for n in lr.CASES if not lr.deviates_from_statement(lr.get_case(n))])
def test_agrees_with_the_statement_in_float64(name):
    case = lr.get_case(name)
    # (the statement multiplies focal_x and trans_dist in double: the comparison needs the float32 product to be exact)
    assert lr.k_disp_of(case) == float(np.float32(case["focal_x"])) * -float(np.float32(case["trans_dist"]))
    w2d = stmt._gaussian_window(11, 1.5, 3, torch.zeros(1, dtype=torch.float64))[0, 0]
    ref, st = lr.reference(case, w2d=w2d, lambda_smooth=0.05), lr.statement_outputs(stmt.binocular_loss, case, torch.float64)
    np.testing.assert_allclose(ref["parts"], st["parts"], rtol=1e-12, atol=1e-15)
    unit = 1.0 / (3.0 * case["H"] * case["W"])     # one pixel's weight in a mean: what every gradient here is made of
    for key in GRADS:
        assert np.abs(ref[key] - st[key]).max() <= 1e-12 * max(np.abs(st[key]).max(), unit), key


@pytest.mark.parametrize("name", lr.CASES)
def test_flip_budget_stays_under_the_cap_and_no_floor_is_fragile(name):
    case, ref = lr.get_case(name), lr.ref_of(name)
    shares = {k: float((ref["budget"][k] > 0).mean()) for k in GRADS}
    print(name, "share of elements with a budget:", shares)
    for k, v in shares.items():
        assert v <= lr.CAP, (name, k, v)
        assert np.all(np.isfinite(ref[k])) and np.all(ref["budget"][k] >= 0)
    assert np.all(np.isfinite(ref["parts"]))
    if case["shifted"] is not None:
        assert not bool(lr.floor_fragile(case["depth"], lr.k_disp_of(case), case["W"]).any())
        assert bool((case["depth"] >= 0).all())
    for k in ("image", "gt", "depth", "alpha"):
        assert case[k].dtype == torch.float32 and not case[k].requires_grad      # (inputs stay inputs: nobody marks them)
    assert max(case["W"], 0) <= 70 and case["H"] <= 50


def _aux(name):
    return lr.get_case(name), lr.ref_of(name), lr.ref_of(name)["aux"]


def test_d_merge_shares_floors_and_has_exact_zero_blocks_on_the_seams():
    case, ref, a = _aux("d_merge_48x19")
    rows = np.arange(19)
    ramp, blk = rows % 6 != 5, (rows % 3 != 0) & (rows % 6 != 5)
    assert np.all(a["floor"][ramp] == 2) and np.all(a["valid"][ramp, :45]) and not a["valid"][:, 45:].any()
    assert any(len(set(a["floor"][r])) > 2 for r in rows[~ramp])           # runs that do not share, next to those that do
    has_all, has_any = a["has"].all(0), a["has"].any(0)
    for lo, hi in ((0, 2), (7, 10), (14, 18), (30, 33), (42, 44)):
        assert not has_any[blk, lo:hi + 1].any(), (lo, hi)
        if lo > 0:
            assert has_all[blk, lo - 1].all()
        if hi < 44:
            assert has_all[blk, hi + 1].all()
    assert not has_any[blk][:, [15, 16, 17]].any() and not has_any[blk][:, [31, 32]].any()
    assert has_all[~blk & ramp][:, :45].all()                               # the same columns carry a tap on the other rows


def test_e_many_collects_a_run_on_one_column_and_merges_nothing_on_the_rising_rows():
    case, ref, a = _aux("e_many_48x19")
    has = a["has"].all(0)
    most = 0
    for r in range(10):
        tgt = a["c0"][r][has[r]]
        most = max(most, int(np.bincount(tgt, minlength=48).max()))
    assert most >= 8
    for r in range(10, 19):
        both = a["valid"][r, :-1] & a["valid"][r, 1:]
        step = (a["c0"][r, 1:] - a["c0"][r, :-1])[both]                    # (+2 inside a run, -10 where the next begins)
        assert both.sum() >= 8 and np.all(step != 1) and (step == 2).sum() >= 30


@pytest.mark.parametrize("name,below", [("f_uncov_k4_40x24", True), ("f_uncov_k16_40x24", False)])
def test_f_uncovered_blocks_sit_where_claimed(name, below):
    case, ref, a = _aux(name)
    d32 = np.float32(lr.k_disp_of(case)) / np.float32(1e-5)                 # the kernel's d on a zero-depth pixel
    assert (abs(float(d32)) < 1.0e6) == below
    zero = (case["depth"][0] == 0).numpy()
    for r0, r1, c0, c1 in lr.F_BLOCKS:
        assert zero[r0:r1, c0:c1].all()
    assert zero[:, 0].any() and zero[:, -1].any() and zero[0].any() and zero[-1].any() and zero[16, 15] and zero[16, 16]
    assert not a["valid"][zero].any() and np.all(ref["g_depth"][0][zero] == 0) and np.all(np.isfinite(ref["g_depth"]))
    assert a["valid"].any() and np.abs(ref["g_depth"]).max() > 0


def test_g_everything_is_outside():
    case, ref, a = _aux("g_outside_20x20")
    assert not a["valid"].any() and a["d"].min() > 100
    assert ref["parts"][3] == 0 and ref["parts"][4] == 0
    assert not ref["g_shifted"].any() and not ref["g_depth"].any()


def test_seam_alias_pairs_the_last_lane_of_a_row_with_the_first_of_the_next():
    case, ref, a = _aux("seam_alias_48x19")
    has = a["has"].all(0)
    n = 0
    for r in range(0, 16, 2):               # (rows r, r+1 are neighbours in one wave of a 16x16 workgroup: 4 rows per wave)
        for b in (0, 16):
            n += int(has[r, b + 15] and has[r + 1, b] and a["c0"][r + 1, b] == a["c0"][r, b + 15] + 1)
    assert n == 16


def test_trans_dist_zero_has_zero_disparity_and_only_the_last_column_invalid():
    case, ref, a = _aux("tzero_35x20")
    assert not a["d"].any() and a["valid"][:, :-1].all() and not a["valid"][:, -1].any()
    assert not ref["g_depth"].any() and ref["g_shifted"].any()


def test_small_and_thin_cases():
    for name in ("smooth_3x3", "smooth_3x40", "smooth_40x3", "smooth_4x4", "smooth_17x17", "smooth_18x18"):
        case, ref, a = _aux(name)
        assert np.all(a["floor"] == 0) and ref["parts"][4] > 0 and np.abs(ref["g_depth"]).max() > 0
    assert lr.get_case("smooth_ls0_17x17")["lambda_smooth"] == 0.0 and lr.get_case("smooth_ls02_18x18")["lambda_smooth"] == 0.2
    assert lr.ref_of("smooth_ls0_17x17")["parts"][4] == lr.ref_of("smooth_17x17")["parts"][4]
    for name in ("thin_2x9", "thin_9x2", "thin_1x1"):
        case, ref, a = _aux(name)
        assert case["shifted"] is not None and ref["parts"][4] == 0 and lr.deviates_from_statement(case)
        assert all(np.all(np.isfinite(ref[k])) for k in GRADS)
    assert lr.ref_of("thin_2x9")["aux"]["valid"][:, 0].all() and lr.ref_of("thin_2x9")["parts"][3] > 0


def test_ssim_variants_and_alpha_cases():
    same, same0, black = (lr.ref_of(n) for n in ("ssim_same_33x33", "ssim_same_l0_33x33", "ssim_black_33x33"))
    assert same["parts"][1] == 0 and abs(same["parts"][2] - 1.0) < 1e-12 and not same0["g_image"].any()
    assert black["parts"][1] == 0 and abs(black["parts"][2] - 1.0) < 1e-12 and not black["g_image"].any()
    case, ref = lr.get_case("alpha_zero_gam_33x17"), lr.ref_of("alpha_zero_gam_33x17")
    z = ((case["alpha"][0] == 0) & (lr.alpha_weight_of(case)[0] != 0)).numpy()
    assert z.sum() > 50 and not ref["g_alpha"][0][z].any() and (ref["g_alpha"] < 0).any()
    case, ref = lr.get_case("alpha_neg_bg_33x17"), lr.ref_of("alpha_neg_bg_33x17")
    assert bool(((case["alpha"] < 0) & (case["bg_mask"] != 0)).any()) and (ref["g_alpha"] < 0).any() and (ref["g_alpha"] > 0).any()
    assert not lr.ref_of("ssim_65x34")["g_alpha"].any()


def test_the_mixed_batch_is_the_one_described():
    cs = [lr.get_case(n) for n in lr.BATCH]
    assert sorted((c["W"], c["H"]) for c in cs) == sorted([(65, 34), (16, 16), (1, 1), (33, 17), (50, 37), (3, 40), (48, 19), (20, 20)])
    assert (cs[0]["W"], cs[0]["H"]) != (65, 34)
    assert sum(c["shifted"] is None for c in cs) == 2 and sum(lr.alpha_weight_of(c) is None for c in cs) == 2
    assert all(c["lambda_smooth"] == 0.05 and c["lambda_dssim"] == 0.2 for c in cs)
    assert len({(c["W"], c["H"]) for c in (lr.get_case(n) for n in lr.REUSE)}) == 1
    assert [lr.get_case(n)["shifted"] is None for n in lr.REUSE] == [False, True, False]
