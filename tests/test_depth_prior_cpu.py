"""CPU: the depth-prior yardstick (tests/depth_prior_ref.py) against torch.autograd on the definition, its invariances, the
shared inputs' properties, the resize yardstick, the rules between the training flags and the loader's errors."""
import argparse
import os

import numpy as np
import pytest
import torch

import depth_prior_ref as ref

KW = dict(w_global=0.7, w_local=1.3, min_valid=ref.MIN_VALID, alpha_min=ref.ALPHA_MIN)


def _run(name, mode, mutant=None, **over):
    W, H, p, off = ref.CASES[name]
    d, a, pr, m, _ = ref.make_case(W, H, p, off)
    kw = dict(KW, mode=mode, patch=p, offset=off)
    kw.update(over)
    return ref.loss(d, a, pr, m, mutant=mutant, **kw), (d, a, pr, m), kw


def _autograd(planes, kw):
    d, a, pr, m = planes
    t = torch.tensor(d, dtype=torch.float64, requires_grad=True)
    L, rho = ref.torch_loss(t, torch.tensor(a, dtype=torch.float64), torch.tensor(pr, dtype=torch.float64), torch.tensor(m), **kw)
    L.backward()
    return float(L), float(rho), t.grad[0].numpy()


@pytest.mark.parametrize("mode", ["depth", "disparity"])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_yardstick_gradient_against_autograd(name, mode):
    """bound: 2^-20 of the plane's largest magnitude (float32 rounding of the output, with margin)"""
    got, planes, kw = _run(name, mode)
    L, rho, grad = _autograd(planes, kw)
    bound = 2.0 ** -20 * np.abs(grad).max()
    err = np.abs(got["grad"].astype(np.float64) - grad).max()
    print(f"{name} {mode}: L {got['parts'][0]:.12f} / {L:.12f}, max |dgrad| {err:.3e}, bound {bound:.3e}")
    assert np.abs(grad).max() > 0 and err <= bound
    assert abs(got["parts"][0] - L) <= 1e-9 and abs(got["parts"][5] - rho) <= 1e-9


@pytest.mark.parametrize("name", list(ref.CASES))
def test_shared_inputs_have_the_properties_the_device_test_relies_on(name):
    W, H, p, off = ref.CASES[name]
    d, a, pr, m, (const, low_alpha, masked) = ref.make_case(W, H, p, off)
    kw = dict(KW, mode="depth", patch=p, offset=off)
    got = ref.loss(d, a, pr, m, **kw)
    open_alpha = ref.loss(d, a, pr, m, **dict(kw, alpha_min=0.0))
    flags, sums = got["patch_flags"], got["patch_sums"]
    real = np.unique(ref.patch_ids(W, H, p, off))
    assert flags[masked] == 0 and sums[masked][0] < ref.MIN_VALID                      # skipped for n < min_valid
    n, sy, syy = sums[const][0], sums[const][2], sums[const][4]
    assert flags[const] == 0 and n >= ref.MIN_VALID and syy - (sy * sy) / n == 0.0       # skipped for Syy = 0
    assert flags[low_alpha] == 0 and open_alpha["patch_flags"][low_alpha] == 1           # skipped by alpha_min
    assert flags[real].sum() > len(real) / 2 and flags.sum() == flags[real].sum() == got["parts"][4]
    assert got["parts"][1] > 0 and got["parts"][3] >= ref.MIN_VALID and got["parts"][5] != 0   # the image is not skipped


def test_rho_is_invariant_to_scale_and_shift_of_the_prior():
    W, H, p, off = ref.CASES["70x37_o5_9"]
    d, a, pr, m, _ = ref.make_case(W, H, p, off)
    kw = dict(KW, mode="depth", patch=p, offset=off)
    one, two = ref.loss(d, a, pr, m, **kw), ref.loss(d, a, 3 * pr + 7, m, **kw)
    assert abs(one["parts"][5] - two["parts"][5]) <= 1e-6 and abs(one["parts"][2] - two["parts"][2]) <= 1e-6
    assert np.array_equal(one["patch_flags"], two["patch_flags"])
    # the fit follows: D ~ a P + b = (a / 3) (3 P + 7) + (b - 7 a / 3)
    assert abs(two["parts"][6] - one["parts"][6] / 3) <= 1e-6 and abs(two["parts"][7] - (one["parts"][7] - 7 * one["parts"][6] / 3)) <= 1e-5


def test_an_image_that_is_skipped_has_no_loss_and_no_gradient():
    got, _, _ = _run("70x37_o0_0", "depth", min_valid=70 * 37 + 1)
    assert got["parts"][0] == 0 and not got["grad"].any() and got["parts"][4] == 0


@pytest.mark.parametrize("mutant", ["origin", "drop_rho"])
def test_mutants_are_caught(mutant):
    good, planes, kw = _run("70x37_o5_9", "depth")
    bad, _, _ = _run("70x37_o5_9", "depth", mutant=mutant)
    _, _, grad = _autograd(planes, kw)
    bound = 2.0 ** -20 * np.abs(grad).max()
    assert np.abs(good["grad"] - grad).max() <= bound < np.abs(bad["grad"] - grad).max()


def test_resize_yardstick():
    rng = np.random.default_rng(1)
    src = (1 + rng.random((37, 70))).astype(np.float32)
    src[5:9, 10:20] = np.nan
    src[20, 3] = -1.0
    p, m = ref.resize(src, 70, 37)
    bad = ~(np.isfinite(src) & (src > 0))
    assert np.array_equal(m == 0, bad) and np.array_equal(p[~bad].view(np.uint32), src[~bad].view(np.uint32)) and not p[bad].any()
    up, mu = ref.resize(src[:11, :23], 70, 37)
    assert up.shape == (37, 70) and mu.any() and (mu == 0).any() and up[mu == 1].min() >= 1 and up[mu == 1].max() <= 2
    # fma32 rounds once: a product whose float64 sum with c lands exactly on a float32 tie
    a, b, c = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    assert ref.fma32(a, b, c) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23) and ref.fma32(a, b, -c) == np.float32(1 + 2.0 ** -11)


def _args(**kw):
    from binocular3dgs_amd.train import parser
    args = parser().parse_args(["-s", "src", "-m", "out"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_check_args_rules():
    from binocular3dgs_amd.train import check_args
    check_args(_args())
    check_args(_args(depth_priors="priors", depth_prior_weight=0.05))
    check_args(_args(depth_priors="priors", depth_prior_local=0.05, depth_prior_patch=64))
    with pytest.raises(ValueError, match="--depth_priors"):
        check_args(_args(depth_prior_weight=0.05))
    with pytest.raises(ValueError, match="--depth_priors"):
        check_args(_args(depth_prior_local=0.05, depth_prior_patch=64))
    with pytest.raises(ValueError, match="depth_prior_patch"):
        check_args(_args(depth_priors="priors", depth_prior_local=0.05, depth_prior_patch=4))
    check_args(_args(depth_priors="priors", depth_prior_weight=0.05, step="graph"))


def test_load_priors_names_the_missing_file(tmp_path):
    from binocular3dgs_amd.depth_prior import load_priors
    cams = [argparse.Namespace(image_name="view_a", image_width=8, image_height=6), argparse.Namespace(image_name="view_b", image_width=8, image_height=6)]
    np.save(tmp_path / "view_a.npy", np.ones((6, 8), np.float32))
    with pytest.raises(FileNotFoundError, match="view_b.npy"):
        load_priors(str(tmp_path), cams, device="cpu")
    np.save(tmp_path / "view_b.npy", np.ones((6, 8), np.int32))
    with pytest.raises(ValueError, match="view_b.npy"):
        load_priors(str(tmp_path), cams, device="cpu")


def test_mixed_prior_set_is_refused():
    from binocular3dgs_amd._lib import B3gsError
    from binocular3dgs_amd.depth_prior import check_prior_set
    with_p, without = argparse.Namespace(depth_prior=torch.zeros(1), image_name="a"), argparse.Namespace(depth_prior=None, image_name="b")
    assert check_prior_set([with_p, with_p]) and not check_prior_set([without])
    with pytest.raises(B3gsError, match="all or none"):
        check_prior_set([with_p, without])
