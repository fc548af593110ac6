"""CPU: the MCMC strategy's yardstick (tests/mcmc_ref.py) against known answers and exact arithmetic, the argument checks of the
new entry points (no device is touched) and the rules between the training flags."""
import ctypes as C
import math
from decimal import Decimal, getcontext

import numpy as np
import pytest

import mcmc_ref as ref


def test_philox_known_answers():
    """Random123's known-answer vectors of philox4x32-10 (kat_vectors): zero counter and key, all ones, the digits of pi."""
    ka = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
          ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in ka:
        assert tuple(ref.philox4x32(ctr, key)) == want, [hex(x) for x in ref.philox4x32(ctr, key)]
    # the vectorised form is the same function: counter (index, offset, stream_id, 0), key = the seed's two words
    seed = 0x299f31d0a4093822
    b = ref.philox_blocks(np.array([0x243f6a88, 5]), 0x85a308d3, 0x13198a2e, seed)
    assert [int(x) for x in b[1]] == ref.philox4x32((5, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    assert [int(x) for x in b[0]] == ref.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    w = ref.random_u32(7, seed, 3, 9)
    assert [int(x) for x in w[4:7]] == ref.philox4x32((1, 9, 3, 0), (0xa4093822, 0x299f31d0))[:3]


def test_normals_of_the_yardstick_are_standard():
    z = ref.random_normal64(1 << 16, 11, 0, 4)
    n = z.shape[0]
    assert np.isfinite(z).all()
    assert abs(z.mean()) < 5 / math.sqrt(n) and abs(z.var() - 1) < 5 * math.sqrt(2 / n)
    assert abs(np.mean(z[:-1] * z[1:])) < 5 / math.sqrt(n)


def _decimal_correction(o, N):
    getcontext().prec = 50
    o = Decimal(o)
    on = 1 - (1 - o) ** (Decimal(1) / Decimal(N))
    denom = Decimal(0)
    for a in range(1, N + 1):
        for k in range(a):
            denom += Decimal(math.comb(a - 1, k)) * (-1) ** k * on ** (k + 1) / Decimal(k + 1).sqrt()
    return on, denom


@pytest.mark.parametrize("N", [2, 3, 51])
@pytest.mark.parametrize("o", [0.01, 0.5, 0.99])
def test_correction_in_float64_against_50_digits(o, N):
    """float64 in the kernel's operation order loses nothing that matters: 1e-12 relative, four decades below float32."""
    _, _, on, denom = ref.corrected(o, N, [0.0, 0.0, 0.0], 0.005)
    d_on, d_denom = _decimal_correction(o, N)
    assert abs(Decimal(on) - d_on) <= Decimal(1e-12) * d_on
    assert abs(Decimal(denom) - d_denom) <= Decimal(1e-12) * d_denom


@pytest.mark.parametrize("N", [2, 3, 7, 51])
@pytest.mark.parametrize("o", [0.01, 0.5, 0.99])
def test_correction_preserves_the_opacity_of_the_stack(o, N):
    """N copies at one place composite to 1 - (1 - o')^N: the source's opacity."""
    _, _, on, _ = ref.corrected(o, N, [0.0] * 3, 0.005)
    assert abs(1.0 - (1.0 - on) ** N - o) <= 1e-12


@pytest.mark.parametrize("o", [0.01, 0.5, 0.99])
def test_two_copies_reproduce_the_integrated_footprint(o):
    """Along a ray through the centre, a 1D Gaussian of opacity o and scale s contributes alpha(x) = o exp(-x^2 / (2 s^2)),
    whose integral is o s sqrt(2 pi).  Two coincident copies (o', s') composite to
        1 - (1 - alpha')^2 = 2 alpha' - alpha'^2,   alpha'(x) = o' exp(-x^2 / (2 s'^2)),
    and alpha'^2 = o'^2 exp(-x^2 / s'^2) is a Gaussian of scale s' / sqrt(2), so the integral is
        (2 o' s' - o'^2 s' / sqrt(2)) sqrt(2 pi).
    Equal footprints: 2 o' s' - o'^2 s' / sqrt(2) == o s.  The formula's denom at N = 2 is o' (i = 1) + o' - o'^2 / sqrt(2)
    (i = 2), and s' = s o / denom: the identity holds exactly, here to float64."""
    raw = float(np.float32(math.log(0.37)))                   # (the raw scale is a float32 word)
    s = math.exp(raw)
    raw_o, raw_s, on, denom = ref.corrected(o, 2, [raw] * 3, 0.005)
    s2 = math.exp(raw_s[0])
    assert abs(2 * on * s2 - on * on * s2 / math.sqrt(2) - o * s) <= 1e-12 * o * s
    assert abs(1 / (1 + math.exp(-raw_o)) - max(on, float(np.float32(0.005)))) <= 1e-12


def _results(mutant=None):
    out = {}
    for name, dead, draws in ref.relocation_cases(sizes=(1, 63, 64, 65, 1023, 1025)):
        rows = ref.make_rows(dead.shape[0], dead, seed=3)
        out[name] = ref.relocate_ref(rows, seed=21, offset=150, draws=draws, mutant=mutant)
    return out


def test_the_case_set_discriminates_both_mutants():
    good, ge, cnt = _results(), _results("ge"), _results("count")
    assert any(not np.array_equal(good[k]["src"], ge[k]["src"]) for k in good), "no case lands a draw on a zero-weight row"
    k = "runs_draw_ends"
    assert good[k]["dead"][ge[k]["src"][ge[k]["src"] >= 0]].any() and not good[k]["dead"][good[k]["src"][good[k]["src"] >= 0]].any()
    # N = count changes the corrected values far beyond the GPU tests' 1 ulp
    worst = max(float(np.max(np.abs(good[k]["opacity64"] - cnt[k]["opacity64"]))) for k in good)
    assert worst > 1e-2
    # both ends of the search: u = 0 takes the first alive row, u = 2^64 - 1 the last one
    alive = np.flatnonzero(~good[k]["dead"])
    taken = good[k]["src"][good[k]["dead"]]
    assert set(taken.tolist()) == {int(alive[0]), int(alive[-1])}
    # the structural cases
    assert (good["no_dead"]["src"] == -1).all() and not good["no_dead"]["written"].any()
    assert good["all_dead"]["total"] == 0 and not good["all_dead"]["written"].any()
    one = good["one_alive_200_dead"]
    assert one["count"][77] == 200 and (one["src"][one["dead"]] == 77).all()


def test_argument_errors_without_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    E = -1
    fake = 4096                                               # a non-NULL, 256-byte aligned address that is never read
    assert L.b3gs_mcmc_random(-1, 0, 0, 0, 0, fake, None) == E
    assert L.b3gs_mcmc_random((1 << 32) + 1, 0, 0, 0, 0, fake, None) == E
    assert L.b3gs_mcmc_random(4, 0, 0, 0, 2, fake, None) == E
    assert L.b3gs_mcmc_random(4, 0, 0, 0, 1, None, None) == E and b"NULL" in L.b3gs_last_error()
    assert L.b3gs_mcmc_random(0, 0, 0, 0, 0, None, None) == 0
    assert L.b3gs_mcmc_noise(-1, fake, fake, fake, fake, None, 0, 0, 1.0, 1.0, None, None) == E
    assert L.b3gs_mcmc_noise(5, fake, fake, fake, fake, None, 0, 0, float("nan"), 1.0, None, None) == E
    assert L.b3gs_mcmc_noise(5, fake, fake, fake, fake, None, 0, 0, 1.0, float("nan"), None, None) == E
    for k in range(4):
        a = [fake] * 4
        a[k] = None
        assert L.b3gs_mcmc_noise(5, *a, None, 0, 0, 1.0, 1.0, None, None) == E
    assert L.b3gs_mcmc_noise(0, None, None, None, None, None, 0, 0, 1.0, 1.0, None, None) == 0
    assert L.b3gs_mcmc_workspace_bytes(0) == 0 and L.b3gs_mcmc_workspace_bytes(-3) == 0
    assert L.b3gs_mcmc_workspace_bytes(1000) % 256 == 0 and L.b3gs_mcmc_workspace_bytes(1000) >= 1000 * 37
    v = _lib.B3gsMcmcViews()
    assert L.b3gs_mcmc_views(0, fake, C.byref(v)) == E and L.b3gs_mcmc_views(5, None, C.byref(v)) == E
    assert L.b3gs_mcmc_views(5, fake + 4, C.byref(v)) == E and L.b3gs_mcmc_views(5, fake, None) == E
    assert L.b3gs_mcmc_views(5, fake, C.byref(v)) == 0 and v.head == fake and v.src > fake

    def io(**kw):
        s = _lib.B3gsMcmcIO()
        s.P, s.P_old, s.K, s.n_max, s.min_opacity = 10, 10, 9, 51, 0.005
        for t in range(6):
            s.param[t] = fake
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    assert L.b3gs_mcmc_relocate(None, fake, None) == E
    for bad in (dict(P=-1), dict(P_old=11), dict(P_old=-1), dict(K=-1), dict(n_max=0), dict(n_max=52), dict(min_opacity=0.0),
                dict(min_opacity=1.0), dict(min_opacity=float("nan"))):
        assert L.b3gs_mcmc_relocate(C.byref(io(**bad)), fake, None) == E, bad
    for t in range(6):
        s = io()
        s.param[t] = None
        assert L.b3gs_mcmc_relocate(C.byref(s), fake, None) == E
    s = io()
    s.exp_avg[0] = fake                                       # one moment pointer of twelve
    assert L.b3gs_mcmc_relocate(C.byref(s), fake, None) == E and b"moments" in L.b3gs_last_error()
    assert L.b3gs_mcmc_relocate(C.byref(io()), None, None) == E
    assert L.b3gs_mcmc_relocate(C.byref(io()), fake + 8, None) == E
    assert L.b3gs_mcmc_relocate(C.byref(io(P=0, P_old=0)), None, None) == 0       # no rows: nothing to do


def test_python_layer_refuses_host_tensors_and_sharded_adam():
    import torch
    from binocular3dgs_amd import _lib, mcmc
    from binocular3dgs_amd.gaussian_model import GaussianModel
    rows = [torch.from_numpy(a) for a in ref.make_rows(8, np.zeros(8, dtype=bool))]
    m = GaussianModel.from_tensors(*rows, sh_degree=1)
    with pytest.raises(_lib.B3gsError, match="HIP device"):
        mcmc.inject_noise(m, 1e-4, iteration=1, seed=0)
    with pytest.raises(_lib.B3gsError, match="HIP device"):
        mcmc.relocate(m, None, iteration=1, seed=0)
    with pytest.raises(_lib.B3gsError, match="HIP device"):
        mcmc.grow(m, None, 100, iteration=1, seed=0)

    class Sharded:
        def gather_full_state(self):
            raise AssertionError("not reached")

    with pytest.raises(_lib.B3gsError, match="ShardedAdam"):
        mcmc._moments(Sharded(), m.parameters())


def test_parser_rules():
    from binocular3dgs_amd import train
    p = train.parser()
    a = p.parse_args(["-s", "x"])
    assert a.densify == "adc" and a.cap_max is None and a.noise_lr == 5e5 and a.opacity_reg == 0.01 and a.scale_reg == 0.01
    train.check_args(a)
    with pytest.raises(ValueError, match="--cap_max"):
        train.check_args(p.parse_args(["-s", "x", "--densify", "mcmc"]))
    with pytest.raises(ValueError, match="--step graph"):
        train.check_args(p.parse_args(["-s", "x", "--densify", "mcmc", "--cap_max", "1000", "--step", "graph"]))
    train.check_args(p.parse_args(["-s", "x", "--densify", "mcmc", "--cap_max", "1000"]))
    with pytest.raises(SystemExit):
        p.parse_args(["-s", "x", "--densify", "split"])
    with pytest.raises(SystemExit):
        train.main(["-s", "x", "--densify", "mcmc", "--quiet"])
