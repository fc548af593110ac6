"""tests/projection_ref.py (float64) against oracle/tile_ref.c (float32) on the scenes of tests/test_gpu_projection_edges.py:
the populations every stratum must hold, the float32 noise that sets the GPU bounds (helpers.PROJ_*_BOUND = 10 x the largest
99th percentile found here), the fragile set (every integer or boolean disagreement between the two lies inside it, and it
stays small), and mutations of the reference that the criteria must catch.  No GPU."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import helpers
import projection_ref
from helpers import PROJ_SH_CONFIGS, PROJ_SIZES, PROJ_STRATA
from oracle import tile_ref

CAMS = ("A", "A2", "B")
BOUNDS = dict(pos="PROJ_POS_BOUND", conic="PROJ_CONIC_BOUND", rgb="PROJ_RGB_BOUND", depth="PROJ_DEPTH_BOUND")


@functools.lru_cache(maxsize=None)
def _scene(W, H, K, deg):
    d, cams, planted = helpers.projection_scene(W, H, K, deg)
    return helpers.torch_activations(d), cams, planted


@functools.lru_cache(maxsize=None)
def _oracle(W, H, K, deg, cam):
    act, cams, _planted = _scene(W, H, K, deg)
    st = tile_ref.forward(**helpers.oracle_kwargs(helpers.with_camera(act, cams[cam])))
    return projection_ref.implementation_view(st.radii, st.rect, st.clamped, helpers.oracle_records(st))


def _reference(W, H, K, deg, cam, ref=projection_ref):
    act, cams, planted = _scene(W, H, K, deg)
    o = ref.project(**helpers.with_camera(act, cams[cam]))
    return o, helpers.projection_strata(o, planted, W, H), planted


@functools.lru_cache(maxsize=None)
def _case(W, H, K, deg, cam):
    return _reference(W, H, K, deg, cam) + (_oracle(W, H, K, deg, cam),)


ALL_CASES = [(W, H, K, deg, cam) for W, H in PROJ_SIZES for K, deg in PROJ_SH_CONFIGS for cam in CAMS]


@pytest.mark.parametrize("W,H", PROJ_SIZES)
def test_populations_and_fragility_caps(W, H):
    for K, deg in PROJ_SH_CONFIGS:
        for cam in CAMS:
            o, strata, planted, _impl = _case(W, H, K, deg, cam)
            pop = helpers.projection_populations(o, strata, planted, cam, projection_ref)
            print(f"{W}x{H} K {K} degree {deg} camera {cam}: visible {int(o['visible'].sum())}; (members, fragile) {pop}")


def test_float32_noise_of_the_oracle_pins_the_gpu_bounds():
    worst = {k: 0.0 for k in BOUNDS}
    for W, H, K, deg, cam in ALL_CASES:
        o, _strata, _planted, impl = _case(W, H, K, deg, cam)
        err, both = projection_ref.word_errors(o, impl)
        assert len(both) > 600
        line = []
        for k, e in err.items():
            p99, mx = float(np.percentile(e, 99)), float(e.max())
            worst[k] = max(worst[k], p99)
            line.append(f"{k} {p99:.1e} / {mx:.1e}")
        print(f"{W}x{H} K {K} degree {deg} camera {cam} ({len(both)} records), 99th percentile / maximum: " + "  ".join(line))
        assert np.array_equal(impl["records"][both, 5], o["opacity"][both]), "the opacity word is the input's bits"
    print("largest 99th percentiles:", {k: f"{v:.3e}" for k, v in worst.items()})
    for k, name in BOUNDS.items():          # 10 x the measurement, rounded up by less than 10 %
        assert 10 * worst[k] <= getattr(helpers, name) <= 11 * worst[k], (k, worst[k], getattr(helpers, name))


def test_every_disagreement_with_the_oracle_is_fragile_and_the_fragile_set_is_small():
    need_max, ratio_max, frag_share = {}, {}, 0.0
    for W, H, K, deg, cam in ALL_CASES:
        o, strata, _planted, impl = _case(W, H, K, deg, cam)
        dis = projection_ref.disagreements(o, impl)
        for k, v in projection_ref.needed_ulps(o, impl).items():
            if len(v):
                need_max[k] = max(need_max.get(k, 0.0), float(v.max()))
        for k, v in projection_ref.rounding_ratios(o, impl).items():
            ratio_max[k] = max(ratio_max.get(k, 0.0), float(v.max()))
        n_dec = n_frag = 0
        for k, (differs, frag, counted) in dis.items():
            bad = differs & ~frag
            assert not bad.any(), f"{W}x{H} K {K} degree {deg} camera {cam}: {k} differs outside the fragile set at {np.nonzero(bad)[0][:5]}"
            n_dec += int(counted.sum())
            n_frag += int((frag & counted).sum())
        assert n_frag <= 0.005 * n_dec, f"{W}x{H} K {K} degree {deg} camera {cam}: {n_frag} of {n_dec} decisions fragile"
        frag_share = max(frag_share, n_frag / n_dec)
    print("largest margin / (EPS32 * scale) among the disagreements, per decision:", {k: f"{v:.2f}" for k, v in need_max.items()})
    print("largest |float32 - float64| / (EPS32 * scale) of the stored quantities:", {k: f"{v:.2f}" for k, v in ratio_max.items()})
    print(f"largest share of fragile decisions in a view: {100 * frag_share:.3f} %")
    # the multiple: 4 x the largest movement a float32 evaluation shows, in the reference's own scale units (rounded up to the
    # next integer), and above every disagreement that occurred
    worst = max(list(ratio_max.values()) + list(need_max.values()))
    assert 4 * worst <= projection_ref.FRAGILE_ULPS <= 4 * worst + 1, (worst, projection_ref.FRAGILE_ULPS)


def _mutant(**knobs):
    spec = importlib.util.spec_from_file_location("projection_ref_mutant", os.path.abspath(projection_ref.__file__))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.KNOBS = dict(mod.KNOBS, **knobs)
    return mod


def _failures(W, H, K, deg, cam, ref):
    """The criteria of the GPU test, applied to oracle/tile_ref.c against `ref`: -> {stratum: failing Gaussians}"""
    o, strata, _planted = _reference(W, H, K, deg, cam, ref)
    strata = dict(strata, all=np.ones(len(o["mx"]), bool), near=np.isin(np.arange(len(o["mx"])), _planted["near"]))
    impl = _oracle(W, H, K, deg, cam)
    bad = np.zeros(len(o["mx"]), bool)
    for _k, (differs, frag, _c) in ref.disagreements(o, impl).items():
        bad |= differs & ~frag
    err, both = ref.word_errors(o, impl)
    for k, name in BOUNDS.items():
        bad[both[err[k].reshape(len(both), -1).max(1) > getattr(helpers, name)]] = True
    # the tight rect must be conservative on the oracle's own records
    ids, _tiles, reach = ref.dropped_reach(o, W, H, impl["records"])
    tight_bad = np.zeros(len(bad), bool)
    tight_bad[ids[reach >= projection_ref.ALPHA_MIN]] = True
    out = {k: int((bad & m).sum()) for k, m in strata.items()}
    out["tight"] = int(tight_bad.sum())
    out["tight_faint"] = int((tight_bad & strata["faint"]).sum())
    return out


def test_the_unmutated_reference_passes_its_own_criteria():
    for W, H, K, deg, cam in ALL_CASES:
        f = _failures(W, H, K, deg, cam, projection_ref)
        assert not any(f.values()), (W, H, K, deg, cam, {k: v for k, v in f.items() if v})


MUTANTS = {
    "near_strict": (dict(near_strict=True), ("near",), [(80, 48, 4, 1, "B")]),
    "clamp_1.2": (dict(clamp=1.2), ("clamp_x", "clamp_y", "clamp_xy"), [(80, 48, 4, 1, "A"), (33, 17, 4, 1, "A2")]),
    "sh_row_6_sign": (dict(sh6_sign=-1.0), ("all",), [(80, 48, 9, 2, "A"), (75, 33, 16, 3, "A")]),
    "upper_edge_without_15": (dict(upper_pad=0.0), ("edge_l", "edge_t", "align"), [(80, 48, 4, 1, "A"), (75, 33, 4, 1, "A")]),
    "tau2_ln": (dict(tau_factor=1.0), ("tight",), [(80, 48, 4, 1, "A"), (33, 17, 4, 1, "A")]),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_a_mutated_reference_fails_the_criteria_in_its_stratum(name):
    knobs, where, cases = MUTANTS[name]
    ref = _mutant(**knobs)
    for case in cases:
        f = _failures(*case, ref)
        print(f"{name} {case}: failing Gaussians per stratum {({k: v for k, v in f.items() if v})}")
        for s in where:
            assert f[s] > 0, f"{name} {case}: stratum {s} passes"
    if name == "sh_row_6_sign":       # rows 4.. are not read below degree 2
        assert not any(_failures(80, 48, 16, 1, "A", ref).values())
