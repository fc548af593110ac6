"""Merging Gaussians on the device (csrc/lod.hip, binocular3dgs_amd/lod.py) against the restatement of tests/lod_ref.py: the six
outputs, cluster_of, members and the totals are compared bit for bit on every case of lod_ref.cases()."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lod_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
CASES = lr.cases()
_WANT = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _inputs(arrs):
    pos, sc, quat, alpha, dc, rest = arrs
    P = pos.shape[0]
    return [_dev(pos), _dev(sc), _dev(quat), _dev(alpha), _dev(dc.reshape(P, 1, 3)), _dev(rest.reshape(P, rest.shape[1] // 3, 3))]


def _want(name):
    if name not in _WANT:                                  # computed once, shared, left unchanged
        arrs, cell, w = CASES[name]
        _WANT[name] = lr.merge(*arrs, cell, w)
    return _WANT[name]


def _run(arrs, cell, w):
    from binocular3dgs_amd import lod
    ins = _inputs(arrs)
    before = [t.clone() for t in ins]
    out = lod.merge_activated(*ins, cell, None if w is None else _dev(w))
    assert all(torch.equal(a, b) for a, b in zip(ins, before))              # the inputs are untouched
    got = {k: v.detach().cpu().numpy() for k, v in zip(lr.OUTPUTS, out[:8])}
    rows = got["positions"].shape[0]
    got["features_dc"] = got["features_dc"].reshape(rows, 3)
    got["features_rest"] = got["features_rest"].reshape(rows, arrs[5].shape[1])
    return got, out[8]


@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_the_restatement_bit_for_bit(name):
    arrs, cell, w = CASES[name]
    want = _want(name)
    got, totals = _run(arrs, cell, w)
    t = want["totals"]
    assert (totals["clusters"], totals["pass_through"], totals["merged_members"], totals["nonfinite_rows"], totals["over_range_rows"]) == \
        (t["clusters"], t["pass"], t["merged"], 0, 0)
    for k in lr.OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, int((got[k] != want[k]).sum()))


def test_the_cases_are_what_they_claim():
    assert (_want("singletons")["members"] == 1).all()
    assert _want("one_cell")["members"].tolist() == [2000]
    m = _want("straddle")["members"]
    ends = np.cumsum(m)
    assert all(((ends - m < b) & (ends > b)).any() for b in (256, 512, 4096))   # a cluster across each of these sorted positions
    assert _want("pass_through")["totals"]["pass"] == 53
    assert _want("identical")["opacities"][0] == F(0.99) and _want("collinear_flat")["scales"][0][2] == F(1e-6)


def test_two_calls_give_identical_bits():
    arrs, cell, w = CASES["straddle"]
    a, _ = _run(arrs, cell, w)
    b, _ = _run(arrs, cell, w)
    assert lr.same_bits(a, b)


def test_errors_are_reported_with_their_count():
    from binocular3dgs_amd import lod
    from binocular3dgs_amd._lib import B3gsError
    arrs, cell, _ = CASES["P65_deg1"]
    pos, sc = arrs[0].copy(), arrs[1].copy()
    pos[7, 1] = np.nan
    sc[9, 0] = np.inf
    sc[7, 2] = np.inf                                      # two values in one row: the row is counted once
    with pytest.raises(B3gsError, match="2 rows hold a value that is not finite"):
        lod.merge_activated(*_inputs((pos, sc) + tuple(arrs[2:])), cell)
    rest = arrs[5].copy()
    rest[64, 8] = -np.inf
    with pytest.raises(B3gsError, match="1 rows hold a value that is not finite"):
        lod.merge_activated(*_inputs(tuple(arrs[:5]) + (rest,)), cell)
    fine = 4.0 / 1100.0
    n = lr.merge(*arrs, fine)["totals"]["over"]
    assert n > 0
    with pytest.raises(B3gsError, match=f"{n} rows lie beyond the 1024 cells of an axis.*smallest admissible cell"):
        lod.merge_activated(*_inputs(arrs), fine)
    torch.cuda.synchronize()
    got, _ = _run(arrs, cell, None)                        # and the next call is as good as ever
    assert lr.same_bits(got, _want("P65_deg1"))


def test_host_tensors_and_wrong_shapes_are_refused_without_a_launch():
    from binocular3dgs_amd import _C
    from binocular3dgs_amd._lib import B3gsError
    arrs, cell, _ = CASES["P65_deg1"]
    ins = _inputs(arrs)
    for k in range(6):
        bad = list(ins)
        bad[k] = bad[k].cpu()
        with pytest.raises(B3gsError, match="is on cpu"):
            _C.gaussian_merge_count(*bad, None, cell)
    with pytest.raises(B3gsError, match="is on cpu"):
        _C.gaussian_merge_count(*ins, torch.ones(65, dtype=torch.float64), cell)
    for k, shape in ((0, (65, 2)), (1, (64, 3)), (2, (65, 3)), (3, (64,)), (4, (65, 2, 3)), (5, (65, 4, 3)), (5, (65, 9))):
        bad = list(ins)
        bad[k] = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError):
            _C.gaussian_merge_count(*bad, None, cell)
    with pytest.raises(ValueError):
        _C.gaussian_merge_count(*ins, torch.ones(64, dtype=torch.float64, device=DEV), cell)
    with pytest.raises(ValueError):
        _C.gaussian_merge_count(*ins, torch.ones(65, device=DEV), cell)            # float32 weights
    with pytest.raises(ValueError):
        _C.gaussian_merge_count(ins[0].double(), *ins[1:], None, cell)
    for c in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _C.gaussian_merge_count(*ins, None, c)
    ws, totals = _C.gaussian_merge_count(*ins, None, cell)
    with pytest.raises(ValueError):
        _C.gaussian_merge_emit(*ins, None, cell, ws[:1024], totals.tolist()[:5])
    with pytest.raises(ValueError):
        _C.gaussian_merge_emit(*ins, None, cell, ws, [66, 0, 0, 0, 0])


# ---- the model level -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from binocular3dgs_amd import synth
    return synth.synth_model(2000, seed=31, width=64, height=48, K=4, device=DEV, requires_grad=False, scale_mult=3.0)


def _singleton_cell(m):
    from binocular3dgs_amd.mesh_tools import smallest_cell
    xyz = m.get_xyz
    return smallest_cell(float((xyz.amax(0) - xyz.amin(0)).max()))


def _params(m):
    return [p.detach() for p in (m._xyz, m._features_dc, m._features_rest, m._scaling, m._rotation, m._opacity)]


def test_coarsen_of_its_own_singleton_output_is_the_identity_up_to_row_order():
    from binocular3dgs_amd import lod
    from binocular3dgs_amd.gaussian_model import GaussianModel
    arrs, cell, _ = CASES["singletons"]
    ins = _inputs(arrs)
    m = GaussianModel.from_tensors(ins[0], ins[4], ins[5], torch.log(ins[1]), ins[2], torch.log(ins[3] / (1 - ins[3])).reshape(-1, 1),
                                   sh_degree=1, requires_grad=False)
    a, cluster_of, members = lod.coarsen(m, cell)
    assert (members == 1).all() and a._xyz.shape[0] == 2000 and a.max_sh_degree == 1 and a.active_sh_degree == m.active_sh_degree
    assert a.optimizer is None and not a._xyz.requires_grad
    for p, q in zip(_params(m), _params(a)):
        assert torch.equal(q[cluster_of.long()], p)                             # a permutation of the raw rows, bit for bit
    b, again, members = lod.coarsen(a, cell)
    assert (members == 1).all()
    assert torch.equal(again, torch.arange(2000, dtype=torch.int32, device=DEV))   # sorted already: the identity
    for p, q in zip(_params(a), _params(b)):
        assert torch.equal(p, q)


def test_coarsen_to_and_build_levels(model):
    from binocular3dgs_amd import lod
    P = model._xyz.shape[0]
    w = torch.rand(P, dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    for target in (1500, 300, 1):
        m, cluster_of, members, cell = lod.coarsen_to(model, target, w)
        n = m._xyz.shape[0]
        assert 1 <= n <= target and members.sum() == P and cluster_of.shape[0] == P and cell > 0
    levels, cells = lod.build_levels(model, (0.5, 0.25, 0.125), w, return_cells=True)
    counts = [l._xyz.shape[0] for l in levels]
    assert counts[0] <= 1000 and counts[1] <= 500 and counts[2] <= 250 and counts == sorted(counts, reverse=True) and min(counts) >= 1
    assert cells == sorted(cells)
    m, cluster_of, members = lod.coarsen(model, cells[1], w)
    s = lod.level_stats(model, m, members)
    assert s["P_before"] == P and s["P_after"] == counts[1] and 0.0 < s["merged_share"] <= 1.0 and s["mass_before"] > 0 and s["mass_after"] > 0
    with pytest.raises(ValueError):
        lod.coarsen_to(model, 0)


def test_renders_of_a_singleton_level_and_of_a_coarse_level(model):
    """At the singleton cell only the row order differs: the renders agree within the project's colour tolerance against the
    oracle, 2e-5 (1 + |x|).  A genuinely coarsened level renders finite pixels everywhere."""
    from binocular3dgs_amd import lod, synth
    from binocular3dgs_amd.evaluate import render_views
    cams = [c.to(DEV) for c in synth.synth_cameras(64, 48, yaws=(0.0, 4.0))]
    bg = torch.zeros(3, device=DEV)
    same, _, members = lod.coarsen(model, _singleton_cell(model))
    want = [x.clone() for x in render_views(model, cams, bg)]
    if bool((members == 1).all()):
        got = render_views(same, cams, bg)
        for g, x in zip(got, want):
            err = float(((g - x).abs() / (1 + x.abs())).max())
            print(f"singleton level: max |dC| / (1 + |C|) = {err:.3e}")
            assert err <= 2e-5
    else:
        pytest.fail("the smallest admissible cell still merges Gaussians of the synthetic model")
    coarse, _, members = lod.coarsen(model, 0.25 * float((model.get_xyz.amax(0) - model.get_xyz.amin(0)).max()))
    assert coarse._xyz.shape[0] < 1000 and int(members.max()) >= 2
    for g in render_views(coarse, cams, bg):
        assert bool(torch.isfinite(g).all())


def test_command_line_writes_the_levels(model, tmp_path):
    """lod.main on a model folder with uniform weights: one PLY and lod.json per ratio, counts within the targets, --model_out
    a folder that loads again."""
    import json
    from binocular3dgs_amd import lod
    from binocular3dgs_amd.gaussian_model import GaussianModel
    root, new = str(tmp_path / "model"), str(tmp_path / "new")
    os.makedirs(os.path.join(root, "point_cloud", "iteration_7"))
    with open(os.path.join(root, "cfg_args"), "w") as fp:
        fp.write("Namespace(sh_degree=1)")
    model.save_ply(os.path.join(root, "point_cloud", "iteration_7", "point_cloud.ply"))
    assert lod.main(["-m", root, "--uniform", "--ratios", "0.5", "0.125", "--model_out", new]) == 0
    counts = []
    for k, target in ((1, 1000), (2, 250)):
        d = os.path.join(root, "point_cloud", f"iteration_7_lod{k}")
        with open(os.path.join(d, "lod.json")) as fp:
            info = json.load(fp)
        m = GaussianModel(1)
        m.load_ply(os.path.join(d, "point_cloud.ply"))
        assert info["P_before"] == 2000 and 1 <= info["P_after"] == m._xyz.shape[0] <= target and info["cell"] > 0
        assert info["mass_before"] > 0 and info["mass_after"] > 0 and 0.0 < info["merged_share"] <= 1.0
        counts.append(m._xyz.shape[0])
    assert counts[1] <= counts[0]
    m = GaussianModel(1)
    m.load_ply(os.path.join(new, "point_cloud", "iteration_7", "point_cloud.ply"))
    assert m._xyz.shape[0] == counts[1] and os.path.exists(os.path.join(new, "cfg_args"))
