"""preprocess_fwd_kernel (csrc/preprocess.hip) at its cull, clamp and rect seams: bit-exact against oracle/tile_ref.c, against
the float64 reference tests/projection_ref.py, the tight rect from both sides, the predicted-tile flags, mark_visible.

The library is driven through its C ABI like tests/test_gpu_binning_edges.py (BinDevice: b3gs_forward_raw_batch(phases = 1)
projects and bins).  Both references run on the device's own activation bits (b3gs_debug_activations).  Tile rects are observed
through tiles_touched and through the set of tiles in whose list a Gaussian appears.  Scenes: helpers.projection_scene (P = 829,
scale modifier 0.8, cameras A / its binocular partner / the axis-aligned B; 80x48, 75x33, 33x17); which stratum a Gaussian belongs
to in a view is decided by the float64 reference, the populations are asserted (helpers.projection_populations) and printed.

Bounds (helpers.PROJ_*_BOUND) = 10 x the largest 99th percentile of oracle/tile_ref.c (float32) against projection_ref (float64)
over 3 sizes x 3 cameras x 6 SH configurations (tests/test_projection_ref_cpu.py measures and pins them; never taken from the
kernel).  |err| / (1 + |x|), the conic against the largest conic entry of its Gaussian; 99th percentile / maximum, the range
over the 54 views:
    pixel position  6.2e-7 .. 1.4e-6 / 1.3e-6 .. 6.3e-6      conic  2.2e-6 .. 3.8e-6 / 8.9e-6 .. 3.8e-5
    colour          3.3e-8 .. 1.1e-7 / 5.5e-8 .. 2.2e-7      depth  0 (camera B: exact) .. 7.7e-8 / 4.0e-8 .. 8.7e-8
  largest 99th percentiles 1.40e-6, 3.78e-6, 1.12e-7, 7.72e-8 -> bounds 1.5e-5, 4.1e-5, 1.2e-6, 8.4e-7.  (Needles longer than
  12 pixels were taken out of the scene: their float32 determinant cancels, and the ORACLE's own conic error reached 2.2e-4,
  past 10 x its 99th percentile.)
Fragile decisions: margin < projection_ref.FRAGILE_ULPS (= 4) x EPS32 x scale.  The oracle decides none of its ~330 000 integer
and boolean decisions against the float64 reference; its stored quantities move by at most 0.84 EPS32 x scale (view depth;
pixel position 0.45, colour 0.47), and 4 x that is the multiple.  Fragile: at most 0.09 % of the decisions of a view, at most
one or two members of a stratum.  A tight-rect edge is also left out of the not-loose check when it lies within the kernel's
deliberate slack (0.2 % + 0.06 px, the widest a stored extent may be) of a tile boundary.
A speck (all scales 1e-4 z) has radius ceil(3 sqrt(0.3 + sqrt(0.1))) = 3, not 2: the discriminant is floored at 0.1.

Mutations of preprocess_fwd_kernel (scratch builds of the library, never committed; this whole file run once per build, 47
cases; the unmutated build passes all 47):
  pv[2] < B3GS_NEAR                   24 fail: every single-view and batch-of-8 case with camera B (the 8 Gaussians at view z = 0.2f
                                      get a key, a radius and tiles: radius / tiles_touched / depth key / rect differ from the
                                      oracle in stratum near) and the three tight cases
  0.0039f -> 0.0040f                  3 fail, (c) at every size: the ext words of the 10 members of band (1/255, 0.0040) -- and of
                                      the 10 of [0.0039, 1/255) -- are -1e30 where the float64 extent is positive
  floorf((mx + ext_x) / T), no + 1    3 fail, (c): dropped tiles are reached, by the float64 reference and by the device's records,
                                      in every stratum that holds visible splats
  tau2 = logf(...)                    3 fail, (c): ~690 ext words below the float64 extent
  rm shifted by rx0                   2 fail, (d) 80x48 and 16x1024 (exact masks): Gaussians behind K1 missing from planted
                                      tiles; 1040x32 and 16x2064 pass by construction (all-ones masks: rm is not consulted)
  SH_C2[2] negated                    13 fail: every case of (K, degree) = (9, 2) and (16, 3) -- colour words and clamp bits against
                                      both references; degrees 0 and 1 never read row 6 and pass
  held_rect not updated for role 1    NOT RUN on the device: view 0 of a pair would then carry tiles_touched > 0 with an all-zero
                                      rect, and the instance emission divides by the rect's width -- tile ids out of range are
                                      written through.  The pair test compares view 0's rect (the tiles of its lists) with the
                                      oracle's, which such a build cannot pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import binning_ref
import helpers
import projection_ref as pr
from helpers import PROJ_SH_CONFIGS, PROJ_SIZES
from test_gpu_binning_edges import BinDevice, assert_two_rounds, bin_state, plant_pred, read_pred, reference

pytestmark = pytest.mark.gpu
BOUNDS = dict(pos=helpers.PROJ_POS_BOUND, conic=helpers.PROJ_CONIC_BOUND, rgb=helpers.PROJ_RGB_BOUND, depth=helpers.PROJ_DEPTH_BOUND)
CULLED = binning_ref.CULLED


def device_activations(dev):
    """exp / normalize / sigmoid of the raw parameters as the kernels evaluate them -> (scales, rotations, opacities) on the host"""
    s, q = torch.empty_like(dev.params[2]), torch.empty_like(dev.params[3])
    o = torch.empty(dev.P, device="cuda")
    dev.lib.check(dev.L.b3gs_debug_activations(dev.P, C.byref(dev.rp), s.data_ptr(), q.data_ptr(), o.data_ptr(), dev.stream),
                  "b3gs_debug_activations")
    torch.cuda.synchronize()
    return s.cpu(), q.cpu(), o.cpu()


_SCENES = {}


def scene(W, H, K, deg):
    """-> (Device, scene dict with the device's activations, cameras, planted); built once per configuration"""
    key = (W, H, K, deg)
    if key not in _SCENES:
        d, cams, planted = helpers.projection_scene(W, H, K, deg)
        dev = BinDevice(d, K)
        s, q, o = device_activations(dev)
        _SCENES[key] = (dev, dict(d, scales=s, rotations=q, opacities=o.reshape(-1, 1)), cams, planted)
    return _SCENES[key]


_REFS = {}


def references(key, act_view, planted, cam):
    """float64 reference, strata and populations, and oracle/tile_ref.c of one view; computed once and left unchanged"""
    if key not in _REFS:
        from oracle import tile_ref
        o = pr.project(**act_view)
        strata = helpers.projection_strata(o, planted, act_view["W"], act_view["H"])
        strata["near"] = np.isin(np.arange(len(o["mx"])), planted["near"])          # (meaningful with camera B)
        pop = helpers.projection_populations(o, strata, planted, cam, pr) if cam else None
        st = tile_ref.forward(**helpers.oracle_kwargs(act_view))
        _REFS[key] = (o, strata, pop, st)
    return _REFS[key]


def device_rects(st):
    """The rect of every Gaussian as the set of tiles whose list holds it: must be a full rectangle -> [P, 4], tiles per Gaussian"""
    gx = (st["W"] + 15) // 16
    P = len(st["radii"])
    rect, count = np.zeros((P, 4), np.int64), np.bincount(st["point_list"], minlength=P)
    order = np.argsort(st["point_list"], kind="stable")
    g_sorted, t_sorted = st["point_list"][order], st["tile_ids"][order]
    start = np.searchsorted(g_sorted, np.arange(P))
    for g in np.nonzero(count)[0]:
        t = t_sorted[start[g]:start[g] + count[g]]
        x, y = t % gx, t // gx
        rect[g] = (x.min(), y.min(), x.max() + 1, y.max() + 1)
        assert len(np.unique(t)) == len(t) == (rect[g, 2] - rect[g, 0]) * (rect[g, 3] - rect[g, 1]), f"Gaussian {g}: tiles {sorted(t)} are no rectangle"
    return rect, count


def implementation(st):
    rect, count = device_rects(st)
    assert np.array_equal(count, st["touched"]), "tiles_touched == the number of lists that hold the Gaussian"
    bits = st["records"][:, 12].copy().view(np.uint32).astype(np.int64)
    clamped = np.stack([(bits >> ch) & 1 for ch in range(3)], 1).astype(bool)
    impl = pr.implementation_view(st["radii"], rect, clamped, st["records"], near=st["keys"] != CULLED)
    impl["bits"] = bits
    return impl


def view_z_float32(act_view):
    """View z with the kernel's four float32 operations, each correctly rounded: ((m2 x + m6 y) + m10 z) + m14"""
    m, V = act_view["means3D"].numpy().astype(np.float32), act_view["viewmatrix"].numpy().astype(np.float32).reshape(16)
    return ((V[2] * m[:, 0] + V[6] * m[:, 1]) + V[10] * m[:, 2]) + V[14]


def per_stratum(mask, strata):
    return {k: int((mask & m).sum()) for k, m in strata.items() if (mask & m).any()}


def check_bit_exact(name, st, impl, tref, strata, act_view):
    """(a) against oracle/tile_ref.c on the same input bits"""
    z32 = view_z_float32(act_view)
    want_key = np.where(z32 > np.float32(0.2), z32.view(np.uint32).astype(np.int64), CULLED)
    vis = tref.radii > 0
    assert np.array_equal(tref.depths[vis].view(np.uint32), want_key[vis].astype(np.uint32)), "the oracle's depths are these bits"
    bad = {"radius": st["radii"] != tref.radii, "tiles_touched": st["touched"] != tref.tiles_touched.astype(np.int64),
           "depth key": st["keys"] != want_key, "rect": (impl["rect"] != tref.rect).any(1),
           "clamp bits": vis & (impl["bits"] != (tref.clamped * np.array([1, 2, 4])).sum(1))}
    want = helpers.oracle_records(tref)
    got = np.ascontiguousarray(st["records"][:, :10])
    for w, word in enumerate(("mx", "my", "conic xx", "conic xy", "conic yy", "opacity", "r", "g", "b", "depth")):
        bad[f"word {w} ({word})"] = vis & (got[:, w].view(np.uint32) != want[:, w].view(np.uint32))
    report = {k: (int(v.sum()), per_stratum(v, strata)) for k, v in bad.items() if v.any()}
    assert not report, f"{name}: differs from oracle/tile_ref.c bit for bit: {report}"


def check_float64(name, impl, o, strata):
    """(b) float words within the bounds, every non-fragile decision equal"""
    report = {}
    for k, (differs, frag, _c) in pr.disagreements(o, impl).items():
        v = differs & ~frag
        if v.any():
            report[k] = (int(v.sum()), per_stratum(v, strata))
    err, both = pr.word_errors(o, impl)
    for k, e in err.items():
        e = e.reshape(len(both), -1).max(1)
        print(f"{name}: {k} max error {e.max():.2e} (bound {BOUNDS[k]:.1e})")
        over = np.zeros(len(o["mx"]), bool)
        over[both[e > BOUNDS[k]]] = True
        if over.any():
            report[k] = (float(e.max()), per_stratum(over, strata))
    assert np.array_equal(impl["records"][both, 5], o["opacity"][both])
    assert not report, f"{name}: against the float64 reference: {report}"


def check_near(name, st, o, planted):
    i = planted["near"]
    z = o["pv"][i, 2]
    want = np.where(z > helpers.PROJ_NEAR_Z[0], z.astype(np.float32).view(np.uint32).astype(np.int64), CULLED)
    assert np.array_equal(st["keys"][i], want), f"{name}: near-plane keys {st['keys'][i]} against {want}"
    gone = want == CULLED
    assert (st["radii"][i][gone] == 0).all() and (st["touched"][i][gone] == 0).all() and (st["radii"][i][~gone] > 0).all()


def run_views(label, W, H, K, deg, cams_used, batch_sizes=None):
    """One launch of the named cameras (batch_sizes: (cam, W, H) views of the W x H scene at other sizes); checks (a), (b)."""
    dev, act, cams, planted = scene(W, H, K, deg)
    specs = [(c, W, H) for c in cams_used] if batch_sizes is None else batch_sizes
    ds = [helpers.with_camera(act, (cams if (w, h) == (W, H) else helpers.projection_cameras(w, h))[c]) for c, w, h in specs]
    views = dev.views(ds)
    # a partner right behind its camera borrows that view's depth order: rect roles 1 and 2
    order = [k - 1 if k and specs[k][0] == "A2" and specs[k - 1] == ("A",) + specs[k][1:] else -1 for k in range(len(specs))]
    dev.launch(views, reference_binning=1, order_from=order)
    for k, (v, d_view, (c, w, h)) in enumerate(zip(views, ds, specs)):
        st = bin_state(v)
        floors = c if (w, h) == (W, H) else None          # the scene is placed for W x H: other sizes are compared, not counted
        o, strata, pop, tref = references((W, H, K, deg, c, w, h), d_view, planted, floors)
        name = f"{label} view {k} (camera {c}, {w}x{h}, K {K} degree {deg})"
        print(f"{name}: visible {int(o['visible'].sum())} N {st['N']}; (members, fragile) {pop}")
        assert st["flag"] == 0
        impl = implementation(st)
        check_bit_exact(name, st, impl, tref, strata, d_view)
        check_float64(name, impl, o, strata)
        if c == "B":
            check_near(name, st, o, planted)


@pytest.mark.parametrize("K,deg", PROJ_SH_CONFIGS)
@pytest.mark.parametrize("W,H", PROJ_SIZES)
def test_single_views_bit_exact_and_against_float64(W, H, K, deg):
    for cam in ("A", "B"):
        run_views("single", W, H, K, deg, [cam])


@pytest.mark.parametrize("K,deg", PROJ_SH_CONFIGS)
@pytest.mark.parametrize("W,H", PROJ_SIZES)
def test_binocular_pair_as_one_batch(W, H, K, deg):
    """rect roles 1 and 2: the partner borrows the depth order, the two rects leave in one 16-byte store"""
    run_views("pair", W, H, K, deg, ["A", "A2"])


@pytest.mark.parametrize("K,deg", [(16, 3), (4, 1), (1, 0)])
def test_eight_views_of_three_sizes_in_one_launch(K, deg):
    (w0, h0), (w1, h1), (w2, h2) = PROJ_SIZES
    batch = [("A", w0, h0), ("A2", w0, h0), ("B", w1, h1), ("A", w2, h2), ("A2", w2, h2), ("A", w1, h1), ("B", w0, h0), ("B", w2, h2)]
    run_views("batch of 8", w0, h0, K, deg, None, batch)


@pytest.mark.parametrize("W,H", PROJ_SIZES)
def test_tight_rect_is_conservative_and_not_loose(W, H):
    """(c) reference_binning = 0, the product path"""
    K, deg = 4, 1
    dev, act, cams, planted = scene(W, H, K, deg)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    for cam in ("A", "A2", "B"):
        d_view = helpers.with_camera(act, cams[cam])
        (v,) = dev.views([d_view])
        dev.launch([v], reference_binning=0)
        st = bin_state(v)
        o, strata, pop, tref = references((W, H, K, deg, cam, W, H), d_view, planted, cam)
        name = f"tight {W}x{H} camera {cam}"
        impl = implementation(st)                                      # tiles_touched == area == number of lists
        rect, vis = impl["rect"], st["radii"] > 0
        assert np.array_equal(st["radii"], tref.radii), name
        full = tref.rect.astype(np.int64)
        has = st["touched"] > 0
        inside = (rect[:, 0] >= full[:, 0]) & (rect[:, 1] >= full[:, 1]) & (rect[:, 2] <= full[:, 2]) & (rect[:, 3] <= full[:, 3])
        assert inside[has].all(), f"{name}: tight rect outside the reference rect: {per_stratum(has & ~inside, strata)}"
        # ext words
        ex, ey = st["records"][:, 10].astype(np.float64), st["records"][:, 11].astype(np.float64)
        gate = o["gate"]
        assert (ex[vis & ~gate] == np.float32(-1e30)).all() and (ey[vis & ~gate] == np.float32(-1e30)).all(), name
        m = vis & gate
        for got, want, axis in ((ex, o["ext_x"], "x"), (ey, o["ext_y"], "y")):
            low, high = got[m] < want[m], got[m] > want[m] * 1.002 + 0.06
            assert not low.any() and not high.any(), f"{name}: ext_{axis} below the float64 extent at {int(low.sum())}, above 1.002 x + 0.06 at {int(high.sum())}"
        b1 = strata["faint1"] & vis
        assert (ex[b1] == np.float32(0.05)).all() and (ey[b1] == np.float32(0.05)).all(), f"{name}: band [0.0039, 1/255): tau2 = 0, ext = 0.05"
        b0 = strata["faint0"] & o["visible"]
        assert b0.sum() >= 6 and (st["radii"][b0] > 0).all() and (st["touched"][b0] == 0).all() and (tref.tiles_touched[b0] > 0).all(), \
            f"{name}: band [0.0030, 0.0039): a record, a radius, no tile under tight binning"
        assert np.array_equal(st["records"][b0][:, :10].view(np.uint32), helpers.oracle_records(tref)[b0].view(np.uint32))
        # conservative: every tile of the reference rect that the tight rect leaves out, from both sides
        dev_o = dict(o, rect=full, tight=rect, visible=vis)
        for side, records in (("float64 reference", None), ("device records", st["records"])):
            use = dict(dev_o, visible=vis & o["visible"]) if records is None else dev_o
            ids, tiles, reach = pr.dropped_reach(use, W, H, records)
            over = reach >= pr.ALPHA_MIN
            worst = f"{reach.max():.3e}" if len(reach) else "-"
            print(f"{name}: {len(ids)} dropped (Gaussian, tile) pairs, largest reach by the {side} {worst} (1/255 = {pr.ALPHA_MIN:.3e})")
            who = np.zeros(len(vis), bool)
            who[ids[over]] = True
            assert not over.any(), f"{name}: a dropped tile is reached ({side}): {per_stratum(who, strata)}, first {list(zip(ids[over][:4], tiles[over][:4].tolist()))}"
        assert len(ids) > 200, name
        # not loose: the tiles of [mx +- ext] x [my +- ext] by the float64 reference, cut to the reference rect
        both = vis & o["visible"] & (full == o["rect"]).all(1)
        empty_ref, empty_dev = pr.rect_area(o["tight"]) == 0, st["touched"] == 0
        any_frag = np.any([pr.fragile(o, e) for e in pr.TIGHT_DECISIONS], 0)
        loose = {}
        diff = both & ~any_frag & (empty_ref != empty_dev)          # no tile at all on one side only
        if diff.any():
            loose["empty"] = (int(diff.sum()), per_stratum(diff, strata))
        for k, edge in enumerate(pr.TIGHT_DECISIONS):
            ok = both & ~pr.fragile(o, edge) & ~empty_ref & ~empty_dev
            diff = ok & (rect[:, k] != o["tight"][:, k])
            if diff.any():
                loose[edge] = (int(diff.sum()), per_stratum(diff, strata))
            print(f"{name}: tight edge {edge}: {int(ok.sum())} compared, {int((both & pr.fragile(o, edge)).sum())} fragile or in the slack")
        assert not loose, f"{name}: tight rect differs from the float64 footprint: {loose}"
        n_shrunk = int((has & (pr.rect_area(rect) < pr.rect_area(full))).sum())
        print(f"{name}: N {st['N']} of {int(tref.tiles_touched.sum())}; {n_shrunk} rects shrunk; populations {pop}")
        assert n_shrunk > 100


PFLAG_GRIDS = {"80x48": (80, 48), "16x1024": (16, 1024), "1040x32": (1040, 32), "16x2064": (16, 2064)}
PFLAG_P, PFLAG_K1 = 4096 + 300, 4096


@pytest.mark.parametrize("grid", sorted(PFLAG_GRIDS))
def test_predicted_tile_flags(grid):
    """(d) pflag: exact row / column masks (80x48; 64 rows: the masks' last bit), all-ones masks (65 columns, two words per row),
    the walk in global memory (129 words > PRE_PRED_WORDS).  Two rounds need K1 = 4096 < P, so P = 4396 here."""
    W, H = PFLAG_GRIDS[grid]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    rng = np.random.RandomState(helpers.hash_name(grid) % (2 ** 31))
    rank = rng.permutation(PFLAG_P)
    tile = rng.randint(0, gx * gy, PFLAG_P)
    tile[rank >= PFLAG_K1] = (rank[rank >= PFLAG_K1] - PFLAG_K1) % (gx * gy)       # the 300 behind K1: on every tile in turn
    d = helpers.splat_scene(W, H, **helpers._bin_spec(rng, W, H, PFLAG_P, rank * 0.002 + 0.5, two=0.15, big=0.02, cull_every=0, tile=tile))
    dev = BinDevice(d)
    runs = {}
    sets = {"unplanted": None, "nothing": [], "one tile": [gx * (gy // 2) + gx // 2], "the last tile": [gx * gy - 1],
            "a full row": list(range(gx * (gy - 1), gx * gy))}
    for label, tiles in sets.items():
        (v,) = dev.views([d])
        v.cap = 200000
        if tiles is not None:
            plant_pred(v, tiles)
        dev.launch([v], key_bits=27, seg1_fraction=0.5)
        st = bin_state(v)
        assert st["flag"] == 0 and (tiles is None or read_pred(v) == sorted(tiles))
        ref = reference(st)
        assert len(ref.order) == PFLAG_P > PFLAG_K1
        want = ref.two_rounds(PFLAG_K1, tiles or [], [])
        behind = int((ref.rank >= PFLAG_K1)[np.isin(ref.tile_ids, tiles or [])].sum())
        print(f"pflag {grid} {label}: N1 {want['N1']} V {want['V']}; entries behind K1 in the planted tiles {behind}")
        assert behind > 0 or not tiles, "the planted tiles hold Gaussians behind K1"
        assert_two_rounds(f"pflag {grid} {label}", st, want, n1_only=True)
        runs[label] = st
    for k in ("point_list", "tile_ids", "ranges", "counts"):
        assert np.array_equal(np.asarray(runs["nothing"][k]), np.asarray(runs["unplanted"][k])), f"nothing planted differs from the unplanted run: {k}"


def test_mark_visible_at_the_near_plane_value_by_value():
    """(e) camera B: view z = z_world + 2^-6 without rounding; visible iff z > 0.2f"""
    from binocular3dgs_amd import _C
    W, H = PROJ_SIZES[0]
    d, cams, planted = helpers.projection_scene(W, H, 4, 1)
    b = helpers.with_camera(d, cams["B"])
    got = _C.mark_visible(b["means3D"].cuda(), b["viewmatrix"].cuda(), b["projmatrix"].cuda()).cpu().numpy().astype(bool)
    o = pr.project(**helpers.torch_activations(b))
    i = planted["near"]
    z = o["pv"][i, 2]
    for value in helpers.PROJ_NEAR_Z:
        m = z == value
        print(f"mark_visible: view z {value!r}: {int(m.sum())} Gaussians, visible {got[i][m].tolist()}")
        assert m.sum() >= 6 and (got[i][m] == (value > helpers.PROJ_NEAR_Z[0])).all()
    assert (o["s_near"][i] == 0).all()
    ok = ~pr.fragile(o, "near")
    assert np.array_equal(got[ok], o["visible_z"][ok]) and ok.sum() >= len(ok) - 2
