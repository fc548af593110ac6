"""The binning kernels of csrc/binning.hip against tests/binning_ref.py, list for list, at their radix, scan and round seams.

The library is driven through its C ABI like tests/test_gpu_blend_edges.py (its Device and _View): b3gs_forward_raw_batch(phases
= 1) projects and bins.  The reference runs on the device's own depth keys and on rects recomputed in float32 from the device's
records and radii; binning_ref.guard_rects ties them to the device (area == tiles_touched for every Gaussian -- it holds
exactly on every scene here, so b3gs_debug_views was NOT extended).  Every comparison is exact: point_list, tile_ids, ranges,
the header words N1, V, N2 and the device-side N word.  Scenes: helpers.binning_scene; what each holds is
asserted from the device state before anything is compared.

Populations measured on the device (single view, reference rects; P / N / V / culled / tied keys):
  seam: 1/1/1/0/0  63/91/60/3/0  64/66/61/3/0  65/79/62/3/0  2047/2584/1945/102/0  2048/2554/1945/103/0  2049/2716/1946/103/0
    4095/5088/3890/205/0  4096/5114/3891/205/0  4097/4836/3892/205/0  8193/10301/7783/410/2  16384/20161/15565/819/4
    16385/20166/15566/819/6  32769/40176/31130/1639/29
  ties (P 4097 | 8193; N, distinct keys, ties): one 4962, 1, 3891 | 10284, 1, 7782; three 5156, 3, 3889 | 9995, 3, 7780;
    low 9 bits 5234, 511, 3381 | 10122, 512, 7271; bits 18-26 5107, 510, 3382 | 10031, 512, 7271
  span: N 326 V 300, keys KEY27_BASE + 1 .. KEY27_BASE + 2^27 - 3; count<N>: N as named, V = N - 5, five two-tile Gaussians
  cover: N 798 V 600, the two 100-tile Gaussians at depth ranks 255 and 256; sparse: N 1325 V 1000 of P 5000
  onetile: N 8550 in tile 5; tiles256 / 257 / 257 (grid_x 1) / 513 / 1: N 515 / 517 / 517 / 1029 / 40, every tile occupied
  batch of 8: N per view 6095, 8031, 0, 7123, 2989, 6373, 0, 11012; shared orders: N 9995 (donor) 10219 (partner) 14876 (third)
  adopted: N 9996 V 7783 ties 7779; capacity: N 4097 at capacities 4097, 4096, 1365
  packed flip: P 65537 at 2912 x 2896 (32942 tiles): packed_idx_bits -1, N 71481, 29162 distinct tiles; P 65536: 16, N 71587
  two rounds (P 4608 / 8492, K1 4096 / 8192, both views): N1 708 V 648 N2 202 of N 920 V 840; tile 9 terminated (segment 1 alone),
    segment 2 in tiles 0-5, 7, 8, which are also the tiles the forward predicts open.  In a two-round forward header word 1 (V)
    counts the Gaussians the first round gathered: rank < K1 with a tile, and those behind K1 that reach a predicted tile.
  adopting pair (planted predictions 0, 3, 5 | 1, 3, 8): N1 838 V 778 | N1 818 V 758, against N1 708 V 648 with nothing predicted
Mutations (scratch builds, never committed; run through phases = 1 cases only): a second 9-bit pass with shift 8 fails 34 cases
(every seam size from 63 on, the key span, the instance counts, cover, sparse, digit skew, the batch of 8, the packed flip); equal
digits of a 64-lane row ranked in descending lane order in radix_scatter fails 57 of 58 (all but P = 1); adopted order words that
keep the donor's flag bits fail both cases of test_adopted_order_carries_this_pairs_predicted_tiles at view 0 (counts
[708, 648, 0] against N1 838 V 778: the Gaussians behind K1 are missing from the predicted tiles) and change nothing in a
one-round forward.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binning_ref
import helpers
from binning_ref import KEY27_BASE, KEY27_SPAN
from test_gpu_blend_edges import CAPACITY, Device

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class BinDevice(Device):
    """Device with every field of B3gsForwardView the binning reads."""

    def launch(self, views, phases=1, cap=CAPACITY, reference_binning=1, key_bits=0, seg1_fraction=0.0, order_from=None,
               hint=None, trusted=0):
        arr = self._fwd_table(views, reference_binning, seg1_fraction)
        for k, v in enumerate(views):
            arr[k].binning_capacity = cap
            arr[k].depth_key_bits = key_bits
            arr[k].depth_order_from = -1 if order_from is None else order_from[k]
            v.cap = cap
            if hint is not None and hint[k] is not None:
                v.mismatch = torch.zeros(1, dtype=torch.int32, device="cuda")
                arr[k].depth_order_hint, arr[k].hint_mismatch, arr[k].hint_trusted = hint[k].geom.data_ptr(), v.mismatch.data_ptr(), trusted
        self.lib.check(self.L.b3gs_forward_raw_batch(len(views), arr, C.byref(self.rp), phases, self.stream), "b3gs_forward_raw_batch")
        torch.cuda.synchronize()


def bin_state(v):
    """Host copies of what phase 1 left in view v."""
    from binocular3dgs_amd.debug import state_views
    s = state_views(v.P, v.W, v.H, v.cap, v.geom, v.binning, v.img)
    u32 = lambda t: t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF  # noqa: E731
    n = int(v.n.item())
    m = min(n, v.cap)
    return dict(N=n, counts=u32(s["counts"]).tolist(), keys=u32(s["depth_bits"]), touched=u32(s["tiles_touched"]),
                records=s["records"].cpu().numpy().copy(), radii=v.radii.cpu().numpy(), point_list=u32(s["point_list"])[:m],
                tile_ids=u32(s["tile_ids"])[:m], ranges=u32(s["ranges"]), ranges2=u32(s["ranges2"]), flag=int(v.flag.item()),
                high=int(v.high.item()), W=v.W, H=v.H)


def reference(st, tight=False, keys=None):
    """binning_ref on the device's keys (or a donor's) and the rects recomputed from its records; the rect guard."""
    rect = binning_ref.rects_from_records(st["records"], st["radii"], st["W"], st["H"], tight)
    binning_ref.guard_rects(rect, st["touched"])
    return binning_ref.Lists(st["keys"] if keys is None else keys, rect, st["W"], st["H"])


def assert_exact(name, st, ref):
    assert st["N"] == ref.N and st["counts"] == [ref.N, ref.V, 0], f"{name}: N {st['N']} counts {st['counts']} against N {ref.N} V {ref.V}"
    assert st["high"] == ref.N, f"{name}: high water {st['high']}"
    for k, want in (("point_list", ref.point_list), ("tile_ids", ref.tile_ids), ("ranges", ref.ranges)):
        bad = np.nonzero(st[k] != want)
        assert len(bad[0]) == 0, f"{name}: {k} differs at {len(bad[0])} places, first {bad[0][:4]}: {st[k][bad][:4]} against {want[bad][:4]}"
    assert not st["ranges2"].any(), f"{name}: a second segment after one round"


def visible_keys(st):
    return st["keys"][st["keys"] != binning_ref.CULLED]


def n_ties(st):
    k = visible_keys(st)
    return len(k) - len(np.unique(k))


def same_bytes(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("point_list", "tile_ids", "ranges")) and a["N"] == b["N"] and a["counts"] == b["counts"]


SEAM_SIZES = ((64, 48), (80, 48), (48, 64))


def run_modes(name, d, sizes=None, tight=False, populate=None):
    """Scene d as a single view and (sizes) as a batch, with four 8-bit passes (depth_key_bits 0) and three 9-bit passes
    (27): every view exact, the two sorts byte-identical.  -> state of the single view, its reference"""
    dev = BinDevice(d)
    out = {}
    for label, ds in (("single", [d]),) + ((("batch", helpers.binning_views(d, sizes)),) if sizes else ()):
        for bits in (0, 27):
            views = dev.views(ds)
            dev.launch(views, key_bits=bits, reference_binning=0 if tight else 1)
            for k, v in enumerate(views):
                st = bin_state(v)
                ref = reference(st, tight)
                if populate and bits == 0:
                    populate(f"{name} {label}[{k}]", st, ref)
                assert st["flag"] == 0, f"{name} {label}[{k}] bits {bits}: overflow word {st['flag']}"
                assert_exact(f"{name} {label}[{k}] bits {bits}", st, ref)
                if bits == 27:
                    assert same_bytes(st, out[label, 0, k][0]), f"{name} {label}[{k}]: the 9-bit sort differs from the 8-bit sort"
                out[label, bits, k] = (st, ref)
    return out["single", 0, 0]


@pytest.mark.parametrize("P", helpers.BIN_SEAM_P)
def test_depth_sort_tile_seams(P):
    def populate(name, st, ref):
        culled = int((st["keys"] == binning_ref.CULLED).sum())
        print(f"{name}: P {P} N {ref.N} V {ref.V} culled {culled} ties {n_ties(st)}")
        assert culled == len(range(7, P, 20)) and ref.V <= P - culled, name
        assert (st["keys"][7::20] == binning_ref.CULLED).all(), "culled keys interleaved by index"
        if "single" in name:
            assert ref.N > ref.V or P < 20, "some splats reach more than one tile"
            assert n_ties(st) <= P // 500 + 1      # (random float32 depths: a birthday's worth)
    run_modes("seam", helpers.binning_scene("seam", P), SEAM_SIZES, populate=populate)


def _ties_population(kind, P, tight=False):
    def populate(name, st, ref):
        k = visible_keys(st)
        d = k - KEY27_BASE
        print(f"{name}: {kind} P {P} N {ref.N} V {ref.V} distinct keys {len(np.unique(k))} ties {n_ties(st)}")
        assert (k > KEY27_BASE).all() and (d < KEY27_SPAN - 2).all()
        if kind == "ties_one":
            assert len(np.unique(k)) == 1
        elif kind == "ties3":
            assert len(np.unique(k)) == 3
        elif kind == "ties_low9":
            assert len(np.unique(k >> 9)) == 1 and len(np.unique(k)) > 256
        else:
            assert not (d & ~(0x1FF << 18) & ~1).any() and len(np.unique(k)) > 256
        assert n_ties(st) > P // 2 and ref.N > ref.V
        if "single" in name:      # (tight: the Gaussians below 1/255, every 11th, have no tile)
            assert ref.V > (0.85 if tight else 0.9) * P - 1
    return populate


@pytest.mark.parametrize("tight", [False, True], ids=["reference_rects", "tight_rects"])
@pytest.mark.parametrize("P", [4097, 8193])
@pytest.mark.parametrize("kind", ["ties_one", "ties3", "ties_low9", "ties_mid9"])
def test_stability_of_tied_depths(kind, P, tight):
    d = helpers.binning_scene(kind, P)
    if tight:
        d["opacities"] = d["opacities"].clone()
        d["opacities"][3::11] = 0.003          # below 1/255: no tile under tight binning
    st, ref = run_modes(kind, d, SEAM_SIZES if not tight else None, tight=tight, populate=_ties_population(kind, P, tight))
    if tight:
        check_tight_against_full(kind, d, st, ref)


def check_tight_against_full(name, d, st, ref):
    """st / ref: the tight lists (already exact); against the 3-sigma lists of the same scene: order-preserving sub-lists"""
    dev = BinDevice(d)
    (v,) = dev.views([d])
    dev.launch([v], reference_binning=1)
    full = reference(bin_state(v))
    faint = d["opacities"].numpy().reshape(-1) < 1.0 / 255
    assert faint.sum() > 0 and (ref.tiles_touched[faint] == 0).all() and (full.tiles_touched[faint] > 0).any()
    assert 0 < ref.N < full.N
    print(f"{name} tight: N {ref.N} of {full.N}, {int(faint.sum())} Gaussians below 1/255")
    for t in range(ref.tiles):
        a, b = st["point_list"][st["ranges"][t, 0]:st["ranges"][t, 1]], full.tile_list(t)
        assert len(a) <= len(b) and np.array_equal(a, b[np.isin(b, a)]), f"{name}: tile {t} is no sub-list of the 3-sigma list"


def test_key_span_edges():
    def populate(name, st, ref):
        k = visible_keys(st)
        assert k.min() == KEY27_BASE + 1 and k.max() == KEY27_BASE + KEY27_SPAN - 3 and len(k) == 300
        assert (st["keys"][[11, 200]] == k.min()).all() and (st["keys"][[12, 201]] == k.max()).all()
        assert all(g in ref.point_list for g in (11, 12, 200, 201)) and ref.tiles_touched[[11, 12]].min() >= 1
        print(f"{name}: N {ref.N} V {ref.V} min key base+{k.min() - KEY27_BASE} max key base+2^27-{KEY27_SPAN - (k.max() - KEY27_BASE)}")
    run_modes("span", helpers.binning_scene("span"), populate=populate)        # both sorts exact, overflow word 0
    d = helpers.binning_scene("span_out")
    dev = BinDevice(d)
    for bits in (27, 0):
        (v,) = dev.views([d])
        dev.launch([v], key_bits=bits)
        st = bin_state(v)
        assert visible_keys(st).max() == KEY27_BASE + KEY27_SPAN - 2 == st["keys"][100]
        assert st["flag"] == (2 if bits == 27 else 0), f"overflow word {st['flag']} with depth_key_bits {bits}"
        if bits == 0:
            assert_exact("span_out bits 0", st, reference(st))


@pytest.mark.parametrize("tight", [False, True], ids=["reference_rects", "tight_rects"])
@pytest.mark.parametrize("N", helpers.BIN_N_TARGETS)
def test_instance_count_seams(N, tight):
    d = helpers.binning_scene(f"count{N}")
    if tight:
        d["opacities"] = d["opacities"].clone()
        d["opacities"][3::11] = 0.003

    def populate(name, st, ref):
        print(f"{name}: N {st['N']} V {ref.V} two-tile {int((ref.tiles_touched == 2).sum())}")
        faint = len(range(3, N - 5, 11)) if tight else 0          # (tight: Gaussian 102, one of the two-tile ones, is faint)
        assert len(visible_keys(st)) == N - 5 and n_ties(st) <= N // 500 + 1 and ref.V == N - 5 - faint
        assert st["N"] == N - (faint + 1 if tight else 0) and int((ref.tiles_touched == 2).sum()) == (4 if tight else 5)
    st, ref = run_modes(f"count{N}", d, tight=tight, populate=populate)
    if tight:
        check_tight_against_full(f"count{N}", d, st, ref)


def test_one_gaussian_over_every_tile_at_a_sub_block_boundary():
    def populate(name, st, ref):
        big = np.nonzero(ref.tiles_touched == 100)[0]
        rank = np.argsort(ref.order)[big]
        print(f"{name}: N {ref.N} V {ref.V} Gaussians of 100 tiles at depth ranks {sorted(rank.tolist())}")
        assert sorted(rank.tolist()) == [255, 256] and ref.tiles == 100 and ref.V == 600 and ref.N == 598 + 200
    run_modes("cover", helpers.binning_scene("cover"), populate=populate)


def test_mostly_empty_rects():
    def populate(name, st, ref):
        print(f"{name}: N {ref.N} V {ref.V} of P 5000")
        assert 0 < ref.V <= 0.25 * 5000 and (st["keys"] != binning_ref.CULLED).sum() == 5000 - len(range(7, 5000, 20))
    run_modes("sparse", helpers.binning_scene("sparse"), populate=populate)


@pytest.mark.parametrize("name", ["onetile"] + list(helpers.BIN_TILE_IMAGES))
def test_digit_skew_and_tile_id_widths(name):
    def populate(tag, st, ref):
        tiles = np.unique(ref.tile_ids)
        print(f"{tag}: N {ref.N} V {ref.V} distinct tiles {len(tiles)} of {ref.tiles} grid_x {ref.gx}")
        if name == "onetile":
            assert tiles.tolist() == [5] and ref.N > 8192
        else:
            W, H, T = helpers.BIN_TILE_IMAGES[name]
            assert len(tiles) == T == ref.tiles and ref.gx == (W + 15) // 16 and (np.bincount(ref.tile_ids) >= 2).all()
    run_modes(name, helpers.binning_scene(name), populate=populate)


def test_eight_views_of_different_sizes_in_one_launch():
    d = helpers.binning_scene("seam", 5000)
    shifts = [(0.0, 0.0)] * 8
    shifts[2] = shifts[6] = (1.0e5, 0.0)          # nothing on screen: N = 0
    ds = helpers.binning_views(d, helpers.BIN_BATCH_SIZES, shifts)
    dev = BinDevice(d)
    for bits in (0, 27):
        views = dev.views(ds)
        dev.launch(views, key_bits=bits)
        alone = dev.views(ds)
        for v in alone:
            dev.launch([v], key_bits=bits)
        ns = []
        for k, (v, w) in enumerate(zip(views, alone)):
            st = bin_state(v)
            ref = reference(st)
            ns.append(ref.N)
            assert st["flag"] == 0
            assert_exact(f"batch of 8, view {k} bits {bits}", st, ref)
            assert same_bytes(st, bin_state(w)), f"view {k} launched alone differs"
        print(f"batch of 8 bits {bits}: N per view {ns}")
        assert ns[2] == ns[6] == 0 and all(n > 300 for k, n in enumerate(ns) if k not in (2, 6)) and len(set(ns)) >= 5


@pytest.mark.parametrize("order", [(-1, 0, -1), (-1, -1, 0)], ids=["adjacent", "non_adjacent"])
def test_shared_depth_orders(order):
    d = helpers.binning_scene("ties3", 8193)
    pair, other = (0.0, 0.0), (0.0, 0.5)            # the partner is moved along x only; the third view has other keys
    shifts = [pair, (0.3, 0.0), other] if order[1] == 0 else [pair, other, (0.3, 0.0)]
    ds = helpers.binning_views(d, ((64, 48), (64, 48), (80, 48)) if order[1] == 0 else ((64, 48), (80, 48), (64, 48)), shifts)
    dev = BinDevice(d)
    for bits in (0, 27):
        views = dev.views(ds)
        dev.launch(views, key_bits=bits, order_from=order)
        sts = [bin_state(v) for v in views]
        borrower, third = (1, 2) if order[1] == 0 else (2, 1)
        assert np.array_equal(sts[borrower]["keys"], sts[0]["keys"]) and not np.array_equal(sts[third]["keys"], sts[0]["keys"])
        assert not np.array_equal(sts[borrower]["touched"], sts[0]["touched"]), "the partner's rects are its own"
        for k, st in enumerate(sts):
            ref = reference(st, keys=sts[0]["keys"] if k == borrower else None)
            print(f"shared order {order} bits {bits} view {k}: N {ref.N} V {ref.V} ties {n_ties(st)}")
            assert st["flag"] == 0 and ref.N > 4096
            assert_exact(f"shared order {order} bits {bits} view {k}", st, ref)


@pytest.mark.parametrize("bits", [0, 27])
def test_adopted_depth_orders(bits):
    d = helpers.binning_scene("ties3", 8193)
    dev = BinDevice(d)
    (a,) = dev.views([d])
    dev.launch([a], key_bits=bits)
    sa = bin_state(a)
    assert_exact("forward A", sa, reference(sa))
    for trusted in (0, 1):                          # equal keys: adopted, nothing sorted
        (b,) = dev.views([d])
        dev.launch([b], key_bits=bits, hint=[a], trusted=trusted)
        sb = bin_state(b)
        assert int(b.mismatch.item()) == 0 and sb["flag"] == 0 and np.array_equal(sb["keys"], sa["keys"])
        assert_exact(f"forward B adopting A (trusted {trusted})", sb, reference(sb))
        assert same_bytes(sa, sb)
    j = int(np.nonzero(sa["touched"] > 0)[0][40])   # one key changed: the mismatch word is raised and B sorts itself
    dev.params[0][j, 2] = 5.5
    (b,) = dev.views([d])
    dev.launch([b], key_bits=bits, hint=[a])
    sb = bin_state(b)
    assert int(b.mismatch.item()) == 1 and sb["flag"] == 0 and int((sb["keys"] != sa["keys"]).sum()) == 1
    ref = reference(sb)
    assert_exact("forward B with one key changed", sb, ref)
    assert not np.array_equal(ref.order, binning_ref.depth_order(sa["keys"]))
    print(f"adopted orders bits {bits}: N {ref.N} V {ref.V} ties {n_ties(sb)}; Gaussian {j} moved")


def test_capacity():
    d = helpers.binning_scene("count4097")
    dev = BinDevice(d)
    full = None
    for cap in (4097, 4096, 4097 // 3):
        (v,) = dev.views([d])
        dev.launch([v], cap=cap)
        st = bin_state(v)
        ref = reference(st)
        assert st["N"] == ref.N == 4097, "the device N is the true N"
        if cap >= ref.N:
            assert st["flag"] == 0
            assert_exact("capacity N", st, ref)
            full = ref
            continue
        assert st["flag"] & 1 and not st["flag"] & ~1, f"overflow word {st['flag']}"
        r = st["ranges"][st["ranges"][:, 1] > st["ranges"][:, 0]]
        assert r[0, 0] == 0 and r[-1, 1] == cap and (r[1:, 0] == r[:-1, 1]).all(), f"ranges cover exactly {cap} entries, tile-major"
        for t in range(ref.tiles):
            b, e = st["ranges"][t]
            assert (st["tile_ids"][b:e] == t).all()
            assert binning_ref.is_subsequence(st["point_list"][b:e], full.tile_list(t)), f"capacity {cap}: tile {t}"
        print(f"capacity {cap} of N {ref.N}: overflow word {st['flag']}, lists hold {int((r[:, 1] - r[:, 0]).sum())} entries")


def test_packed_and_two_word_instances():
    """bits(P) + bits(tiles) > 32 flips the instances to two words: P = 65537 (17 bits) over 182 x 181 = 32942 tiles (16 bits),
    the smallest that flips short of an image of 65537 tiles; P = 65536 (16 bits) on the same image stays packed."""
    from binocular3dgs_amd import _lib
    W, H = 182 * 16, 181 * 16
    for P, want in ((65537, -1), (65536, 16)):
        rng = np.random.RandomState(P)
        spec = helpers._bin_spec(rng, W, H, P, rng.uniform(0.5, 40.0, P).astype(np.float32).astype(np.float64), big=0.0)
        d = helpers.splat_scene(W, H, **spec)
        dev = BinDevice(d)
        (v,) = dev.views([d])
        dev.launch([v], key_bits=27)
        dv = _lib.B3gsDebugViews()
        _lib.check(dev.L.b3gs_debug_views(P, W, H, CAPACITY, v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr(), C.byref(dv)), "b3gs_debug_views")
        assert dv.packed_idx_bits == want
        st = bin_state(v)
        ref = reference(st)
        print(f"P {P} {W}x{H}: packed_idx_bits {dv.packed_idx_bits} N {ref.N} V {ref.V} distinct tiles {len(np.unique(ref.tile_ids))}")
        assert ref.N > P and len(np.unique(ref.tile_ids)) > 24000 and ref.tile_ids.max() >= 32768
        assert_exact(f"P {P}", st, ref)


# ---- two rounds: the only case that runs the blend (phases = 3) ---------------------------------------------------------------
TWO_ROUND_CASES = ((4096 + 512, 4096, 0.5), (8192 + 300, 4096, 0.3), (8192 + 300, 8192, 0.6))      # P, K1, seg1_fraction
PAIR_SIZES, PAIR_SHIFTS = ((160, 16), (160, 16)), [(0.0, 0.0), (0.002, 0.0)]      # a view and its binocular partner


def _pred_words(v):
    """ImgView::pred_rows of view v (b3gs_internal.h, b3gs_img_view: behind ranges2 come tile_work, the tile order and
    open_rows, every array carved to a multiple of 256 bytes) as int64 words: tile (x, y) = bit x % 64 of word y * rw + x / 64.
    run_two_rounds pins the layout: what a two-round forward leaves there must be the tiles it left open."""
    from binocular3dgs_amd import _lib
    dv = _lib.B3gsDebugViews()
    _lib.check(_lib.lib().b3gs_debug_views(v.P, v.W, v.H, v.cap, v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr(), C.byref(dv)), "b3gs_debug_views")
    gx, gy = binning_ref.grid(v.W, v.H)
    a256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    rw = (gx + 63) // 64
    nbytes = 8 * (gy + 1) * rw
    o = dv.ranges2 - v.img.data_ptr() + a256(8 * gx * gy) + a256(4 * gx * gy) + a256(4 * 8 * (gx * gy + 8)) + a256(nbytes)
    assert o % 8 == 0 and o + 2 * a256(nbytes) <= v.img.numel()
    return v.img[o:o + 8 * gy * rw].view(torch.int64), gx, rw


def read_pred(v):
    words, gx, rw = _pred_words(v)
    w = words.cpu().numpy().astype(np.uint64)
    return [t for t in range(gx * (len(w) // rw)) if (int(w[(t // gx) * rw + (t % gx) // 64]) >> ((t % gx) % 64)) & 1]


def plant_pred(v, tiles):
    words, gx, rw = _pred_words(v)
    w = np.zeros(len(words), np.uint64)
    for t in tiles:
        w[(t // gx) * rw + (t % gx) // 64] |= np.uint64(1 << ((t % gx) % 64))
    words.copy_(torch.from_numpy(w.view(np.int64)).cuda())
    torch.cuda.synchronize()


def assert_two_rounds(name, st, want, n1_only=False):
    """point_list, tile_ids, ranges, ranges2 and the header words N1, V, N2 against binning_ref.Lists.two_rounds"""
    n = want["N1"] if n1_only else want["N1"] + want["N2"]
    assert st["counts"] == [want["N1"], want["V"], 0 if n1_only else want["N2"]] and st["N"] == n, \
        f"{name}: counts {st['counts']} N {st['N']} against N1 {want['N1']} V {want['V']} N2 {want['N2']}"
    for k in ("point_list", "tile_ids"):
        assert np.array_equal(st[k][:n], want[k][:n]), f"{name}: {k}"
    assert np.array_equal(st["ranges"], want["ranges"]), f"{name}: ranges"
    assert np.array_equal(st["ranges2"], np.zeros_like(want["ranges2"]) if n1_only else want["ranges2"]), f"{name}: ranges2"


def _segments(st):
    r1, r2 = st["ranges"], st["ranges2"]
    return [(st["point_list"][r1[t, 0]:r1[t, 1]], st["point_list"][r2[t, 0]:r2[t, 1]]) for t in range(len(r1))]


def _terminated_tiles(st, segs, bg):
    """Tiles whose every pixel saturates (transmittance test below 1e-4) inside segment 1, by the float64 blend reference on
    the device's records.  (The blend stores final_T BEFORE the saturating entry, so a stored final_T is never below 1e-4:
    "terminated" is read from the reference's saturation position, which is the rule the kernels apply.)  The verdict must
    not hang on float32 rounding: it has to be the same with the threshold moved by a thousandth either way."""
    import blend_ref
    gx = (st["W"] + 15) // 16
    verdicts = []
    eps = blend_ref.T_EPS
    try:
        for scale in (1.0, 1.0 - 1e-3, 1.0 + 1e-3):
            blend_ref.T_EPS = eps * scale
            b = blend_ref.forward(st["records"], [s1 for s1, _ in segs], st["W"], st["H"], bg)
            out = []
            for t in range(len(segs)):
                px, py, inside, _q = blend_ref._tile_pixels(t, gx, st["W"], st["H"])
                out.append(bool((b.sat_pos[py[inside], px[inside]] >= 0).all()))
            verdicts.append(out)
    finally:
        blend_ref.T_EPS = eps
    assert verdicts[0] == verdicts[1] == verdicts[2], "a tile terminates within rounding of the 1e-4 threshold: fragile scene"
    return verdicts[0]


def run_two_rounds(P, K1, frac):
    d = helpers.two_segment_scene(P, K1)
    ds = helpers.binning_views(d, PAIR_SIZES, PAIR_SHIFTS)
    dev = BinDevice(d)
    views = dev.views(ds)
    dev.launch(views, phases=3, key_bits=27, seg1_fraction=frac, order_from=(-1, 0))          # first forward: nothing predicted
    first = [bin_state(v) for v in views]
    predicted = []
    for k, st in enumerate(first):
        assert st["flag"] == 0, f"overflow word {st['flag']}"
        ref = reference(st, keys=first[0]["keys"])
        assert ref.order[K1 - 1] != ref.order[K1] and len(ref.order) == P > K1
        segs = _segments(st)
        term = _terminated_tiles(st, segs, ds[k]["bg"].numpy())
        whole, closed = [], []
        for t, (s1, s2) in enumerate(segs):
            b, e = ref.ranges[t]
            full, rk = ref.point_list[b:e], ref.rank[b:e]
            assert np.array_equal(s1, full[rk < K1]), f"view {k} tile {t}: segment 1 is not the entries of rank < K1"
            if np.array_equal(np.concatenate([s1, s2]), full):
                whole.append(t)
            else:
                assert len(s2) == 0 and term[t], f"view {k} tile {t}: segment 1 alone in a tile that did not terminate"
                closed.append(t)
        repaired = [t for t, (_, s2) in enumerate(segs) if len(s2)]
        want = ref.two_rounds(K1, [], whole)
        print(f"two rounds P {P} K1 {K1} view {k}: N1 {want['N1']} V {want['V']} N2 {want['N2']} of N {ref.N} V {ref.V}; closed tiles "
              f"{closed}, tiles with a segment 2 {repaired}")
        assert closed and repaired, "both kinds of tile occur"
        assert_two_rounds(f"first forward, view {k}", st, want)
        # what the forward left in the image buffer for the next one: the tiles it left open (at least those it repaired)
        pred = read_pred(views[k])
        assert set(repaired) <= set(pred) <= set(whole), f"view {k}: predicted {pred}, repaired {repaired}, closed {closed}"
        predicted.append(pred)
    dev.launch(views, phases=3, key_bits=27, seg1_fraction=frac, order_from=(-1, 0))          # second forward, same buffers
    for k, st in enumerate(bin_state(v) for v in views):
        ref = reference(st, keys=first[0]["keys"])
        assert st["flag"] == 0
        assert_two_rounds(f"second forward, view {k}", st, ref.two_rounds(K1, predicted[k], []))
        assert not st["ranges2"].any(), "every tile left open has its whole list in segment 1 now"
        for (a1, a2), (b1, b2) in zip(_segments(first[k]), _segments(st)):
            assert np.array_equal(np.concatenate([a1, a2]), np.concatenate([b1, b2])), "the union per tile is unchanged"


@pytest.mark.parametrize("P,K1,frac", TWO_ROUND_CASES)
def test_two_rounds_through_the_repair_launch(P, K1, frac):
    run_two_rounds(P, K1, frac)


def test_two_rounds_as_separate_launches():
    """B3GS_ROUND2_LEGACY is read once per process: the same checks in an interpreter of its own."""
    env = dict(os.environ, B3GS_ROUND2_LEGACY="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--two-round-child"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "two-round child: passed" in r.stdout, f"exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"


@pytest.mark.parametrize("P,K1,frac", TWO_ROUND_CASES[1:])
def test_adopted_order_carries_this_pairs_predicted_tiles(P, K1, frac):
    """Projection and binning only (phases = 1).  The donor forward runs into zeroed buffers -- nothing predicted, so its order
    words carry no predicted-tile flags.  A pair (view 0 adopts the donor's order, view 1 borrows view 0's) runs into image
    buffers in which two different sets of predicted tiles were planted: segment 1 of each must hold its OWN predicted tiles
    complete (the flags A and B of the adopted words are this pair's, not the donor's)."""
    d = helpers.two_segment_scene(P, K1)
    ds = helpers.binning_views(d, PAIR_SIZES, PAIR_SHIFTS)
    dev = BinDevice(d)
    (donor,) = dev.views(ds[:1])
    dev.launch([donor], key_bits=27, seg1_fraction=frac)
    sd = bin_state(donor)
    bare = reference(sd).two_rounds(K1, [], [])
    assert_two_rounds("donor", sd, bare, n1_only=True)
    views = dev.views(ds)
    planted = ([0, 3, 5], [1, 3, 8])
    for v, tiles in zip(views, planted):
        v.cap = CAPACITY
        plant_pred(v, tiles)
    dev.launch(views, key_bits=27, seg1_fraction=frac, order_from=(-1, 0), hint=[donor, None])
    assert int(views[0].mismatch.item()) == 0, "equal keys: the order is adopted"
    for k, v in enumerate(views):
        st = bin_state(v)
        assert st["flag"] == 0 and read_pred(v) == planted[k] and np.array_equal(st["keys"], sd["keys"])
        want = reference(st, keys=sd["keys"]).two_rounds(K1, planted[k], [])
        print(f"adopting pair P {P} K1 {K1} view {k}: N1 {want['N1']} V {want['V']} (nothing predicted: N1 {bare['N1']} V {bare['V']})")
        assert want["N1"] > bare["N1"] + 20 and want["V"] > bare["V"] + 20, "the planted tiles hold Gaussians behind K1"
        assert_two_rounds(f"adopting pair, view {k}", st, want, n1_only=True)


if __name__ == "__main__" and "--two-round-child" in sys.argv:
    for case in TWO_ROUND_CASES:
        run_two_rounds(*case)
    print("two-round child: passed")
