"""The blend kernels of csrc/render.hip against tests/blend_ref.py (float64), per pixel and per Gaussian, at their seams.

The library is driven through its C ABI: b3gs_forward_raw_batch(phases = 1) projects and bins, b3gs_blend_forward_batch and
b3gs_blend_backward_batch run only the blend, the backward into a zeroed scratch that is read before any chain rule.  The
reference runs on the device's own records and tile lists (debug.state_views), so projection and binning are out of the
comparison; pixel gradients are zeroed at the pixels whose decisions are fragile in the reference (helpers.FRAGILE_MARGIN).
Scenes: helpers.blend_scene / BLEND_CASES; what each holds is asserted from the device state before anything is compared.

Bounds (helpers.BLEND_*_BOUND) = 10 x the largest 99th percentile of float32 blend_ref against float64 blend_ref on these
scenes (tests/test_blend_ref_cpu.py measures them; never taken from the kernels).  Measured, 99th percentile of
image error / (1 + |x|), |final_T error|, row_err:
    stack1    1.4e-8  3.0e-8  2.1e-7     stack63   4.3e-7  1.4e-6  1.9e-6     stack64   4.3e-7  1.4e-6  2.0e-6
    stack65   4.4e-7  1.4e-6  2.2e-6     stack127  9.8e-7  1.8e-6  3.6e-6     stack128  1.0e-6  1.8e-6  3.6e-6
    stack129  1.0e-6  1.8e-6  3.7e-6     stack255  2.0e-6  2.0e-6  1.0e-5     stack256  2.0e-6  2.0e-6  9.2e-6
    stack257  2.0e-6  2.0e-6  9.1e-6     stack513  3.3e-6  1.2e-6  1.0e-5     ladder_b  1.7e-6  1.3e-6  3.2e-6
    ladder_c  1.6e-6  1.3e-6  1.0e-5     cull 96x64 2.1e-7 1.5e-7  9.7e-7     cull 72x41 2.0e-7 1.6e-7  1.1e-6
    cull 75x33 1.7e-7 1.3e-7  1.5e-6     wide      3.7e-7  9.8e-7  1.9e-6
  largest: image 3.28e-6, final_T 2.01e-6, row_err 1.03e-5  ->  final_T 2.1e-5, rows 1.1e-4; the image figure asks for
  3.3e-5 (stack513, 513 blended entries per pixel), above the existing contract of 3e-5 (1 + |x|): the bound stays 3e-5.
Populations (reference binning; fragile pixels / strata as (members, lost to fragility)): stacks, wide: no fragile pixel;
ladder_b 1 of 1024, corner 91, sat_at_seam 255, late 13; ladder_c 0, corner 95, sat_at_seam 257, late 18; cull 96x64: 7 of
6144, cullable 200 (415 pairs), corner 321 (466 pairs), clamped 98 (2), faint 128, seam 24; cull 72x41: 5 of 2952, cullable
258, corner 311, clamped 88, faint 109; cull 75x33: 12 of 2475 (0.485 %), cullable 288 (1), corner 277 (1), clamped 75;
batch views 80x48 / 72x41 / 33x17: 6, 5, 0 fragile pixels, touched rows 576 / 559 / 522, cullable pairs 387 / 372 / 139, corner
pairs 409 / 416 / 452; two segments (160x16): no fragile pixel, len1 64, 70, 128, 100, 0, 256, 0, 30, 30, 30, len2 20, 30, 10,
70, 12, 40, 0, 10, 10, 0.
Two of the issue's mutations change no result and pass by construction: `Tw = test_T` (a saturated Tw stays below 1e-4, so the
stop fires again: only the early exits are lost -- on the two-round path it does change state, every tile is then flagged open,
which the two-segment test sees as a segment 2 in the terminated tile) and `hx > 8.0f` (equality is a single float value inside
the box's 0.05 pixel margin).
"""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import blend_ref
import helpers
from helpers import BLEND_CASES, BLEND_IMG_BOUND, BLEND_ROW_BOUND, BLEND_STRATA, BLEND_T_BOUND, FRAGILE_MARGIN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = 200000


class _View:
    """One view's device buffers and B3gsScene."""

    def __init__(self, L, d, P, K=1):
        from binocular3dgs_amd import _lib
        dev = "cuda"
        self.W, self.H, self.P = d["W"], d["H"], P
        self.keep = [d[k].float().contiguous().to(dev) for k in ("bg", "viewmatrix", "projmatrix", "campos")]
        bg, vm, pm, cp = self.keep
        # (K SH rows stored, the scene's active degree and scale modifier: 1, 0 and 1.0 in the blend and binning scenes)
        self.scene = _lib.B3gsScene(P, d.get("sh_degree", 0) if K > 1 else 0, K, self.W, self.H, d["tanfovx"], d["tanfovy"],
                                    d.get("scale_modifier", 1.0), 0, 0, bg.data_ptr(), None, None,
                                    None, None, None, None, None, vm.data_ptr(), pm.data_ptr(), cp.data_ptr())
        u8 = dict(dtype=torch.uint8, device=dev)
        self.geom = torch.zeros(L.b3gs_geometry_bytes(P), **u8)
        self.binning = torch.zeros(L.b3gs_binning_bytes(P, CAPACITY), **u8)
        self.img = torch.zeros(L.b3gs_image_bytes(self.W, self.H), **u8)
        self.color = torch.zeros(3, self.H, self.W, device=dev)
        self.depth = torch.zeros(1, self.H, self.W, device=dev)
        self.alpha = torch.zeros(1, self.H, self.W, device=dev)
        self.radii = torch.zeros(P, dtype=torch.int32, device=dev)
        self.n = torch.zeros(1, dtype=torch.int32, device=dev)
        self.scratch = torch.zeros(L.b3gs_backward_scratch_floats(P), device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)       # B3gsForwardView::overflow_flag
        self.high = torch.zeros(1, dtype=torch.int32, device=dev)

    def state(self):
        """Host copies of what the forward left: images, final_T, n_contrib, tile_work, records, lists."""
        from binocular3dgs_amd.debug import state_views
        v = state_views(self.P, self.W, self.H, CAPACITY, self.geom, self.binning, self.img)
        tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        # tile_work follows ranges2 in the image buffer, each carved to a multiple of 256 bytes (b3gs_internal.h, b3gs_img_view)
        from binocular3dgs_amd import _lib
        dv = _lib.B3gsDebugViews()
        _lib.check(_lib.lib().b3gs_debug_views(self.P, self.W, self.H, CAPACITY, self.geom.data_ptr(), self.binning.data_ptr(),
                                               self.img.data_ptr(), C.byref(dv)), "b3gs_debug_views")
        o = dv.ranges2 - self.img.data_ptr() + ((tiles * 8 + 255) // 256) * 256
        work = self.img[o:o + 4 * tiles].view(torch.int32).cpu().numpy().astype(np.int64)
        self.order_offset = o + ((tiles * 4 + 255) // 256) * 256     # the backward's tile order follows tile_work
        n = int(self.n.item())
        assert 0 < n <= CAPACITY
        lists, len1 = blend_ref.tile_lists(v["point_list"].cpu().numpy(), v["ranges"].cpu().numpy(),
                                           v["point_list2"].cpu().numpy(), v["ranges2"].cpu().numpy())
        # ... which pins that layout: the words read as tile_work must be each tile's deepest n_contrib on the device's own data
        nc = v["n_contrib"].cpu().numpy().astype(np.int64)
        gx = (self.W + 15) // 16
        for t in range(tiles):
            px, py, inside, _q = blend_ref._tile_pixels(t, gx, self.W, self.H)
            assert work[t] == nc[py[inside], px[inside]].max() <= len(lists[t]), f"tile_work[{t}] = {work[t]}: image buffer layout?"
        return dict(color=self.color.cpu().numpy().astype(np.float64), depth=self.depth[0].cpu().numpy().astype(np.float64),
                    alpha=self.alpha[0].cpu().numpy().astype(np.float64), final_T=v["final_T"].cpu().numpy().astype(np.float64),
                    n_contrib=v["n_contrib"].cpu().numpy().astype(np.int64), work=work, records=v["records"].cpu().numpy().copy(),
                    lists=lists, len1=len1, bg=self.keep[0].cpu().numpy())


class Device:
    """The Gaussians of a scene dict on the device, and the three calls of the blend on views of them."""

    def __init__(self, d, K=1):
        """K: the SH rows of d["shs"] to store (row 0 in features_dc, rows 1.. in features_rest)"""
        from binocular3dgs_amd import _lib
        self.lib = _lib
        self.L = _lib.lib()
        dev = "cuda"
        self.P, self.K = d["means3D"].shape[0], K
        op = d["opacities"].double().reshape(-1, 1)
        self.params = [d["means3D"].float(), d["shs"][:, :1].float(), torch.log(d["scales"].double()).float(),
                       d["rotations"].float(), torch.log(op / (1 - op)).float()]
        self.params = [p.contiguous().to(dev) for p in self.params]
        self.rest = d["shs"][:, 1:K].float().contiguous().to(dev) if K > 1 else None
        self.rp = _lib.B3gsRawParams()
        self.rp.xyz, self.rp.features_dc = self.params[0].data_ptr(), self.params[1].data_ptr()
        self.rp.features_rest = None if self.rest is None else self.rest.data_ptr()
        self.rp.scaling, self.rp.rotation, self.rp.opacity = (p.data_ptr() for p in self.params[2:])
        self.stream = torch.cuda.current_stream().cuda_stream

    def views(self, ds):
        return [_View(self.L, d, self.P, self.K) for d in ds]

    def _fwd_table(self, views, reference_binning, seg1_fraction=0.0):
        arr = (self.lib.B3gsForwardView * len(views))()
        for k, v in enumerate(views):
            arr[k].view = C.pointer(v.scene)
            arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
            arr[k].binning_capacity = CAPACITY
            arr[k].out_color, arr[k].out_depth, arr[k].out_alpha = v.color.data_ptr(), v.depth.data_ptr(), v.alpha.data_ptr()
            arr[k].radii, arr[k].device_num_rendered, arr[k].depth_order_from = v.radii.data_ptr(), v.n.data_ptr(), -1
            arr[k].reference_binning = int(reference_binning)
            arr[k].seg1_fraction = seg1_fraction
            arr[k].overflow_flag, arr[k].high_water = v.flag.data_ptr(), v.high.data_ptr()
        return arr

    def _blend_table(self, views, grads=None):
        arr = (self.lib.B3gsBlendView * len(views))()
        keep = []
        for k, v in enumerate(views):
            arr[k].view = C.pointer(v.scene)
            arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
            arr[k].out_color, arr[k].out_depth, arr[k].out_alpha = v.color.data_ptr(), v.depth.data_ptr(), v.alpha.data_ptr()
            arr[k].binning_capacity = CAPACITY
            if grads is not None:
                g = [None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda") for a in grads[k]]
                keep += g
                arr[k].dL_dcolor = g[0].data_ptr()
                arr[k].dL_ddepth = None if g[1] is None else g[1].data_ptr()
                arr[k].dL_dalpha = None if g[2] is None else g[2].data_ptr()
                v.scratch.zero_()
                arr[k].scratch = v.scratch.data_ptr()
        return arr, keep

    def bin(self, views, reference_binning=1):
        arr = self._fwd_table(views, reference_binning)
        self.lib.check(self.L.b3gs_forward_raw_batch(len(views), arr, C.byref(self.rp), 1, self.stream), "b3gs_forward_raw_batch(1)")
        torch.cuda.synchronize()

    def forward_whole(self, views, reference_binning=1, seg1_fraction=0.0):
        """projection + binning + blend in one call: the forward that adopts the tile order a backward left in the image buffer,
        and the only one that bins in two rounds (0 < seg1_fraction < 1)"""
        arr = self._fwd_table(views, reference_binning, seg1_fraction)
        self.lib.check(self.L.b3gs_forward_raw_batch(len(views), arr, C.byref(self.rp), 3, self.stream), "b3gs_forward_raw_batch(3)")
        torch.cuda.synchronize()

    def blend_forward(self, views):
        arr, _ = self._blend_table(views)
        self.lib.check(self.L.b3gs_blend_forward_batch(len(views), arr, self.stream), "b3gs_blend_forward_batch")
        torch.cuda.synchronize()

    def blend_backward(self, views, grads):
        """-> per view the scratch rows [P, 10] (float64), read before any chain rule"""
        arr, keep = self._blend_table(views, grads)
        self.lib.check(self.L.b3gs_blend_backward_batch(len(views), arr, self.stream), "b3gs_blend_backward_batch")
        torch.cuda.synchronize()
        del keep
        return [v.scratch.cpu().numpy().reshape(self.P, 10).astype(np.float64) for v in views]


_REF = {}


def _reference(key, dev_state, W, H):
    """float64 blend_ref on the device's records and lists: computed once per (scene, records, lists), shared by the tests
    and -- through B3GS_TEST_BLEND_CACHE, a directory -- by the child interpreters of the variant test."""
    sig = (key, dev_state["records"][:, :12].tobytes(), tuple(a.tobytes() for a in dev_state["lists"]))
    h = str(hash(sig) & 0xFFFFFFFFFFFF)
    if h in _REF:
        return _REF[h]
    cache = os.environ.get("B3GS_TEST_BLEND_CACHE")
    path = os.path.join(cache, f"{key}_{W}x{H}.pkl") if cache else None
    if path and os.path.exists(path):
        with open(path, "rb") as f:
            got = pickle.load(f)
        if got["sig"] == sig:
            _REF[h] = got["ref"]
            return got["ref"]
    st = blend_ref.forward(dev_state["records"], dev_state["lists"], W, H, dev_state["bg"])
    ok = st.margin >= FRAGILE_MARGIN
    gc, gd, ga = (g * ok for g in helpers.blend_pixel_grads(W, H))
    masks, lost, pr = blend_ref.strata(st, FRAGILE_MARGIN)
    ref = dict(st=st, ok=ok, grads=(gc, gd, ga), rows=blend_ref.backward(st, gc, gd, ga), masks=masks, lost=lost, pr=pr,
               touched=blend_ref.touched_rows(st, FRAGILE_MARGIN), solid=blend_ref.tile_solid(st, FRAGILE_MARGIN))
    _REF[h] = ref
    if path:
        with open(path, "wb") as f:
            pickle.dump(dict(sig=sig, ref=ref), f)
    return ref


def check_forward(name, got, ref):
    st, ok = ref["st"], ref["ok"]
    assert ok.mean() >= 0.995, f"{name}: {(~ok).sum()} fragile pixels of {ok.size}"
    bad = got["n_contrib"][ok] != st.n_contrib[ok]
    assert not bad.any(), f"{name}: n_contrib differs at {int(bad.sum())} non-fragile pixels"
    for k, a, b in (("colour", got["color"], st.color), ("depth", got["depth"], st.depth), ("alpha", got["alpha"], st.alpha)):
        e = (np.abs(a - b) / (1 + np.abs(b)))[..., ok]
        print(f"{name}: {k} max error / (1 + |x|) {e.max():.2e}")
        assert e.max() <= BLEND_IMG_BOUND, f"{name}: {k} off by {e.max():.2e}"
    e = np.abs(got["final_T"] - st.final_T)[ok]
    print(f"{name}: final_T max error {e.max():.2e}")
    assert e.max() <= BLEND_T_BOUND, f"{name}: final_T off by {e.max():.2e}"
    solid = ref["solid"]
    assert np.array_equal(got["work"][solid], st.work[solid]), f"{name}: tile_work {got['work']} against {st.work}"


def check_rows(name, rows, ref, rows_ref=None, strata=True):
    rows_ref = ref["rows"] if rows_ref is None else rows_ref
    touched = ref["touched"]
    assert touched.any()
    stray = np.nonzero(rows[~touched].any(1))[0]
    assert len(stray) == 0, f"{name}: {len(stray)} Gaussians that are live at no solid pixel received a gradient"
    err = helpers.row_err(rows, rows_ref, touched)
    print(f"{name}: row_err 99th percentile {np.percentile(err, 99):.2e} max {err.max():.2e} over {int(touched.sum())} rows")
    masks = {k: ref["masks"][k] & ~ref["lost"][k] for k in BLEND_STRATA}
    names = tuple(k for k in BLEND_STRATA if strata and (masks[k] & touched).any())
    bad = helpers.row_failures(rows, rows_ref, touched, strata=masks, bound=BLEND_ROW_BOUND, names=names)
    assert not bad, f"{name}: rows above {BLEND_ROW_BOUND}: {bad}"
    for where in ("all",) + names:
        m = touched if where == "all" else (touched & masks[where])
        for c, col in enumerate(blend_ref.COLS):
            den = np.linalg.norm(rows_ref[m, c])
            if den == 0.0:
                assert not rows[m, c].any(), f"{name}: column {col} must be exactly zero ({where})"
                continue
            e = np.linalg.norm(rows[m, c] - rows_ref[m, c]) / den
            assert e <= 2e-4, f"{name}: column {col} relative L2 {e:.2e} over {where} ({int(m.sum())} rows)"


def run_case(name, W, H, reference_binning=1):
    """One scene, one view: bin, blend forward, blend backward; everything checked against the reference.  -> (state, ref)"""
    d = helpers.blend_scene(name, W, H)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.bin([v], reference_binning)
    dev.blend_forward([v])
    got = v.state()
    ref = _reference(f"{name}_rb{reference_binning}", got, v.W, v.H)
    pop, npairs = helpers.blend_populations(name, ref["st"], ref["masks"], ref["lost"], ref["pr"], tight=not reference_binning)
    print(f"{name} {v.W}x{v.H} reference_binning={reference_binning}: strata (members, lost) {pop}, pairs {npairs}")
    check_forward(name, got, ref)
    (rows,) = dev.blend_backward([v], [ref["grads"]])
    check_rows(name, rows, ref)
    return dev, v, got, ref


@pytest.mark.parametrize("name,W,H", BLEND_CASES)
def test_blend_against_float64_reference(name, W, H):
    run_case(name, W, H)


def test_null_depth_and_alpha_gradients_equal_zeros_passed():
    d = helpers.blend_scene("cull", 72, 41)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.bin([v])
    dev.blend_forward([v])
    ref = _reference("cull_rb1", v.state(), v.W, v.H)
    gc, gd, ga = ref["grads"]
    z = np.zeros_like(gd)
    for gd_, ga_ in ((gd, None), (None, ga), (None, None)):
        want = blend_ref.backward(ref["st"], gc, z if gd_ is None else gd_, z if ga_ is None else ga_)
        (rows_null,) = dev.blend_backward([v], [(gc, gd_, ga_)])
        (rows_zero,) = dev.blend_backward([v], [(gc, z if gd_ is None else gd_, z if ga_ is None else ga_)])
        for tag, rows in (("NULL", rows_null), ("zeros", rows_zero)):
            check_rows(f"cull 72x41 depth={'-' if gd_ is None else 'x'} alpha={'-' if ga_ is None else 'x'} {tag}", rows, ref,
                       rows_ref=want, strata=False)
        if gd_ is None:
            assert not rows_null[:, 3].any() and not rows_zero[:, 3].any()     # depth column: exact zeros either way


def test_three_resolutions_in_one_launch_each_way():
    sizes, ds = helpers.BLEND_BATCH_SIZES, helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.bin(views)
    dev.blend_forward(views)
    refs = []
    for (W, H), v in zip(sizes, views):
        got = v.state()
        ref = _reference(f"batch{W}x{H}", got, W, H)
        fig = helpers.blend_batch_populations(ref["st"], ref["pr"], ref["touched"])
        print(f"batch {W}x{H}: {fig}, strata (members, lost) "
              f"{ {k: (int(ref['masks'][k].sum()), int(ref['lost'][k].sum())) for k in BLEND_STRATA} }")
        check_forward(f"batch {W}x{H}", got, ref)
        refs.append(ref)
    rows = dev.blend_backward(views, [r["grads"] for r in refs])
    for (W, H), r, ref in zip(sizes, rows, refs):
        check_rows(f"batch {W}x{H}", r, ref, strata=False)


ORDER_MAGIC = 0xB365A0D1     # render.hip, B3GS_ORDER_MAGIC: "this image buffer holds a tile order", followed by its signature


def _tile_order(views):
    """The longest-tile-first order in view 0's image buffer -> (classes [8, cls_size] or None when absent, signature ok)."""
    blocks = [((((v.W + 15) // 16) * ((v.H + 15) // 16)) + 7) // 8 * 8 for v in views]
    total, v0 = sum(blocks), views[0]
    tiles0 = ((v0.W + 15) // 16) * ((v0.H + 15) // 16)
    words = 8 * (tiles0 + 8)
    o = v0.order_offset
    arr = v0.img[o:o + 4 * words].view(torch.int32).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    if arr[words - 2] != ORDER_MAGIC:
        return None, False
    return arr[:total].reshape(8, total // 8), arr[words - 1] == total * 16 + len(views)


@pytest.mark.parametrize("mixed", [False, True])
def test_forward_after_backward_is_bit_identical(mixed):
    """forward, backward, forward again into the same image buffers: the second forward runs its tiles in the order the
    backward left there (cull fields of 60 tiles -- eight per class of workgroups -- with unequal work, so that the order is a
    real permutation: asserted from the image buffer).  Images, n_contrib and final_T must not change by a bit."""
    sizes = ((160, 96), (144, 82)) if mixed else ((160, 96),)
    ds = helpers.blend_batch_scenes("cull_order", sizes)
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    first = [v.state() for v in views]
    assert len(set(first[0]["work"].tolist())) > 8, "tiles of unequal work"
    assert _tile_order(views)[0] is None, "no order before the first backward"
    dev.blend_backward(views, [helpers.blend_pixel_grads(v.W, v.H) for v in views])
    order, sig_ok = _tile_order(views)
    assert order is not None and sig_ok, "the backward left no order for this batch shape in view 0's image buffer"
    cls = order.shape[1]
    assert cls >= 8 and all(sorted(row.tolist()) == list(range(cls)) for row in order), "every class is a permutation"
    moved = int((order != np.arange(cls)).sum())
    print(f"tile order: {order.shape[0]} classes of {cls}, {moved} of {order.size} positions moved")
    assert moved >= order.size // 4, "the order is (nearly) the identity: the second forward would test nothing"
    dev.forward_whole(views)
    assert _tile_order(views)[1], "the order is still there after the forward that used it"
    for a, v in zip(first, views):
        b = v.state()
        for k in ("color", "depth", "alpha", "final_T", "n_contrib", "work"):
            assert np.array_equal(a[k], b[k]), k


def run_two_segments():
    """Two binning rounds (P = 4096 + 512, segment 1 = the nearest 4096): len1 on and inside a mask word, a tile of segment 2
    only, a terminated tile that must not get a segment 2, lists crossing a chunk behind the switch -- all asserted from the
    device's ranges / ranges2; then everything against blend_ref, the re-blend of the finished state bit for bit, the rows."""
    d = helpers.two_segment_scene()
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v], seg1_fraction=0.5)
    assert int(v.flag.item()) == 0, f"overflow word {int(v.flag.item())} (bit 2: the second round's launch gave up)"
    got = v.state()
    len1 = got["len1"]
    len2 = np.array([len(a) for a in got["lists"]]) - len1
    print(f"two segments: N={int(v.n.item())} len1 {len1.tolist()} len2 {len2.tolist()}")
    helpers.two_segment_populations(len1, len2)
    for t, (n1, n2) in helpers.TWO_SEG_TILES.items():
        assert (len1[t], len2[t]) == (n1, n2), (t, len1[t], len2[t])
    ref = _reference("two_segments", got, v.W, v.H)
    check_forward("two segments", got, ref)
    dev.blend_forward([v])                      # every tile again over segment 1 + segment 2
    again = v.state()
    for k in ("color", "depth", "alpha", "final_T", "n_contrib", "work"):
        assert np.array_equal(got[k], again[k]), k
    (rows,) = dev.blend_backward([v], [ref["grads"]])
    check_rows("two segments", rows, ref)


def test_two_segments_with_len1_on_and_inside_a_mask_word():
    run_two_segments()


@pytest.mark.parametrize("name", ["cull", "ladder_b", "ladder_c"])
def test_tight_binning_against_reference_and_against_reference_binning(name):
    _dev, _v, tight, ref_t = run_case(name, None, None, reference_binning=0)
    _dev, _v, full, ref_f = run_case(name, None, None, reference_binning=1)
    assert sum(len(a) for a in tight["lists"]) <= sum(len(a) for a in full["lists"])
    ok = ref_t["ok"] & ref_f["ok"]
    for k in ("color", "depth", "alpha"):
        e = (np.abs(tight[k] - full[k]) / (1 + np.abs(full[k])))[..., ok]
        assert e.max() <= BLEND_IMG_BOUND, (k, e.max())


# ---- the backward variants, each in an interpreter of its own (the switch is read once per process) ------------------------
VARIANTS = (("default", {}), ("wave", {"B3GS_BWD_KERNEL": "wave"}), ("tile", {"B3GS_BWD_KERNEL": "tile"}),
            ("tile128", {"B3GS_BWD_KERNEL": "tile", "B3GS_BWD_CHUNK": "128"}),
            ("tile256", {"B3GS_BWD_KERNEL": "tile", "B3GS_BWD_CHUNK": "256"}))
_child_died = []


def _child_main():
    for name, W, H in BLEND_CASES:
        run_case(name, W, H)
    run_two_segments()
    print("variant child: all scenes passed")


def test_variant_switches_are_the_ones_the_launcher_reads():
    """Which kernel a launch took cannot be read back through the C ABI; what can be pinned is that the names and values the
    children set are the ones b3gs_launch_blend_backward compares with (a renamed switch would run the default five times)."""
    with open(os.path.join(ROOT, "binocular3dgs_amd", "csrc", "render.hip")) as f:
        src = f.read()
    for needle in ('getenv("B3GS_BWD_KERNEL")', '!strcmp(which, "tile")', '!strcmp(which, "wave")', 'getenv("B3GS_BWD_CHUNK")',
                   "bwd_chunk == 256", "bwd_chunk == 128"):
        assert needle in src, needle
    assert {v for _n, e in VARIANTS for v in e.values()} == {"tile", "wave", "128", "256"}


@pytest.mark.parametrize("variant,env_add", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_backward_variant_against_float64_reference(variant, env_add, tmp_path_factory):
    """Every scene of BLEND_CASES under one backward kernel, checked against blend_ref inside the child (never against another
    kernel).  A child that dies by a signal or runs out of time fails the test, and no further child is started."""
    if _child_died:
        pytest.fail(f"not started: the child of variant {_child_died[0]} died or timed out")
    env = {k: v for k, v in os.environ.items() if k not in ("B3GS_BWD_KERNEL", "B3GS_BWD_CHUNK")}
    env.update(env_add)
    cache = os.environ.get("B3GS_TEST_BLEND_CACHE") or str(tmp_path_factory.getbasetemp() / "blend_ref_cache")
    os.makedirs(cache, exist_ok=True)
    env["B3GS_TEST_BLEND_CACHE"] = cache
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant-child"], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired:
        _child_died.append(variant)
        pytest.fail(f"variant {variant}: the child ran out of time")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_died.append(variant)
    assert r.returncode == 0, f"variant {variant}: exit status {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-2500:]}"
    assert "all scenes passed" in r.stdout


if __name__ == "__main__" and "--variant-child" in sys.argv:
    _child_main()
