"""b3gs_blend_contribution_batch (csrc/contrib.hip) against tests/contrib_ref.py (float64), through the C ABI.

The forward runs with reference binning; the reference runs on the device's own records and tile lists (debug.state_views), so
projection and binning are out of the comparison.  The pixel mask handed to the device is zero at the pixels whose blend
decisions are fragile in the reference (helpers.FRAGILE_MARGIN) and at those whose two largest weights are a near-tie
(contrib_ref.TIE_THRESHOLD); the reference counts the same pixels.  Then hits and dominant are equal exactly, weight and wmax
within contrib_ref.WEIGHT_BOUND / WMAX_BOUND (10 x the float32 noise of the reference, measured in tests/test_contrib_ref_cpu.py,
never taken from the kernel), relative, with an absolute floor of 2^-32 per hit (the quantisation).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_ref
import contrib_ref
import helpers
from helpers import BLEND_IMG_BOUND, FRAGILE_MARGIN

pytestmark = pytest.mark.gpu
CAPACITY = 200000
CASES = tuple(("stack%d" % L, None, None) for L in (1, 63, 64, 65, 255, 256, 257, 513)) + (
    ("ladder_b", None, None), ("cull", 96, 64), ("cull", 72, 41), ("cull", 75, 33), ("wide", None, None))
KEYS = ("weight_q", "hits", "wmax_bits", "dominant")


class _View:
    """One view's device buffers and B3gsScene (as in tests/test_gpu_blend_edges.py)."""

    def __init__(self, L, d, P):
        from binocular3dgs_amd import _lib
        dev = "cuda"
        self.W, self.H, self.P = d["W"], d["H"], P
        self.keep = [d[k].float().contiguous().to(dev) for k in ("bg", "viewmatrix", "projmatrix", "campos")]
        bg, vm, pm, cp = self.keep
        self.scene = _lib.B3gsScene(P, 0, 1, self.W, self.H, d["tanfovx"], d["tanfovy"], 1.0, 0, 0, bg.data_ptr(), None, None,
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
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.high = torch.zeros(1, dtype=torch.int32, device=dev)

    def state(self):
        """Host copies of what the forward left: alpha image, n_contrib, records, lists (both segments), len1."""
        from binocular3dgs_amd.debug import state_views
        v = state_views(self.P, self.W, self.H, CAPACITY, self.geom, self.binning, self.img)
        assert 0 < int(self.n.item()) <= CAPACITY
        lists, len1 = blend_ref.tile_lists(v["point_list"].cpu().numpy(), v["ranges"].cpu().numpy(),
                                           v["point_list2"].cpu().numpy(), v["ranges2"].cpu().numpy())
        return dict(alpha=self.alpha[0].cpu().numpy().astype(np.float64), n_contrib=v["n_contrib"].cpu().numpy().astype(np.int64),
                    final_T=v["final_T"].cpu().numpy().astype(np.float64), records=v["records"].cpu().numpy().copy(), lists=lists,
                    len1=len1, bg=self.keep[0].cpu().numpy())


class Device:
    """The Gaussians of a scene dict on the device; the forward, the blend backward and the contribution call on views of them."""

    def __init__(self, d):
        from binocular3dgs_amd import _lib
        self.lib = _lib
        self.L = _lib.lib()
        dev = "cuda"
        self.P = d["means3D"].shape[0]
        op = d["opacities"].double().reshape(-1, 1)
        self.params = [d["means3D"].float(), d["shs"][:, :1].float(), torch.log(d["scales"].double()).float(),
                       d["rotations"].float(), torch.log(op / (1 - op)).float()]
        self.params = [p.contiguous().to(dev) for p in self.params]
        self.rp = _lib.B3gsRawParams()
        self.rp.xyz, self.rp.features_dc, self.rp.features_rest = self.params[0].data_ptr(), self.params[1].data_ptr(), None
        self.rp.scaling, self.rp.rotation, self.rp.opacity = (p.data_ptr() for p in self.params[2:])
        self.stream = torch.cuda.current_stream().cuda_stream

    def views(self, ds):
        return [_View(self.L, d, self.P) for d in ds]

    def forward_whole(self, views, seg1_fraction=0.0):
        arr = (self.lib.B3gsForwardView * len(views))()
        for k, v in enumerate(views):
            arr[k].view = C.pointer(v.scene)
            arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
            arr[k].binning_capacity = CAPACITY
            arr[k].out_color, arr[k].out_depth, arr[k].out_alpha = v.color.data_ptr(), v.depth.data_ptr(), v.alpha.data_ptr()
            arr[k].radii, arr[k].device_num_rendered, arr[k].depth_order_from = v.radii.data_ptr(), v.n.data_ptr(), -1
            arr[k].reference_binning = 1
            arr[k].seg1_fraction = seg1_fraction
            arr[k].overflow_flag, arr[k].high_water = v.flag.data_ptr(), v.high.data_ptr()
        self.lib.check(self.L.b3gs_forward_raw_batch(len(views), arr, C.byref(self.rp), 3, self.stream), "b3gs_forward_raw_batch(3)")
        torch.cuda.synchronize()

    def blend_backward(self, views, grads):
        arr = (self.lib.B3gsBlendView * len(views))()
        keep = []
        for k, v in enumerate(views):
            arr[k].view = C.pointer(v.scene)
            arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
            arr[k].out_color, arr[k].out_depth, arr[k].out_alpha = v.color.data_ptr(), v.depth.data_ptr(), v.alpha.data_ptr()
            arr[k].binning_capacity = CAPACITY
            g = [torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda") for a in grads[k]]
            keep += g
            arr[k].dL_dcolor, arr[k].dL_ddepth, arr[k].dL_dalpha = g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr()
            v.scratch.zero_()
            arr[k].scratch = v.scratch.data_ptr()
        self.lib.check(self.L.b3gs_blend_backward_batch(len(views), arr, self.stream), "b3gs_blend_backward_batch")
        torch.cuda.synchronize()
        return [v.scratch.cpu().numpy().copy() for v in views]

    def contrib(self, views, masks=None, out=None):
        """One call for `views` (masks: per view None or [H, W] array) -> dict of host arrays [P]: weight_q (int64), hits,
        wmax_bits, dominant (uint32 as int64) and wmax (float64 of the float32 the bits are).  out: device tensors to
        accumulate into (default: fresh zeros)."""
        dev = "cuda"
        if out is None:
            out = [torch.zeros(self.P, dtype=torch.int64, device=dev)] + [torch.zeros(self.P, dtype=torch.int32, device=dev) for _ in range(3)]
        arr = (self.lib.B3gsContribView * len(views))()
        keep = []
        for k, v in enumerate(views):
            arr[k].view = C.pointer(v.scene)
            arr[k].geometry, arr[k].binning, arr[k].image = v.geom.data_ptr(), v.binning.data_ptr(), v.img.data_ptr()
            if masks is not None and masks[k] is not None:
                m = torch.tensor(np.ascontiguousarray(masks[k]).astype(np.uint8), device=dev)
                assert m.shape == (v.H, v.W)
                keep.append(m)
                arr[k].pixel_mask = m.data_ptr()
        co = self.lib.B3gsContribOut(*(t.data_ptr() for t in out))
        self.lib.check(self.L.b3gs_blend_contribution_batch(len(views), arr, C.byref(co), self.stream), "b3gs_blend_contribution_batch")
        torch.cuda.synchronize()
        del keep
        res = dict(weight_q=out[0].cpu().numpy().copy())
        for name, t in zip(KEYS[1:], out[1:]):
            res[name] = t.cpu().numpy().view(np.uint32).astype(np.int64)
        res["wmax"] = res["wmax_bits"].astype(np.uint32).view(np.float32).astype(np.float64)
        res["out"] = out
        return res


_REF = {}


def _reference(key, got, W, H):
    """float64 blend_ref + contrib_ref on the device's records and lists, once per scene: -> (State, contributions without a
    mask, the mask of counted pixels)."""
    if key not in _REF:
        st = blend_ref.forward(got["records"], got["lists"], W, H, got["bg"])
        c = contrib_ref.contributions(st)
        _REF[key] = (st, c, contrib_ref.solid_mask(st, c, FRAGILE_MARGIN))
    return _REF[key]


def check_against(name, got, ref, hits_floor=True):
    assert np.array_equal(got["hits"], ref["hits"]), \
        f"{name}: hits differ at {np.nonzero(got['hits'] != ref['hits'])[0][:10]}"
    assert np.array_equal(got["dominant"], ref["dominant"]), \
        f"{name}: dominant differs at {np.nonzero(got['dominant'] != ref['dominant'])[0][:10]}"
    floor = 2.0 ** -32 * ref["hits"]
    w = got["weight_q"] / contrib_ref.Q32
    ew = np.abs(w - ref["weight"]) - floor
    em = np.abs(got["wmax"] - ref["wmax"]) - floor
    h = ref["hits"] > 0
    assert h.any()
    print(f"{name}: {int(h.sum())} Gaussians with hits, {int(ref['hits'].sum())} hits; largest relative error weight "
          f"{(np.abs(w - ref['weight'])[h] / ref['weight'][h]).max():.2e} wmax {(np.abs(got['wmax'] - ref['wmax'])[h] / ref['wmax'][h]).max():.2e}")
    assert (ew <= contrib_ref.WEIGHT_BOUND * ref["weight"]).all(), f"{name}: weight off by {(ew[h] / ref['weight'][h]).max():.2e} (relative)"
    assert (em <= contrib_ref.WMAX_BOUND * ref["wmax"]).all(), f"{name}: wmax off by {(em[h] / ref['wmax'][h]).max():.2e} (relative)"
    assert not got["weight_q"][~h].any() and not got["wmax_bits"][~h].any()


def run_case(name, W, H):
    d = helpers.blend_scene(name, W, H)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    got = v.state()
    st, c, solid = _reference(name + f"_{v.W}x{v.H}", got, v.W, v.H)
    assert (~solid).mean() <= contrib_ref.MASKED_CAP, f"{name}: {(~solid).sum()} pixels left out"
    assert np.array_equal(got["n_contrib"][solid], st.n_contrib[solid])
    return dev, v, got, st, c, solid


@pytest.mark.parametrize("name,W,H", CASES)
def test_contribution_against_float64_reference(name, W, H):
    dev, v, got, st, c, solid = run_case(name, W, H)
    # what the scene is here for, from the device's own lists
    if name.startswith("stack"):
        L = int(name[5:])
        assert len(st.ids[0]) == L and (st.n_contrib[:16, :16] == L).all(), "every pixel of tile 0 blends the whole stack"
        for seam in (64, 256):
            below, above = st.blended[0][:seam].any(), st.blended[0][seam:].any()
            assert below and above == (L > seam), f"stack{L}: entries in front of / behind list position {seam}"
            if L > seam:
                assert st.blended[0][seam - 1].all() and st.blended[0][seam].all()
    if (name, W, H) == ("cull", 75, 33):
        gx, gy = st.grid
        assert v.W % 16 and v.H % 16
        assert any(st.blended[t].any() for t in range(gx - 1, gx * gy, gx)), "a partial tile on the right edge with blended entries"
        assert any(st.blended[t].any() for t in range(gx * (gy - 1), gx * gy)), "a partial tile on the bottom edge"
    ref = contrib_ref.contributions(st, solid)
    check_against(f"{name} {v.W}x{v.H}", dev.contrib([v], [solid]), ref)


@pytest.mark.parametrize("name,W,H", [("cull", 75, 33), ("stack513", None, None), ("ladder_b", None, None)])
def test_device_only_invariants_without_mask_or_reference(name, W, H):
    d = helpers.blend_scene(name, W, H)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    got = v.state()
    r = dev.contrib([v])
    assert int(r["dominant"].sum()) == int((got["n_contrib"] > 0).sum()) > 0
    hits_total = int(r["hits"].sum())
    diff = abs(float(r["weight_q"].sum()) / contrib_ref.Q32 - got["alpha"].sum())
    print(f"{name}: {hits_total} hits, weight sum - alpha image sum = {diff:.3e}")
    assert diff <= hits_total * 2.0 ** -32 + BLEND_IMG_BOUND * v.H * v.W
    assert (r["dominant"] <= r["hits"]).all() and ((r["hits"] > 0) == (r["wmax_bits"] > 0)).all()
    assert ((r["hits"] > 0) == (r["weight_q"] > 0)).all()


def _fold(parts):
    return {k: (np.maximum.reduce([p[k] for p in parts]) if k == "wmax_bits" else np.sum([p[k] for p in parts], 0)) for k in KEYS}


def test_three_resolutions_in_one_call_equal_three_calls_in_any_order():
    ds = helpers.blend_batch_scenes()
    dev = Device(ds[0])
    views = dev.views(ds)
    dev.forward_whole(views)
    singles = [dev.contrib([v]) for v in views]
    assert all(s["hits"].sum() > 0 for s in singles)
    want = _fold(singles)
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0), (0, 1, 2)):
        got = dev.contrib([views[i] for i in order])
        for k in KEYS:
            assert np.array_equal(got[k], want[k]), (order, k)
    # ... and accumulated into the same arrays call by call
    acc = None
    for v in views:
        acc = dev.contrib([v], out=None if acc is None else acc["out"])
    for k in KEYS:
        assert np.array_equal(acc[k], want[k]), k


def test_two_segments_are_both_walked():
    d = helpers.two_segment_scene()
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v], seg1_fraction=0.5)
    assert int(v.flag.item()) == 0
    got = v.state()
    len1 = got["len1"]
    len2 = np.array([len(a) for a in got["lists"]]) - len1
    helpers.two_segment_populations(len1, len2)
    st, c, solid = _reference("two_segments", got, v.W, v.H)
    assert np.array_equal(got["n_contrib"][solid], st.n_contrib[solid])
    r = dev.contrib([v], [solid])
    check_against("two segments", r, contrib_ref.contributions(st, solid))
    for t in (0, 3, 4, 5):          # len1 on a word boundary, inside a word, segment 2 only, a list crossing a chunk
        seg2 = got["lists"][t][len1[t]:]
        assert len(seg2) > 0 and (r["hits"][seg2] > 0).all(), f"tile {t}: segment 2 was not walked"


def test_the_call_reads_the_forward_state_and_writes_only_its_outputs():
    d = helpers.blend_scene("cull", 72, 41)
    dev = Device(d)
    (v,) = dev.views([d])
    dev.forward_whole([v])
    before = [t.clone() for t in (v.geom, v.binning, v.img, v.color, v.depth, v.alpha, v.scratch, v.radii)]
    r = dev.contrib([v])
    assert r["hits"].sum() > 0
    for a, b in zip(before, (v.geom, v.binning, v.img, v.color, v.depth, v.alpha, v.scratch, v.radii)):
        assert torch.equal(a, b)
    # A blend backward after the call against one without it.  The backward adds its per-quadrant sums with float atomics, whose
    # order is free; pixel gradients that are zero outside ONE quadrant give every scratch row one nonzero term (x + 0 is exact
    # in any order), so equal inputs give equal bits.
    gc, gd, ga = helpers.blend_pixel_grads(v.W, v.H)
    keep = np.zeros((v.H, v.W), bool)
    keep[16:24, 24:32] = True
    grads = (gc * keep, gd * keep, ga * keep)
    (after,) = dev.blend_backward([v], [grads])
    (w,) = dev.views([d])
    dev.forward_whole([w])
    (without,) = dev.blend_backward([w], [grads])
    assert np.abs(without).sum() > 0 and np.array_equal(after.view(np.uint32), without.view(np.uint32))


def test_masks():
    dev, v, got, st, c, solid = run_case("cull", 96, 64)
    zero = dev.contrib([v], [np.zeros((v.H, v.W), np.uint8)])
    for k in KEYS:
        assert not zero[k].any(), k
    one_tile = np.zeros((v.H, v.W), bool)
    one_tile[16:32, 32:48] = True
    r = dev.contrib([v], [one_tile & solid])
    ref = contrib_ref.contributions(st, one_tile & solid)
    assert 0 < ref["hits"].sum() < c["hits"].sum()
    check_against("one tile", r, ref)
    a, b = dev.contrib([v]), dev.contrib([v], [np.full((v.H, v.W), 255, np.uint8)])
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
