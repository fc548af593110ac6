"""tests/segment_ref.py pinned to the references it is built on, on the scenes of tests/test_gpu_contrib.py (through
oracle/tile_ref.c; the States are those of tests/test_contrib_ref_cpu.py, computed once); the float32-against-float64 noise of
the winning per-pixel label sum measured on exactly those scenes under the three Gaussian labelings of the GPU test -- the GPU
bound segment_ref.LABEL_WEIGHT_BOUND is 10 x the largest 99th percentile found here, never taken from the kernel; the cap on
the pixels the GPU comparison leaves out; the two mutants; the pure-torch functions of binocular3dgs_amd/segment.py; and the
argument errors of the two entry points, which need no device.  No GPU.

Measured (99th percentile of the relative float32 error of the winning sum, per labeling mod16 / mod3_holes / single; then the
pixels left out -- fragile or a label margin below contrib_ref.TIE_THRESHOLD -- under the three labelings):
    stack1     1.3e-7 1.3e-7 1.3e-7   0 0 0      stack63    7.2e-7 9.6e-7 1.0e-6   0 0 0      stack64    7.2e-7 1.0e-6 1.1e-6   0 0 0
    stack65    9.3e-7 1.0e-6 1.1e-6   0 0 0      stack255   2.8e-6 3.0e-6 3.0e-6   0 0 0      stack256   2.8e-6 3.0e-6 3.1e-6   0 0 0
    stack257   2.9e-6 3.0e-6 3.1e-6   0 0 0      stack513   4.5e-6 4.6e-6 4.5e-6   0 2 0      ladder_b   2.4e-6 2.6e-6 2.5e-6   1 1 1
    cull 96x64 8.7e-7 8.6e-7 6.3e-7   8 7 7      cull 72x41 6.2e-7 5.5e-7 3.0e-7   8 5 5      cull 75x33 3.7e-7 4.3e-7 2.7e-7   13 12 12
    wide       2.0e-7 3.8e-7 6.2e-7   0 0 0
  largest: 4.618e-6 (stack513, mod3_holes)  ->  LABEL_WEIGHT_BOUND 4.7e-5.  Most left out: 13 of 2475 (0.525 %, cull 75x33).
mod3_holes leaves every seventh Gaussian unlabelled; on stack63, stack255, stack257 and ladder_b that labeling puts 126 to 322
of the 1024 pixels on a near-tie (segment_ref.SEVENTH_BREAKS_CAP says why), above the cap of 2 %, so those four scenes leave
every fifth Gaussian unlabelled instead (mod3_holes5; their figures above are of that labeling).  The cap is a condition on the
inputs: the labeling changed, the cap did not.
The floor next to the relative bound is one float32 ulp of 1 (segment_ref.LABEL_WEIGHT_FLOOR): a label sum is a part of the
pixel's alpha, at most 1, and each of its adds rounds by at most half an ulp of 1.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import blend_ref
import contrib_ref
import segment_ref
import test_contrib_ref_cpu
from helpers import FRAGILE_MARGIN

CASES = test_contrib_ref_cpu.CASES


@functools.lru_cache(maxsize=None)
def _render(name, W, H, labeling):
    st, _c = test_contrib_ref_cpu._case(name, W, H)
    gl, L = segment_ref.gaussian_labeling(labeling, np.asarray(st.records).shape[0])
    return st, gl, L, segment_ref.label_render(st, gl, L)


def test_votes_summed_over_the_labels_are_the_contribution_under_the_labelled_pixels():
    for (name, W, H), kind in ((("cull", 75, 33), "draw5"), (("stack65", None, None), "stripes"), (("wide", None, None), "checker")):
        st, c = test_contrib_ref_cpu._case(name, W, H)
        plane, L = segment_ref.label_plane(kind, st.W, st.H)
        v = segment_ref.votes(st, plane, L)
        assert v.shape == (np.asarray(st.records).shape[0], L) and v.dtype == np.int64 and v.sum() > 0
        assert np.array_equal(v.sum(1), contrib_ref.contributions(st, plane < L)["weight_q"])
        if kind != "draw5":
            assert np.array_equal(v.sum(1), c["weight_q"]), "every pixel carries a label: the votes are the whole contribution"
        else:
            assert (v.sum(1) <= c["weight_q"]).all() and (v.sum(1) < c["weight_q"]).any()
        assert (v > 0).any(0).all(), f"{name} / {kind}: a label without a vote"
    none = segment_ref.votes(st, np.full((st.H, st.W), 255, np.uint8), 16)
    assert not none.any()


def test_label_planes_and_labelings_are_what_the_gpu_test_says_they_are():
    for W, H in ((64, 16), (96, 64), (72, 41), (75, 33)):
        p, L = segment_ref.label_plane("checker", W, H)
        assert L == 2 and all(len(np.unique(p[y:y + 8, x:x + 8])) == 1 for y in range(0, H, 8) for x in range(0, W, 8)), "one label per quadrant"
        assert p[0, 0] != p[0, 8] and p[0, 0] != p[8, 0]
        p, L = segment_ref.label_plane("stripes", W, H)
        assert L == 2 and (p[:, 0::2] == 0).all() and (p[:, 1::2] == 1).all()
        p16, L16 = segment_ref.label_plane("draw16", W, H)
        p5, L5 = segment_ref.label_plane("draw5", W, H)
        assert (L16, L5) == (16, 5) and np.array_equal(p16, p5)
        assert set(np.unique(p16)) == set(range(16)) | {255}
        p, L = segment_ref.label_plane("constant", W, H)
        assert L == 1 and not p.any()
    gl, L = segment_ref.gaussian_labeling("mod3_holes", 100)
    assert L == 3 and (gl[6::7] == 255).all() and set(np.unique(gl)) == {0, 1, 2, 255}


@pytest.mark.parametrize("name,W,H", CASES)
def test_label_sums_agree_with_the_blend_reference(name, W, H):
    for labeling in segment_ref.labelings_for(name):
        st, gl, L, r = _render(name, W, H, labeling)
        assert r["sums"].shape == (L, st.H, st.W) and (r["sums"] >= 0).all()
        labelled = r["sums"].sum(0)
        if labeling.startswith("mod3_holes"):
            assert (labelled <= st.alpha * (1 + 1e-12)).all()
        else:   # every Gaussian carries a label: the sums add up to the alpha image
            assert (np.abs(labelled - st.alpha) <= 1e-12).all()
        assert np.array_equal(r["weight"], r["sums"].max(0))
        assert np.array_equal(r["label"] != 255, r["weight"] > 0) and (r["label"][r["weight"] > 0] < L).all()
        assert (r["label"][st.n_contrib == 0] == 255).all()
        if labeling == "single":
            assert np.array_equal(r["label"] == 0, st.n_contrib > 0) and np.isinf(r["margin"]).all()
        solid = segment_ref.solid_mask(st, r, FRAGILE_MARGIN)
        assert np.array_equal(r["label32"][solid], r["label"][solid]), "the float32 restatement picks the same label off the near-ties"


def test_float32_noise_pins_the_gpu_bound_and_the_left_out_share_stays_under_its_cap():
    worst = 0.0
    for name, W, H in CASES:
        figs, left = [], []
        for labeling in segment_ref.labelings_for(name):
            st, gl, L, r = _render(name, W, H, labeling)
            figs.append(segment_ref.noise(r))
            out = ~segment_ref.solid_mask(st, r, FRAGILE_MARGIN)
            left.append(int(out.sum()))
            assert out.mean() <= contrib_ref.MASKED_CAP, f"{name} / {labeling}: {out.sum()} of {out.size} pixels left out"
        print(f"{name:9s} {st.W}x{st.H}: 99th percentile of the winning sum " + " ".join(f"{f:.1e}" for f in figs)
              + "   left out " + " ".join(str(n) for n in left) + f" of {st.W * st.H}")
        worst = max(worst, max(figs))
    print("largest 99th percentile: %.3e" % worst)
    assert 10 * worst <= segment_ref.LABEL_WEIGHT_BOUND <= 11 * worst
    assert segment_ref.LABEL_WEIGHT_FLOOR == 2.0 ** -23 and contrib_ref.MASKED_CAP == 0.02


def test_every_seventh_unlabelled_breaks_the_cap_exactly_where_every_fifth_stands_in():
    for name, W, H in CASES:
        st, gl, L, r = _render(name, W, H, "mod3_holes")
        breaks = (~segment_ref.solid_mask(st, r, FRAGILE_MARGIN)).mean() > contrib_ref.MASKED_CAP
        assert breaks == (name in segment_ref.SEVENTH_BREAKS_CAP), name
        assert ("mod3_holes5" in segment_ref.labelings_for(name)) == breaks


def test_the_vote_planes_of_the_anchor_keep_their_labelled_pixels_solid():
    """The float64 anchor of the GPU test: `cull` at 96x64, labels 255 outside contrib_ref.solid_mask."""
    st, c = test_contrib_ref_cpu._case("cull", 96, 64)
    solid = contrib_ref.solid_mask(st, c, FRAGILE_MARGIN)
    assert (~solid).mean() <= contrib_ref.MASKED_CAP
    plane, L = segment_ref.label_plane("draw5", st.W, st.H)
    plane = np.where(solid, plane, 255).astype(np.uint8)
    v = segment_ref.votes(st, plane, L)
    assert (v > 0).any(0).all()


def test_mutant_ties_to_the_highest_label_is_caught():
    S = np.array([[0.5, 0.0, 0.2, 0.0], [0.5, 0.0, 0.3, 0.25], [0.1, 0.0, 0.3, 0.25]])
    lab, wgt = segment_ref.pick(S)
    assert lab.tolist() == [0, 255, 1, 1] and wgt.tolist() == [0.5, 0.0, 0.3, 0.25]
    bad, _ = segment_ref.pick(S, "ties_high")
    assert bad.tolist() == [1, 255, 2, 2]
    # through the walk: two entries whose float32 weights tie exactly at one pixel
    rec, lists = segment_ref.tie_records()
    st = blend_ref.forward(rec, lists, 16, 16, (0.0, 0.0, 0.0))
    assert st.blended[0][:, 3 * 16 + 3].all()
    r = segment_ref.label_render(st, np.array([1, 0], np.uint8), 2)
    m = segment_ref.label_render(st, np.array([1, 0], np.uint8), 2, mutant="ties_high")
    assert r["weight32"][3, 3] == 0.25 and r["label32"][3, 3] == 0 and m["label32"][3, 3] == 1
    assert r["label"][3, 3] == 0 and 0 < r["margin"][3, 3] < contrib_ref.TIE_THRESHOLD, "in float64 a near-tie: the GPU test leaves it out"
    assert not np.array_equal(r["label32"], m["label32"])


@pytest.mark.parametrize("name,W,H", [("cull", 75, 33), ("stack65", None, None)])
def test_mutant_unlabelled_counted_as_label_0_is_caught(name, W, H):
    st, gl, L, r = _render(name, W, H, "mod3_holes")
    m = segment_ref.label_render(st, gl, L, mutant="unlabelled_as_0")
    solid = segment_ref.solid_mask(st, r, FRAGILE_MARGIN)
    differ = solid & ((m["label"] != r["label"]) | (np.abs(m["weight"] - r["weight"]) >
                                                     segment_ref.LABEL_WEIGHT_BOUND * r["weight"] + segment_ref.LABEL_WEIGHT_FLOOR))
    assert differ.sum() >= 10, "the comparison of the GPU test tells the mutant from the reference"


# ---- binocular3dgs_amd/segment.py: the pure-torch functions -------------------------------------------------------------
def test_assign_labels():
    from binocular3dgs_amd import segment
    q = 1 << 32
    votes = torch.tensor([[3 * q, 3 * q, q],      # tie of 0 and 1 -> the lowest
                          [0, 5 * q, 5 * q],      # tie of 1 and 2
                          [0, 0, 0],              # nothing -> 255
                          [q, 2 * q, 7 * q],
                          [6 * q, q, 3 * q]], dtype=torch.int64)
    got = segment.assign_labels(votes)
    assert got.dtype == torch.uint8 and got.tolist() == [0, 1, 255, 2, 0]
    # many equal maxima: always the first, whatever torch.argmax would return
    assert segment.assign_labels(torch.full((64, 16), q, dtype=torch.int64)).tolist() == [0] * 64
    assert segment.assign_labels(votes, gain=[1.0, 1.0, 4.0]).tolist() == [2, 2, 255, 2, 2]
    assert segment.assign_labels(votes, gain=[1.0, 1.0, 2.0]).tolist() == [0, 2, 255, 2, 0], "6 against 2 * 3: a tie, to the lowest"
    assert segment.assign_labels(votes, min_weight=7.0).tolist() == [255, 1, 255, 2, 0], "total <= min_weight: unassigned"
    assert segment.assign_labels(votes, min_share=0.6).tolist() == [255, 255, 255, 2, 0], "shares 3/7, 1/2, -, 0.7, 0.6"
    assert segment.assign_labels(votes, min_share=0.61).tolist() == [255, 255, 255, 2, 255]
    assert segment.assign_labels(torch.zeros((0, 3), dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError):
        segment.assign_labels(votes, gain=[1.0, 2.0])
    with pytest.raises(ValueError):
        segment.assign_labels(torch.zeros((4, 17), dtype=torch.int64))


def test_label_iou_and_colours():
    from binocular3dgs_amd import segment
    given = torch.tensor([[0, 0, 1, 1], [2, 2, 255, 255], [0, 1, 7, 1]], dtype=torch.uint8)
    rend = torch.tensor([[0, 1, 1, 1], [2, 255, 0, 1], [0, 1, 2, 255]], dtype=torch.uint8)
    got = segment.label_iou(rend, given, 3)
    assert got.dtype == torch.int64 and got.tolist() == [[2, 3], [3, 5], [1, 2]], "bytes >= 3 of `given` (255 and 7) are ignored"
    assert segment.label_iou(given, given, 3).tolist() == [[3, 3], [4, 4], [2, 2]]
    with pytest.raises(ValueError):
        segment.label_iou(rend, given, 17)
    col = segment.label_colours(given)
    assert col.shape == (3, 4, 3) and col.dtype == torch.uint8
    assert col[1, 2].tolist() == [0, 0, 0] and col[0, 0].tolist() == list(segment.PALETTE[0]) and col[2, 2].tolist() == list(segment.PALETTE[7])
    assert len(set(segment.PALETTE)) == 16


def _png(W, H, ctype, rows, extra=b""):
    """An 8-bit PNG of colour type `ctype` from raw rows (filter byte 0 prepended here)."""
    import struct
    import zlib

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    raw = b"".join(b"\x00" + bytes(r) for r in rows)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)) + extra
            + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_read_labels(tmp_path):
    import struct
    import zlib
    from binocular3dgs_amd import frames, segment
    plane = np.array([[0, 1, 2, 255, 4], [5, 5, 0, 15, 1], [2, 2, 2, 255, 255]], np.uint8)
    np.save(tmp_path / "a.npy", plane)
    got = segment.read_labels(str(tmp_path / "a.npy"))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), plane)
    np.save(tmp_path / "b.npy", plane.astype(np.int64))
    assert np.array_equal(segment.read_labels(str(tmp_path / "b.npy")).numpy(), plane)
    np.save(tmp_path / "bad.npy", plane.astype(np.float32))
    with pytest.raises(ValueError):
        segment.read_labels(str(tmp_path / "bad.npy"))
    (tmp_path / "gray.png").write_bytes(_png(5, 3, 0, plane))
    assert np.array_equal(segment.read_labels(str(tmp_path / "gray.png")).numpy(), plane)
    # a palette PNG: the indices are the labels; frames.read_png itself still refuses the file
    plte = bytes(range(256)) * 3
    body = b"PLTE" + plte
    extra = struct.pack(">I", len(plte)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
    (tmp_path / "pal.png").write_bytes(_png(5, 3, 3, plane, extra))
    assert np.array_equal(segment.read_labels(str(tmp_path / "pal.png")).numpy(), plane)
    with pytest.raises(ValueError):
        frames.read_png(str(tmp_path / "pal.png"))
    # frames.write_png writes RGB: label_colours pictures are not label planes ...
    frames.write_png(str(tmp_path / "rgb.png"), segment.label_colours(torch.from_numpy(plane)))
    with pytest.raises(ValueError, match="3 channels"):
        segment.read_labels(str(tmp_path / "rgb.png"))
    # ... but the picture round-trips through read_png, and the palette leads back to the labels
    back = frames.read_png(str(tmp_path / "rgb.png"))
    assert np.array_equal(back, segment.label_colours(torch.from_numpy(plane)).numpy())
    pal = np.array(segment.PALETTE + ((0, 0, 0),), np.uint8)
    idx = (back[:, :, None, :] == pal[None, None]).all(-1).argmax(-1)
    assert np.array_equal(np.where(idx == 16, 255, idx), plane)


# ---- the two entry points: argument errors need no device ---------------------------------------------------------------
def test_argument_errors_of_the_entry_points_need_no_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    sc = _lib.B3gsScene()
    sc.P, sc.W, sc.H = 10, 32, 16
    buf = (C.c_uint8 * 64)()                      # host bytes: never read, the calls must fail before any HIP call
    p = C.addressof(buf)
    other = _lib.B3gsScene()
    other.P, other.W, other.H = 11, 32, 16
    empty = _lib.B3gsScene()
    empty.P, empty.W, empty.H = 0, 32, 16
    for fn, View, tail, name in ((L.b3gs_label_votes_batch, _lib.B3gsLabelVoteView, (p,), b"b3gs_label_votes_batch"),
                                 (L.b3gs_label_render_batch, _lib.B3gsLabelRenderView, (p, p), b"b3gs_label_render_batch")):
        view = View(C.pointer(sc), p, p, p, *tail)
        views = (View * 9)(*([view] * 9))
        for n in (0, 9, -1):
            assert fn(n, views, 2, p, None) == -1 and b"1..8 views" in L.b3gs_last_error()
        for nl in (0, 17, -3):
            assert fn(1, views, nl, p, None) == -1 and b"1..16 labels" in L.b3gs_last_error()
        assert fn(1, None, 2, p, None) == -1 and b"NULL view table" in L.b3gs_last_error()
        assert fn(1, views, 2, None, None) == -1 and b"NULL" in L.b3gs_last_error()      # votes_q32 / gaussian_label
        for k in ("geometry", "binning", "image"):
            v = (View * 1)(View(C.pointer(sc), p, p, p, *tail))
            setattr(v[0], k, None)
            assert fn(1, v, 2, p, None) == -1 and b"NULL state buffer" in L.b3gs_last_error()
        for k in [f[0] for f in View._fields_[4:]]:                                          # labels | label, weight
            v = (View * 1)(View(C.pointer(sc), p, p, p, *tail))
            setattr(v[0], k, None)
            assert fn(1, v, 2, p, None) == -1 and (b"NULL label plane" in L.b3gs_last_error() or b"NULL output plane" in L.b3gs_last_error())
        v = (View * 1)(View(None, p, p, p, *tail))
        assert fn(1, v, 2, p, None) == -1 and b"B3gsScene" in L.b3gs_last_error()
        for W, H in ((0, 16), (32, 0), (-1, 16)):
            z = _lib.B3gsScene()
            z.P, z.W, z.H = 10, W, H
            v = (View * 1)(View(C.pointer(z), p, p, p, *tail))
            assert fn(1, v, 2, p, None) == -1 and b"W/H" in L.b3gs_last_error()
        v = (View * 2)(view, View(C.pointer(other), p, p, p, *tail))
        assert fn(2, v, 2, p, None) == -1 and b"share P" in L.b3gs_last_error()
        v = (View * 1)(View(C.pointer(empty), p, p, p, *tail))
        assert fn(1, v, 2, p, None) == 0, "P == 0: nothing to do, and no HIP call"
        with pytest.raises(_lib.B3gsError, match=name.decode() + " failed: B3GS_ERR_ARG"):
            _lib.check(fn(0, views, 2, p, None), name.decode())
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "b3gs_raster.h")).read()
    assert "#define B3GS_MAX_LABELS 16" in header and _lib.ABI_VERSION == 18


def test_the_compiled_module_refuses_host_tensors_and_wrong_shapes():
    from binocular3dgs_amd import _C, _lib
    u8 = torch.zeros(64, dtype=torch.uint8)
    plane = torch.zeros(16, 16, dtype=torch.uint8)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.label_votes([(u8, u8, u8, 16, 16, plane)], 2, torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.label_render([(u8, u8, u8, 16, 16, plane, torch.zeros(16, 16))], 2, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        _C.label_votes([], 2, torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        _C.label_votes([(u8, u8, u8, 16, 16, plane)], 17, torch.zeros(4, 17, dtype=torch.int64))
    with pytest.raises(ValueError):
        _C.label_render([], 2, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):
        _C.label_render([(u8, u8, u8, 16, 16, plane, torch.zeros(16, 16))], 0, torch.zeros(4, dtype=torch.uint8))
