"""tests/blend_ref.py pinned to independent references, the scenes of tests/test_gpu_blend_edges.py built through
oracle/tile_ref.c (with reference binning the device's lists and records are these), their populations and fragility caps
asserted, and the float32-against-float64 noise of the reference measured on exactly those scenes: the GPU bounds
(helpers.BLEND_*_BOUND) are 10 x the largest 99th percentile found here.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import blend_ref
import helpers
from helpers import BLEND_CASES, FRAGILE_MARGIN
from oracle import tile_ref


@functools.lru_cache(maxsize=None)
def _case(name, W, H):
    d = helpers.blend_scene(name, W, H)
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    return o, helpers.oracle_records(o), lists, blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)


def test_float64_forward_equals_the_tile_oracle_on_small_scene():
    d, _cam = helpers.small_scene()
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
    ok = st.margin >= FRAGILE_MARGIN
    assert ok.mean() > 0.97
    assert np.array_equal(st.n_contrib[ok], o.n_contrib[ok])
    assert np.abs(st.final_T - o.final_T)[ok].max() <= 1e-6
    for a, b in ((st.color, o.color), (st.depth, o.depth[0]), (st.alpha, o.alpha[0])):
        assert np.abs(a - b)[..., ok].max() <= 1e-6 * max(1.0, np.abs(b).max())


def _dense_rows(rec, order_tiles, W, H, bg, blended, gc, gd, ga):
    """float64 autograd of a dense per-pixel composite: every Gaussian of a tile's list against every pixel of the tile,
    membership (which entries a pixel blends) imposed from the reference forward, the 0.99 cap passed straight through."""
    R = torch.tensor(rec[:, :10], dtype=torch.float64, requires_grad=True)
    off = torch.zeros(len(rec), 2, dtype=torch.float64, requires_grad=True)
    gx = (W + 15) // 16
    loss = 0.0
    for t, ids in enumerate(order_tiles):
        if len(ids) == 0:
            continue
        px, py, inside, _q = blend_ref._tile_pixels(t, gx, W, H)
        r = R[torch.tensor(ids)]
        o = off[torch.tensor(ids)]
        dx = (r[:, 0:1] + o[:, 0:1]) - torch.tensor(px, dtype=torch.float64)
        dy = (r[:, 1:2] + o[:, 1:2]) - torch.tensor(py, dtype=torch.float64)
        power = -0.5 * (r[:, 2:3] * dx * dx + r[:, 4:5] * dy * dy) - r[:, 3:4] * dx * dy
        a_raw = r[:, 5:6] * torch.exp(power)
        alpha = a_raw + (torch.clamp(a_raw, max=0.99) - a_raw).detach()
        alpha = torch.where(torch.tensor(blended[t]), alpha, torch.zeros_like(alpha))
        Tin = torch.cumprod(1 - alpha, 0)
        Tex = torch.cat([torch.ones(1, 256, dtype=torch.float64), Tin[:-1]], 0)
        w = alpha * Tex
        m = torch.tensor(inside)
        cy, cx = np.minimum(py, H - 1), np.minimum(px, W - 1)
        for ch in range(3):
            img = (w * r[:, 6 + ch:7 + ch]).sum(0) + Tin[-1] * bg[ch]
            loss = loss + (img * torch.tensor(gc[ch][cy, cx], dtype=torch.float64))[m].sum()
        loss = loss + ((w * r[:, 9:10]).sum(0) * torch.tensor(gd[cy, cx], dtype=torch.float64))[m].sum()
        loss = loss + (w.sum(0) * torch.tensor(ga[cy, cx], dtype=torch.float64))[m].sum()
    loss.backward()
    g = R.grad.numpy()
    m2 = off.grad.numpy() * np.array([0.5 * W, 0.5 * H])
    # (the row's conic xy entry is -0.5 s dx dy like xx and yy -- the published backward's unit -- i.e. HALF the derivative
    # with respect to the off-diagonal entry, which appears twice in the quadratic form)
    return np.concatenate([g[:, 2:3], 0.5 * g[:, 3:4], g[:, 4:5], g[:, 9:10], m2, g[:, 6:9], g[:, 5:6]], 1)


def test_float64_backward_equals_autograd_of_a_dense_composite():
    d, _cam = helpers.small_scene(P=150, W=32, H=32, seed=3, scale_mu=0.12)
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    rec = helpers.oracle_records(o)
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    st = blend_ref.forward(rec, lists, 32, 32, o.bg)
    gc, gd, ga = helpers.blend_pixel_grads(32, 32)
    rows = blend_ref.backward(st, gc, gd, ga)
    want = _dense_rows(rec.astype(np.float64), lists, 32, 32, o.bg.astype(np.float64), st.blended, gc, gd, ga)
    touched = np.abs(want).sum(1) > 0
    assert touched.sum() > 50
    for c in range(10):
        assert np.linalg.norm(rows[:, c] - want[:, c]) <= 1e-9 * np.linalg.norm(want[:, c]), blend_ref.COLS[c]
    assert np.abs(rows - want).max() <= 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("name,W,H", BLEND_CASES)
def test_scene_populations_and_fragility_caps(name, W, H):
    o, rec, lists, st = _case(name, W, H)
    frag = st.margin < FRAGILE_MARGIN
    masks, lost, pr = blend_ref.strata(st, FRAGILE_MARGIN)
    pop, npairs = helpers.blend_populations(name, st, masks, lost, pr)
    print(f"{name} {o.W}x{o.H}: N={o.N} fragile pixels {frag.sum()} of {frag.size} ({100 * frag.mean():.3f} %), "
          f"strata (members, lost) {pop}, pairs {npairs}")
    assert frag.mean() <= 0.005
    # nothing disagrees with the tile oracle outside the fragile pixels
    assert np.array_equal(st.n_contrib[~frag], o.n_contrib[~frag])


def test_views_of_the_batch_scene_hold_their_populations_within_the_fragility_cap():
    for d in helpers.blend_batch_scenes():
        o = tile_ref.forward(**helpers.oracle_kwargs(d))
        lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
        st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
        frag = st.margin < FRAGILE_MARGIN
        fig = helpers.blend_batch_populations(st, blend_ref.pairs(st, FRAGILE_MARGIN), blend_ref.touched_rows(st, FRAGILE_MARGIN))
        print(f"batch view {o.W}x{o.H}: N={o.N}, fragile pixels {frag.sum()} of {frag.size}, {fig}")
        assert frag.mean() <= 0.005


def test_two_segment_scene_puts_len1_on_and_inside_a_mask_word():
    """The scene of the two-round GPU test through the oracle: segment 1 = the nearest 4096 Gaussians by view depth (the camera
    looks down +z from the origin); per tile, len1 = its list entries of segment 1."""
    d = helpers.two_segment_scene()
    assert d["means3D"].shape[0] == helpers.TWO_SEG_P
    o = tile_ref.forward(**helpers.oracle_kwargs(d))
    lists, _ = blend_ref.tile_lists(o.point_list, o.ranges)
    z = d["means3D"][:, 2].numpy()
    seg1 = np.zeros(o.P, bool)
    seg1[np.lexsort((np.arange(o.P), z))[:helpers.TWO_SEG_K1]] = True
    len1 = np.array([int(seg1[a].sum()) for a in lists])
    len2 = np.array([len(a) for a in lists]) - len1
    st = blend_ref.forward(helpers.oracle_records(o), lists, o.W, o.H, o.bg)
    frag = st.margin < FRAGILE_MARGIN
    print(f"two segments: N={o.N} len1 {len1.tolist()} len2 (one round) {len2.tolist()} fragile {frag.sum()} of {frag.size}")
    for t, (n1, n2) in helpers.TWO_SEG_TILES.items():
        assert (len1[t], len2[t]) == (n1, n2)
        assert all(seg1[lists[t][:n1]]) and not any(seg1[lists[t][n1:]]), "segment 1 comes first in every list"
    assert frag.mean() <= 0.005 and np.array_equal(st.n_contrib[~frag], o.n_contrib[~frag])
    # every pixel of the opaque tile terminates inside segment 1: a two-round forward must not give it a segment 2
    assert (st.sat_pos[:, 144:] >= 0).all() and st.sat_pos[:, 144:].max() < len1[9] and len2[9] > 0
    len2_two_round = np.where(np.arange(10) == 9, 0, len2)
    helpers.two_segment_populations(len1, len2_two_round)


def test_the_two_ladders_hold_every_saturation_position_next_to_a_seam():
    got = set()
    for name in ("ladder_b", "ladder_c"):
        st = _case(name, None, None)[3]
        got |= set(st.sat_pos[(st.sat_pos >= 0) & (st.margin >= FRAGILE_MARGIN)].tolist())
    assert set(range(62, 67)) | set(range(254, 259)) <= got, sorted(got)


def test_float32_noise_of_the_reference_pins_the_gpu_bounds():
    worst = dict(img=0.0, T=0.0, row=0.0)
    for name, W, H in BLEND_CASES:
        o, rec, lists, s64 = _case(name, W, H)
        s32 = blend_ref.forward(rec, lists, o.W, o.H, o.bg, dtype=np.float32)
        ok = s64.margin >= FRAGILE_MARGIN
        assert np.array_equal(s32.n_contrib[ok], s64.n_contrib[ok]), name
        gc, gd, ga = (g * ok for g in helpers.blend_pixel_grads(o.W, o.H))
        r64, r32 = blend_ref.backward(s64, gc, gd, ga), blend_ref.backward(s32, gc, gd, ga)
        touched = blend_ref.touched_rows(s64, FRAGILE_MARGIN)
        assert not r64[~touched].any() and not r32[~touched].any()
        e_row = helpers.row_err(r32, r64, touched)
        e_img = max(np.percentile((np.abs(a.astype(np.float64) - b) / (1 + np.abs(b)))[..., ok], 99)
                    for a, b in ((s32.color, s64.color), (s32.depth, s64.depth), (s32.alpha, s64.alpha)))
        e_T = np.percentile(np.abs(s32.final_T.astype(np.float64) - s64.final_T)[ok], 99)
        print(f"{name:9s} {o.W}x{o.H}: 99th percentile image {e_img:.2e}  final_T {e_T:.2e}  "
              f"row_err {np.percentile(e_row, 99):.2e} (max {e_row.max():.2e}, {len(e_row)} rows)")
        worst = dict(img=max(worst["img"], e_img), T=max(worst["T"], e_T), row=max(worst["row"], np.percentile(e_row, 99)))
    print("largest 99th percentiles:", {k: f"{v:.3e}" for k, v in worst.items()})
    # the bounds are 10 x these (rounded up by less than 10 %) -- except the image bound, which the measurement puts at
    # 3.3e-5 (stack513: 513 blended entries per pixel) and the existing contract caps at 3e-5
    assert 10 * worst["T"] <= helpers.BLEND_T_BOUND <= 11 * worst["T"]
    assert 10 * worst["row"] <= helpers.BLEND_ROW_BOUND <= 11 * worst["row"]
    assert helpers.BLEND_IMG_BOUND == min(helpers.BLEND_IMG_CONTRACT, helpers.BLEND_IMG_BOUND)
    assert 10 * worst["img"] >= helpers.BLEND_IMG_BOUND, "the contract no longer binds: take 10 x the measurement"
