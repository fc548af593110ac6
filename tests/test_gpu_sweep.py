"""The plane-sweep matcher on the device (csrc/sweep.hip, binocular3dgs_amd/sweep_matcher.py) against its yardstick, the float64
restatement of tests/sweep_ref.py, on golden G16 (tests/golden/sweep.npz) and on small shapes restated at test time.  Decisions
(validity, k*, kept matches and their order) are equal except at the near-tie nodes the yardstick itself names (at most 2 %);
scores lie within 4 err32, err32 being the float32 restatement's own distance from the float64 one."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_ref as sr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "sweep.npz"))


def _params(p: sr.Params):
    from binocular3dgs_amd.sweep_matcher import SweepParams
    return SweepParams(stride=p.stride, hypotheses=p.hypotheses, min_score=p.min_score, margin=p.margin, min_var=p.min_var,
                       cyc_steps=p.cyc_steps)


def _launch(img_a, img_b, K, c2w_a, c2w_b, near, far, p: sr.Params):
    """the raw outputs of one pair call as numpy arrays"""
    from binocular3dgs_amd import sweep_matcher as sm
    plan = sm.pair_plan(K, c2w_a, c2w_b, near, far, p.hypotheses)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    out = sm.launch_pair(up(img_a), up(img_b), up(plan.homographies), up(plan.proj), plan, near, far, _params(p))
    return [t.cpu().numpy() for t in out]


def _compare(out, want, d, W, H, p, err32, what):
    """direction d of a pair call against the yardstick's dict (has, k, best, lcr, refined, invd, keep, q, near_tie, any_valid, step)"""
    kp_s, kp_t, score, count, node_invd, node_score, node_k = out
    tie = want["near_tie"]
    share = tie.mean()
    print(f"{what}: near-tie nodes {tie.sum()} of {len(tie)}")
    ok = ~tie
    has = node_invd[d] != sr.NONE
    assert np.array_equal(has[ok], want["has"][ok]), what
    anyv = want["any_valid"]
    assert np.array_equal((node_k[d] >= 0)[ok & want["textured"]], anyv[ok & want["textured"]]), what
    sel = ok & anyv & want["textured"]
    assert np.array_equal(node_k[d][sel], want["k"][sel]), what
    ds = np.abs(node_score[d][sel] - want["best"][sel])
    print(f"{what}: largest |score - yardstick| = {ds.max() if len(ds) else 0.0:.3g} (bound {4 * err32:.3g})")
    assert (ds <= 4 * err32).all(), what
    # the refined inverse depth: the change 4 err32 in each of the three scores can cause in the parabola's vertex, plus the
    # float32 rounding of the final sum
    hs = ok & want["has"]
    l, c, r = want["lcr"]
    e = 4 * err32
    ref = hs & want["refined"]
    with np.errstate(invalid="ignore", divide="ignore"):
        # vertex = 0.5 (l - r) / den, den = l - 2 c + r: scores off by e move the numerator by <= e and den by <= 4 e
        den = np.abs((l - 2 * c) + r)
        vertex = np.abs(0.5 * (l - r)) / den
        dv = np.where(ref, (e + vertex * 4 * e) / np.maximum(den - 4 * e, 1e-30), 0.0)
    bound = 4e-7 * np.maximum(np.abs(want["invd"]), 1.0) + dv * want["step"]
    di = np.abs(node_invd[d] - want["invd"])
    print(f"{what}: largest |invd - yardstick| / bound = {(di[hs] / bound[hs]).max() if hs.any() else 0.0:.3g}")
    assert (di[hs] <= bound[hs]).all(), what
    # kept matches and their order
    xs, ys = sr.node_axes(W, H, p.stride)
    nx = len(xs)
    n = int(count[d])
    node_of = ((kp_s[d][:n, 1] - sr.R) / p.stride).astype(np.int64) * nx + ((kp_s[d][:n, 0] - sr.R) / p.stride).astype(np.int64)
    assert (np.diff(node_of) > 0).all(), what                                     # node order, no duplicates
    kept = np.zeros(len(tie), bool)
    kept[node_of] = True
    assert np.array_equal(kept[ok], want["keep"][ok]), what
    both = kept & want["keep"] & ok
    assert np.array_equal(node_of[both[node_of]], np.flatnonzero(both)), what
    dq = np.abs(kp_t[d][:n][both[node_of]] - want["q"][both])
    print(f"{what}: kept {n}, largest |kp_target - yardstick| = {dq.max() if len(dq) else 0.0:.3g} px")
    assert (dq <= 1e-3).all(), what
    assert np.array_equal(score[d][:n], node_score[d][node_of]), what
    return share, n, kept


def _gold_dir(g, x, y):
    tag = f"dir/{x}_{y}/"
    w = {k: g[tag + k] for k in ("has", "k", "best", "lcr", "refined", "invd", "keep", "q", "near_tie", "any_valid", "step", "true_q")}
    w["textured"] = np.ones(len(w["has"]), bool)                                  # (re-derived below for shapes restated at test time)
    return w


def _textured(img, stride, min_var):
    gr = sr.gray(img).astype(np.float64)
    xs, ys = sr.node_axes(img.shape[1], img.shape[0], stride)
    X, Y = np.meshgrid(xs, ys)
    a = np.stack([gr[Y.ravel() + dy, X.ravel() + dx] for dy, dx in sr.TAPS])
    return a.var(axis=0) >= min_var


def test_parity_and_truth_on_the_stored_scene(g):
    """1 and 2 of the issue: decisions equal the float64 yardstick's outside its near-tie list, scores within 4 err32; the kernel's
    matches are as true as the yardstick's (share within 1 px not below its share minus one point, count at least 98 %)"""
    p = sr.Params(stride=int(g["stride"]), hypotheses=int(g["hypotheses"]))
    imgs, K, c2ws, err32 = g["images"], g["K"], g["c2ws"], float(g["err32"])
    H, W = imgs.shape[1:3]
    ties = nodes = n_kernel = n_ref = good_kernel = good_ref = 0
    for a, b in g["pairs"].tolist():
        out = _launch(imgs[a], imgs[b], K, c2ws[a], c2ws[b], float(g["near"]), float(g["far"]), p)
        for d, (x, y) in enumerate(((a, b), (b, a))):
            want = _gold_dir(g, x, y)
            want["textured"] = _textured(imgs[x], p.stride, p.min_var)
            _, n, kept = _compare(out, want, d, W, H, p, err32, f"{x}->{y}")
            ties, nodes = ties + int(want["near_tie"].sum()), nodes + len(kept)
            q = np.full((len(kept), 2), np.nan)
            q[kept] = out[1][d][:n]
            n_kernel, n_ref = n_kernel + n, n_ref + int(want["keep"].sum())
            good_kernel += int((np.linalg.norm(q - want["true_q"], axis=1)[kept] <= 1.0).sum())
            good_ref += int((np.linalg.norm(want["q"] - want["true_q"], axis=1)[want["keep"]] <= 1.0).sum())
    print(f"near-tie share {ties / nodes:.4f}; within 1 px: kernel {good_kernel}/{n_kernel}, yardstick {good_ref}/{n_ref}")
    assert ties <= 0.02 * nodes
    assert good_kernel / n_kernel >= good_ref / n_ref - 0.01
    assert n_kernel >= 0.98 * n_ref


def _restated(sc, imgs, a, b, p):
    args = (imgs[a], imgs[b], sc.K, sr.w2c(sc, a), sr.w2c(sc, b), sc.near, sc.far, p)
    r64, r32 = sr.match_pair(*args, T=np.float64), sr.match_pair(*args, T=np.float32)
    err32, wants = 0.0, []
    for d in range(2):
        both = r64.vols[d].valid & r32.vols[d].valid
        if both.any():
            err32 = max(err32, float(np.abs(r64.vols[d].scores - r32.vols[d].scores)[both].max()))
        sel, dr = r64.sel[d], r64.dirs[d]
        x = (a, b)[d]
        wants.append({"has": sel.has, "k": sel.k, "best": sel.best, "lcr": sel.lcr, "refined": sel.refined, "invd": sel.invd, "keep": dr.keep,
                      "q": dr.q, "near_tie": dr.fragile, "any_valid": r64.vols[d].valid.any(axis=0),
                      "step": float(sr.plan(sc.K, sr.w2c(sc, a), sr.w2c(sc, b), sc.near, sc.far, p.hypotheses).step),
                      "textured": _textured(imgs[x], p.stride, p.min_var)})
    return wants, err32


SHAPES = [(50, 37, 1, 16), (50, 37, 2, 16), (50, 37, 3, 16), (50, 37, 2, 2), (50, 37, 2, 3), (7, 7, 2, 8)]


@pytest.mark.parametrize("W,H,stride,D", SHAPES)
def test_shapes_where_indexing_can_go_wrong(W, H, stride, D):
    """3 of the issue: node counts that are no multiple of a block, the last node on W - 4 or one short of it, D = 2 and 3 (no or
    barely a parabola), an image of exactly one node -- each against the yardstick restated here"""
    sc = sr.make_scene(W=W, H=H, baseline=0.6 * W / 96.0 if W > 7 else 0.05)
    imgs = [sr.render(sc, v) for v in range(2)]
    p = sr.Params(stride=stride, hypotheses=D)
    xs, ys = sr.node_axes(W, H, stride)
    assert xs[-1] in (W - 4, W - 5, W - 6) and (len(xs) * len(ys)) % 64 != 0
    wants, err32 = _restated(sc, imgs, 0, 1, p)
    out = _launch(imgs[0], imgs[1], sc.K, sc.c2ws[0], sc.c2ws[1], sc.near, sc.far, p)
    assert out[0].shape == (2, len(xs) * len(ys), 2)
    ties = 0
    for d in range(2):
        ties += _compare(out, wants[d], d, W, H, p, err32, f"{W}x{H} stride {stride} D {D} dir {d}")[0]
    if W > 7:
        assert ties / 2 <= 0.02


def test_kept_matches_across_the_seam_of_the_block_scan():
    """520 x 520 at stride 1: 514 x 514 = 264 196 nodes per direction, 1033 compaction blocks of 256 -- two steps of the 1024-wide
    scan of the block counts, in both directions (rows of nb + 1 words).  D = 2, the fewest hypotheses the call takes.  Compared
    as the shapes above are, with the same allowance for ties."""
    W = H = 520
    sc = sr.make_scene(W=W, H=H, baseline=0.1 * W / 96.0)      # a short baseline: both views keep matches in their last rows
    imgs = [sr.render(sc, v) for v in range(2)]
    p = sr.Params(stride=1, hypotheses=2)
    xs, ys = sr.node_axes(W, H, 1)
    assert len(xs) * len(ys) == 264196 and (len(xs) * len(ys) + 255) // 256 == 1033
    wants, err32 = _restated(sc, imgs, 0, 1, p)
    out = _launch(imgs[0], imgs[1], sc.K, sc.c2ws[0], sc.c2ws[1], sc.near, sc.far, p)
    assert out[0].shape == (2, len(xs) * len(ys), 2)
    ties = 0
    for d in range(2):
        share, n, kept = _compare(out, wants[d], d, W, H, p, err32, f"{W}x{H} stride 1 D 2 dir {d}")
        ties += share
        assert wants[d]["keep"][:1024 * 256].any() and wants[d]["keep"][1024 * 256:].any()    # the yardstick keeps nodes on both
        assert 0 < n < len(kept) and kept[:1024 * 256].any() and kept[1024 * 256:].any()      # sides of the seam, and so does the kernel
    assert ties / 2 <= 0.02


def test_a_pair_that_looks_away_has_no_matches():
    from binocular3dgs_amd import sweep_matcher as sm
    sc = sr.make_scene(W=50, H=37)
    img = torch.from_numpy(sr.render(sc, 0)).to(DEV)
    away = sc.c2ws[1].copy()
    away[:3, :3] = away[:3, :3] @ np.diag([-1.0, 1.0, -1.0])                      # turned by half a circle about its y axis
    (ka, kab, sa), (kb, kba, sb) = sm.match_pair(img, img, sc.K, sc.c2ws[0], away, sc.near, sc.far, _params(sr.Params(hypotheses=16)))
    for t in (ka, kab, kb, kba):
        assert tuple(t.shape) == (0, 2) and t.dtype == torch.float32
    assert tuple(sa.shape) == (0,) and tuple(sb.shape) == (0,)


def test_both_directions_and_determinism(g):
    """4 of the issue: a -> b of the pair call equals the other half of the call with the views swapped; two runs give the same bytes"""
    p = sr.Params(stride=2, hypotheses=int(g["hypotheses"]))
    imgs, K, c2ws = g["images"], g["K"], g["c2ws"]
    near, far = float(g["near"]), float(g["far"])
    ab = _launch(imgs[0], imgs[2], K, c2ws[0], c2ws[2], near, far, p)
    ba = _launch(imgs[2], imgs[0], K, c2ws[2], c2ws[0], near, far, p)
    again = _launch(imgs[0], imgs[2], K, c2ws[0], c2ws[2], near, far, p)
    for d in range(2):
        n = int(ab[3][d])
        assert n == int(ba[3][1 - d]) and n > 0
        for i in (0, 1, 2):
            assert ab[i][d][:n].tobytes() == ba[i][1 - d][:n].tobytes()
            assert ab[i][d][:n].tobytes() == again[i][d][:n].tobytes()
        for i in (4, 5, 6):
            assert ab[i][d].tobytes() == ba[i][1 - d].tobytes() == again[i][d].tobytes()


def test_the_pair_call_is_captured_in_a_graph(g):
    """5 of the issue: no host read inside the call -- one capture, replayed on a second image pair copied into the static inputs"""
    from binocular3dgs_amd import sweep_matcher as sm
    p = sr.Params(stride=2, hypotheses=int(g["hypotheses"]))
    imgs, K, c2ws = g["images"], g["K"], g["c2ws"]
    near, far = float(g["near"]), float(g["far"])
    plan = sm.pair_plan(K, c2ws[0], c2ws[1], near, far, p.hypotheses)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    sa, sb, hs, pj = up(imgs[0]), up(imgs[1]), up(plan.homographies), up(plan.proj)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sm.launch_pair(sa, sb, hs, pj, plan, near, far, _params(p))               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = sm.launch_pair(sa, sb, hs, pj, plan, near, far, _params(p))
    # the second pair: the same cameras, the images of another seed
    sc2 = sr.make_scene(seed=11)
    other = [sr.render(sc2, v) for v in range(2)]
    eager = sm.launch_pair(up(other[0]), up(other[1]), hs, pj, plan, near, far, _params(p))
    sa.copy_(up(other[0]))
    sb.copy_(up(other[1]))
    graph.replay()
    torch.cuda.synchronize()
    n = eager[3].tolist()
    assert static_out[3].tolist() == n and min(n) > 0
    for d in range(2):
        for i in (0, 1, 2):
            assert torch.equal(static_out[i][d, :n[d]], eager[i][d, :n[d]])
    for i in (4, 5, 6):
        assert torch.equal(static_out[i], eager[i])
    assert not np.array_equal(other[0], imgs[0])


def _write_colmap_folder(root, sc, images, points):
    from binocular3dgs_amd.frames import write_png
    os.makedirs(os.path.join(root, "sparse/0"))
    os.makedirs(os.path.join(root, "images"))
    with open(os.path.join(root, "sparse/0/cameras.txt"), "w") as fp:
        fp.write(f"1 PINHOLE {sc.W} {sc.H} {float(sc.K[0, 0])!r} {float(sc.K[1, 1])!r} {float(sc.K[0, 2])!r} {float(sc.K[1, 2])!r}\n")
    with open(os.path.join(root, "sparse/0/images.txt"), "w") as fp:
        for v, img in enumerate(images):
            m = sr.w2c(sc, v)
            q = _quaternion(m[:3, :3])
            fp.write(f"{v + 1} {' '.join(repr(float(x)) for x in q)} {' '.join(repr(float(x)) for x in m[:3, 3])} 1 view_{v:02d}.png\n\n")
            write_png(os.path.join(root, "images", f"view_{v:02d}.png"), img)
    with open(os.path.join(root, "sparse/0/points3D.txt"), "w") as fp:
        for i, xyz in enumerate(points):
            fp.write(f"{i + 1} {' '.join(repr(float(x)) for x in xyz)} 128 128 128 0.5\n")


def _quaternion(Rm):
    w = np.sqrt(max(0.0, 1.0 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])) / 2.0
    return np.array([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)])


def test_end_to_end_from_a_folder(tmp_path):
    """6 of the issue: the synthetic scene as a COLMAP text folder -> build_cloud(matcher="sweep") at the default parameters; the
    cloud lies on the true surfaces; the CLI writes a PLY and a match file that the file path turns into the same cloud.  The
    rig is the generator's long-baseline form (cameras turned towards the scene), so that at the default D = 128 a hypothesis
    step is about half a pixel, as it is in the stored scene at D = 32."""
    from binocular3dgs_amd import keypoints_to_3d, matcher_cloud as mc
    from binocular3dgs_amd.init_points import fetch_point_cloud
    sc = sr.make_scene(baseline=2.4, toe_in=True, n_views=4)
    images = [sr.render(sc, v) for v in range(4)]
    vv, uu = np.meshgrid(np.arange(4.0, sc.H, 8.0), np.arange(4.0, sc.W, 8.0), indexing="ij")
    pts = np.concatenate([sr.cast(sc, v, uu.ravel(), vv.ravel())[0] for v in range(3)])
    folder = str(tmp_path / "scene")
    _write_colmap_folder(folder, sc, images, pts)
    views = mc.read_views(folder, 1)
    assert mc.select_views(len(views.names), "LLFF", 3) == [0, 1, 2]
    from binocular3dgs_amd import sweep_matcher as sm
    near, far = sm.depth_range(folder, views, [0, 1, 2])
    step = (1.0 / near - 1.0 / far) / 127
    xyz, rgb = mc.build_cloud(folder, matcher="sweep", dataset_name="LLFF", n_views=3, resolution=1, iterations=0)
    assert len(xyz) > 100 and rgb.shape == xyz.shape
    # every point against the true surface along the ray of the view it was matched in (the view whose node it projects onto)
    err = np.full(len(xyz), np.inf)
    for v in range(3):
        m = sr.w2c(sc, v)
        cam = xyz.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        u, w = sc.K[0, 0] * cam[:, 0] / cam[:, 2] + sc.K[0, 2], sc.K[1, 1] * cam[:, 1] / cam[:, 2] + sc.K[1, 2]
        on_node = (np.abs(u - np.rint(u)) < 2e-2) & (np.abs(w - np.rint(w)) < 2e-2) & (cam[:, 2] > 0)
        z_true = sr.cast(sc, v, np.rint(u), np.rint(w))[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.abs(1.0 / cam[:, 2] - 1.0 / z_true) / step                     # in hypothesis steps at that depth
        err = np.where(on_node, np.minimum(err, e), err)
    share = float((err >= 1.0).mean())
    print(f"end to end: {len(xyz)} points, {share:.4f} of them a hypothesis step or more from the true surface")
    assert share <= 0.05
    # the CLI: a PLY that the initial-points reader reads, a match file that the file path turns into the same cloud
    f = str(tmp_path / "m.npz")
    out_dir = str(tmp_path / "keypoints_to_3d" / "LLFF")
    assert keypoints_to_3d.main(["--data_path", folder, "--matcher", "sweep", "--save_matches", f, "--resolution", "1", "--iterations", "0",
                                 "--output_path", out_dir]) == 0
    got = fetch_point_cloud(os.path.join(out_dir, "scene_keypoints_to_3d.ply"))
    assert np.array_equal(got[0], xyz) and np.array_equal(got[1], rgb.astype(np.float32) / 255.0)
    assert sorted(mc.load_matches(f)) == sorted(k for r, s in mc.view_pairs([0, 1, 2]) for k in mc.match_keys(views.names[r], views.names[s]))
    xyz2, rgb2 = mc.build_cloud(folder, f, dataset_name="LLFF", n_views=3, resolution=1, iterations=0)
    assert np.array_equal(xyz2, xyz) and np.array_equal(rgb2, rgb)
