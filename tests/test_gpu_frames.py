"""GPU: frames of a rendered path (binocular3dgs_amd/frames.py, csrc/frames.hip).

  * encode_frames on the inputs of golden G13 (recorded from the reference's spiral.render_set): rgb and gray bit for bit,
    the percentile bounds exactly, the colour map on >= 99.99 % of the pixels (a differing pixel sits within 1e-6 of a bin
    edge k/256: fp32 log ulps), the empty-view rule;
  * the order statistics at full size (8 views of 800x600, random values and real render depths) against torch.sort;
  * render_path on a 1M-Gaussian synthetic model: 19 cameras of two sizes, rgb equal to the quantised render_views output,
    batch 1 == batch 8 == a second call, the PNG files decode to the returned frames under the reference's names;
  * isolation: a path render between training steps changes no bit of the model, the optimiser or the training rasterizer."""
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "spiral.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _quantise_hwc(x):
    return torch.clamp(x * 255 + 0.5, 0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _bounds_ref(v: torch.Tensor, percentile=99.0):
    """np.interp(ps * (n / 100), [1..n], sort(v)) with numpy's dtypes, the sort from torch."""
    s = torch.sort(v.reshape(-1))[0].double().cpu().numpy()
    n = s.size
    f = float(np.float32(n) / np.float32(100))
    ps = np.array([50 - percentile / 2, 50 + percentile / 2])
    return np.interp(ps * f, np.arange(1, n + 1, dtype=np.float64), s)


def test_encode_frames_matches_the_reference(g):
    from binocular3dgs_amd import frames
    nv = int(g["n_frames_views"])
    renders = [_dev(g[f"f{i}_render"]) for i in range(nv)]
    depths = [_dev(g[f"f{i}_rendered_depth"]) for i in range(nv)]
    alphas = [_dev(g[f"f{i}_rendered_alpha"]) for i in range(nv)]
    out = frames.encode_frames(renders, depths, alphas, bounds=True)
    b = out["bounds"].cpu().numpy()
    total = differ = 0
    for i in range(nv):
        assert np.array_equal(out["rgb"][i].cpu().numpy(), g[f"f{i}_rgb"]), i
        assert np.array_equal(out["depth"][i].cpu().numpy(), g[f"f{i}_gray"]), i
        assert np.array_equal(b[i], g[f"f{i}_bounds"], equal_nan=True), (i, b[i], g[f"f{i}_bounds"])
        got, ref = out["cdepth"][i].cpu().numpy(), g[f"f{i}_cdepth"]
        bad = ~(got == ref).all(-1)
        total += bad.size
        differ += int(bad.sum())
        if bad.any():
            x = g[f"f{i}_value"][bad] * 256
            assert np.all(np.abs(x - np.round(x)) <= 256e-6), (i, x)
        if str(g[f"f{i}_kind"]) == "empty":
            assert np.isnan(b[i]).all()
            assert (got == frames.TURBO_U8[0]).all() and (out["depth"][i].cpu().numpy() == 0).all()
    assert differ <= 1e-4 * total, (differ, total)
    # the same bits on every call, batches of any composition
    again = frames.encode_frames(renders[::-1], depths[::-1], alphas[::-1], bounds=True)
    for k in ("rgb", "depth", "cdepth"):
        for i in range(nv):
            assert torch.equal(again[k][nv - 1 - i], out[k][i])
    assert np.array_equal(again["bounds"].flip(0).cpu().numpy(), b, equal_nan=True)


def test_encode_frames_outputs_can_be_skipped(g):
    from binocular3dgs_amd import _C, frames
    r, d, a = _dev(g["f2_render"]), _dev(g["f2_rendered_depth"]), _dev(g["f2_rendered_alpha"])
    H, W = r.shape[1:]
    lut = torch.from_numpy(frames.TURBO_U8.copy()).cuda()
    cm = torch.full((1, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    rg = torch.full_like(cm, 9)
    _C.encode_frames([r], [d], [a], None, None, cm, 99.0, lut)
    _C.encode_frames([r], None, None, rg, None, None, 99.0, lut)
    assert torch.equal(cm[0], frames.encode_frames([r], [d], [a])["cdepth"][0])
    assert np.array_equal(rg[0].cpu().numpy(), g["f2_rgb"])
    q = frames.quantize_rgb([r])[0]
    assert torch.equal(q, rg[0])


@pytest.mark.parametrize("source", ["random", "render"])
def test_order_statistics_at_full_size(source):
    from binocular3dgs_amd import frames, synth
    W, H, nv = 800, 600, 8
    gen = torch.Generator(device="cuda").manual_seed(5)
    if source == "random":
        depths = [torch.rand(1, H, W, device="cuda", generator=gen) * 4 + 0.5 for _ in range(nv)]
        alphas = [torch.rand(1, H, W, device="cuda", generator=gen) for _ in range(nv)]
        alphas[3][:, :100] = 0.0
    else:
        from binocular3dgs_amd import evaluate
        model = synth.synth_model(200_000, seed=2, device="cuda", width=W, height=H)
        cams = synth.synth_cameras(W, H, yaws=synth.YAWS_8, device="cuda")
        outs = []
        for idx, o in evaluate._batches(model, cams, torch.zeros(3, device="cuda"), 8, full=True):
            outs += [{k: x[k].clone() for k in ("rendered_depth", "rendered_alpha")} for x in o]
        depths = [o["rendered_depth"] for o in outs]
        alphas = [o["rendered_alpha"] for o in outs]
    rgb = [torch.zeros(3, H, W, device="cuda") for _ in range(nv)]
    out = frames.encode_frames(rgb, depths, alphas, bounds=True)
    b = out["bounds"].cpu().numpy()
    for i in range(nv):
        d, a = depths[i], alphas[i]
        v = 1.0 - (1.0 - (d - d.min()) / (d.max() - d.min())) * a
        assert np.array_equal(b[i], _bounds_ref(v)), (i, b[i], _bounds_ref(v))
        assert torch.equal(out["depth"][i][..., 0], torch.clamp(v[0] * 255 + 0.5, 0, 255).to(torch.uint8))
    for p in (90.0, 50.0, 100.0):
        bp = frames.encode_frames(rgb[:2], depths[:2], alphas[:2], percentile=p, bounds=True)["bounds"].cpu().numpy()
        for i in range(2):
            d, a = depths[i], alphas[i]
            v = 1.0 - (1.0 - (d - d.min()) / (d.max() - d.min())) * a
            assert np.array_equal(bp[i], _bounds_ref(v, p)), (p, i)


def _path_scene():
    from binocular3dgs_amd import synth
    model = synth.synth_model(1_000_000, seed=4, device="cuda", width=320, height=240)
    cams = (synth.synth_cameras(320, 240, yaws=tuple(range(-26, 26, 4)), device="cuda")      # 13 views
            + synth.synth_cameras(200, 144, yaws=(-9.0, -5.0, -1.0, 3.0, 7.0, 11.0), device="cuda"))  # 6 views
    cams = cams[:5] + cams[13:16] + cams[5:13] + cams[16:]
    return model, cams, torch.tensor([0.0, 0.0, 0.0], device="cuda")


def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, W = 8, b"", None
    while pos < len(data):
        n = int.from_bytes(data[pos:pos + 4], "big")
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert int.from_bytes(data[pos + 8 + n:pos + 12 + n], "big") == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            W, H = int.from_bytes(body[:4], "big"), int.from_bytes(body[4:8], "big")
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3)


def test_render_path(tmp_path):
    from binocular3dgs_amd import evaluate, frames
    model, cams, bg = _path_scene()
    assert len(cams) == 19
    ref = evaluate.render_views(model, cams, bg)
    a = frames.render_path(model, cams, bg, batch=8)
    b = frames.render_path(model, cams, bg, batch=1)
    c = frames.render_path(model, cams, bg, batch=8)
    for i, cam in enumerate(cams):
        assert a[i]["rgb"].shape == (cam.image_height, cam.image_width, 3)
        assert torch.equal(a[i]["rgb"], _quantise_hwc(ref[i])), i
        for k in ("rgb", "depth", "cdepth"):
            assert torch.equal(a[i][k], b[i][k]) and torch.equal(a[i][k], c[i][k]), (i, k)
    out = str(tmp_path / "render" / "ours_7")
    paths = frames.render_path(model, cams, bg, out)
    assert len(paths) == 3 * len(cams)
    names = sorted(os.listdir(out))
    assert names == sorted([f"{i:05d}.png" for i in range(19)] + [f"depth_{i:05d}.png" for i in range(19)]
                           + [f"cdepth_{i:05d}.png" for i in range(19)])
    for i in (0, 6, 18):
        for k, name in (("rgb", "{:05d}.png"), ("depth", "depth_{:05d}.png"), ("cdepth", "cdepth_{:05d}.png")):
            assert np.array_equal(_decode_png(os.path.join(out, name.format(i))), a[i][k].cpu().numpy()), (i, k)
    # render.py's tree: renders/ and gt/
    for cam in cams:
        cam.original_image = torch.rand(3, cam.image_height, cam.image_width, device="cuda")
    base = frames.render_set(str(tmp_path), "test", 7, cams[:9], model, bg)
    assert np.array_equal(_decode_png(os.path.join(base, "renders", "00004.png")), _quantise_hwc(ref[4]).cpu().numpy())
    assert np.array_equal(_decode_png(os.path.join(base, "gt", "00008.png")),
                          _quantise_hwc(cams[8].original_image).cpu().numpy())


def test_path_render_leaves_training_state_alone():
    from binocular3dgs_amd import frames, synth
    from binocular3dgs_amd.fused import FusedRasterizer
    from binocular3dgs_amd.step import FusedAdam, ViewShardedStep
    from test_gpu_evaluate import _train_state
    W, H = 160, 120
    gc, gd, ga = synth.synth_pixel_grads(W, H, seed=1, device="cuda")
    fn = lambda i, pkg, spkg: [(pkg["render"], gc), (pkg["rendered_depth"], gd), (pkg["rendered_alpha"], ga), (spkg["render"], gc)]  # noqa: E731
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 1e-3, 0.05]
    model = synth.synth_model(9000, seed=7, device="cuda", width=W, height=H)
    pairs = synth.synth_view_set(W, H, device="cuda")
    bg = torch.tensor([0.1, 0.0, 0.2], device="cuda")
    model.init_densification_stats()
    opt = FusedAdam(model.parameters(), lrs, eps=1e-15)
    fr = FusedRasterizer(model, W, H, num_slots=2 * len(pairs), want_means2D=False)
    st = ViewShardedStep(model, pairs, bg, optimizer=opt, fused=fr)
    path = synth.synth_cameras(W, H, yaws=(2.0, -3.0, 7.0, 11.0, -9.0), device="cuda")
    for it in range(1, 11):
        st.step(pair_grad_fn=fn)
        if it % 5 == 0:
            torch.cuda.synchronize()
            before, words = _train_state(model, opt, fr)
            got = frames.render_path(model, path, bg)
            assert len(got) == len(path)
            torch.cuda.synchronize()
            after, words2 = _train_state(model, opt, fr)
            assert words == words2
            for k, (x, y) in enumerate(zip(before, after)):
                assert torch.equal(x, y), f"the path render changed training state entry {k} at step {it}"
