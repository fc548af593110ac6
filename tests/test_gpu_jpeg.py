"""GPU: baseline JPEG on the device (csrc/jpeg.hip), frames.jpeg_encode and the video path of render_path / the spiral CLI.

Device scans and lengths equal the numpy yardstick (tests/jpeg_ref.py) bit for bit: at the smallest shapes at which each stage
can go wrong (one MCU; partial MCU row and column; odd sizes with both edges replicated; 1x1; 17x16; 70 MCUs) for a content
per coding path (constant: DC difference 0 and an immediate EOB; natural at quality 90; uniform noise at quality 100: long
codes, stuffed bytes; sparse speckle: zero runs >= 16, ZRL; full range at quality 100: size categories up to 11), in batches of
1, 3 and 8 different views; a frame without room reports -1 and leaves every byte alone; the launch sequence is capturable in
a graph; render_path(video=...) and `spiral --video` write three AVI files whose frames are the yardstick's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as J  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 16), (40, 24), (37, 19), (1, 1), (17, 16), (160, 112)]            # (W, H)
CONTENT = [("constant", 90), ("natural", 90), ("noise", 100), ("sparse", 90), ("full_range", 100)]


def _scans(images, quality, capacity=None, canary=None):
    """The raw entry point: (lengths, out uint8 [n, capacity]) on the host."""
    from binocular3dgs_amd import _C, frames
    dev = [torch.from_numpy(a).cuda() for a in images]
    H, W, _ = images[0].shape
    cap = capacity or frames.jpeg_scan_bound(W, H)
    out = torch.full((len(dev) * cap,), canary if canary is not None else 0, dtype=torch.uint8, device="cuda")
    lengths = torch.full((len(dev),), -7, dtype=torch.int64, device="cuda")
    _C.jpeg_encode(dev, frames._device_qtables(quality, "cuda"), out, cap, lengths)
    return lengths.cpu().tolist(), out.cpu().numpy().reshape(len(dev), cap)


@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("name,quality", CONTENT)
def test_scan_bytes_equal_the_yardstick(name, quality, W, H):
    from binocular3dgs_amd import frames
    img = J.GENERATORS[name](W, H, seed=W + H)
    st = {}
    ref = J.scan(img, quality, st)
    if name == "noise" and W * H >= 40 * 24:
        assert st["stuffed"] > 0 and st["eob"] < st["blocks"] // 2
    if name == "sparse" and W * H >= 37 * 19:
        assert st["zrl"] > 0
    if name == "full_range" and W * H >= 37 * 19:
        assert st["max_size"] == 11
    lengths, out = _scans([img], quality, canary=0x5A)
    assert lengths == [len(ref)]
    assert out[0, :len(ref)].tobytes() == ref
    assert (out[0, len(ref):] == 0x5A).all()
    (data,) = frames.jpeg_encode([torch.from_numpy(img).cuda()], quality)
    assert data == J.encode(img, quality)


def test_scan_bytes_across_the_seam_of_the_looped_scans():
    """528 x 512 is 33 x 32 = 1056 MCUs: two trips of the 1024-thread scan of the MCU bit counts.  Noise at quality 100 gives more
    than 64 KiB of scan (1024 chunks of 64 bytes), so the scan of the stuffed bytes loops as well, with stuffed bytes in every
    trip."""
    W, H, quality = 528, 512, 100
    img = J.GENERATORS["noise"](W, H, seed=3)
    st = {}
    ref = J.scan(img, quality, st)
    assert st["blocks"] == 6 * 1056 and len(ref) > 2 * 1024 * 64 and st["stuffed"] > 0
    lengths, out = _scans([img], quality, canary=0x5A)
    assert lengths == [len(ref)]
    assert out[0, :len(ref)].tobytes() == ref
    assert (out[0, len(ref):] == 0x5A).all()


@pytest.mark.parametrize("n", [1, 3, 8])
def test_batches_of_different_views(n):
    W, H = 40, 24
    names = ("natural", "sparse", "constant", "full_range", "noise", "natural", "sparse", "natural")
    images = [J.GENERATORS[names[k]](W, H, seed=10 + k) for k in range(n)]
    refs = [J.scan(a, 90) for a in images]
    lengths, out = _scans(images, 90)
    assert lengths == [len(r) for r in refs]
    for k, r in enumerate(refs):
        assert out[k, :len(r)].tobytes() == r, k


def test_a_frame_without_room_is_refused_and_touches_nothing():
    from binocular3dgs_amd import frames
    W, H, q = 37, 19, 100
    images = [J.constant(W, H, 1), J.noise(W, H, 2), J.natural(W, H, 3)]
    refs = [J.scan(a, q) for a in images]
    cap = max(len(refs[0]), len(refs[2])) + 3
    assert len(refs[1]) > cap
    lengths, out = _scans(images, q, capacity=cap, canary=0xA5)
    assert lengths == [len(refs[0]), -1, len(refs[2])]
    assert (out[1] == 0xA5).all()                                        # nothing of the refused frame was written
    for k in (0, 2):
        assert out[k, :len(refs[k])].tobytes() == refs[k] and (out[k, len(refs[k]):] == 0xA5).all()
    lengths, out = _scans(images, q, capacity=len(refs[1]), canary=0xA5)  # exactly enough
    assert lengths[1] == len(refs[1]) and out[1].tobytes() == refs[1]
    lengths, out = _scans(images, q, capacity=len(refs[1]) - 1, canary=0xA5)
    assert lengths[1] == -1 and (out[1] == 0xA5).all()
    # jpeg_encode starts from a modest room, meets -1, encodes that frame again at the bound
    frames._jpeg_capacity[(H, W, q)] = cap
    try:
        got = frames.jpeg_encode([torch.from_numpy(a).cuda() for a in images], q)
        assert frames._jpeg_capacity[(H, W, q)] >= len(refs[1])
    finally:
        frames._jpeg_capacity.pop((H, W, q), None)
    assert got == [J.encode(a, q) for a in images]


def test_encode_is_capturable():
    from binocular3dgs_amd import _C, frames
    W, H, q = 40, 24, 90
    inputs = [J.natural(W, H, 5), J.sparse(W, H, 6), J.noise(W, H, 7)]
    cap = frames.jpeg_scan_bound(W, H)
    qt = frames._device_qtables(q, "cuda")
    static = [torch.from_numpy(inputs[0]).cuda(), torch.from_numpy(inputs[1]).cuda()]
    out = torch.zeros(2 * cap, dtype=torch.uint8, device="cuda")
    lengths = torch.zeros(2, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _C.jpeg_encode(static, qt, out, cap, lengths)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _C.jpeg_encode(static, qt, out, cap, lengths)
    for a, b in ((inputs[2], inputs[0]), (inputs[1], inputs[2])):
        static[0].copy_(torch.from_numpy(a).cuda())
        static[1].copy_(torch.from_numpy(b).cuda())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        n, o = lengths.cpu().tolist(), out.cpu().numpy().reshape(2, cap)
        for k, img in enumerate((a, b)):
            ref = J.scan(img, q)
            assert n[k] == len(ref) and o[k, :n[k]].tobytes() == ref


def test_binding_refuses_what_it_cannot_encode():
    from binocular3dgs_amd import _C, _lib, frames
    qt = frames._device_qtables(90, "cuda")
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    out, n = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.jpeg_encode([img.cpu()], qt, out, 4096, n)
    with pytest.raises(ValueError):
        _C.jpeg_encode([img] * 9, qt, out, 16, n)
    with pytest.raises(ValueError):
        _C.jpeg_encode([img], qt, out, 0, n)
    with pytest.raises(ValueError):
        _C.jpeg_encode([img], qt, out, 8192, n)
    with pytest.raises(ValueError):
        frames.jpeg_encode([img.float()])
    assert frames.jpeg_encode([]) == []


# ---- the video path ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from binocular3dgs_amd import frames, synth
    W, H = 100, 76                                           # no multiple of 16: both edges replicated
    model = synth.synth_model(20_000, seed=4, device="cuda", width=W, height=H)
    cams = synth.synth_cameras(W, H, yaws=tuple(range(-16, 20, 4)), device="cuda")       # 9 views: a batch of 8 and one of 1
    bg = torch.tensor([0.0, 0.0, 0.0], device="cuda")
    tensors = frames.render_path(model, cams, bg)
    return model, cams, bg, tensors


def test_render_path_writes_the_three_videos(scene, tmp_path):
    from binocular3dgs_amd import frames
    model, cams, bg, tensors = scene
    res = frames.render_path(model, cams, bg, str(tmp_path / "png"), video=(str(tmp_path / "v"), "fern"), png=False, fps=30.0,
                             quality=85)
    assert res["png"] == [] and not os.path.exists(tmp_path / "png")                      # no PNG was written
    assert [os.path.basename(p) for p in res["video"]] == ["out_fern.avi", "out_depth_fern.avi", "out_cdepth_fern.avi"]
    assert sorted(os.listdir(tmp_path / "v")) == sorted(os.path.basename(p) for p in res["video"])
    for key, path in zip(("rgb", "depth", "cdepth"), res["video"]):
        W, H, fps, got = frames.avi_frames(path)
        assert (W, H, fps, len(got)) == (100, 76, 30.0, len(cams))
        for i, data in enumerate(got):
            assert data == J.encode(tensors[i][key].cpu().numpy(), 85), (key, i)
    # "directory/stem" form; different camera sizes are refused
    res2 = frames.render_path(model, cams[:2], bg, video=str(tmp_path / "w" / "s"))
    assert [os.path.relpath(p, tmp_path) for p in res2["video"]] == ["w/out_s.avi", "w/out_depth_s.avi", "w/out_cdepth_s.avi"]
    assert frames.avi_frames(res2["video"][0])[3][1] == J.encode(tensors[1]["rgb"].cpu().numpy(), 90)
    from binocular3dgs_amd import synth
    with pytest.raises(ValueError, match="one size"):
        frames.render_path(model, cams[:1] + synth.synth_cameras(64, 48, yaws=(0.0,), device="cuda"), bg, video=(str(tmp_path), "x"))


def test_render_path_with_video_keeps_the_png_files(scene, tmp_path):
    from binocular3dgs_amd import frames
    model, cams, bg, tensors = scene
    plain = frames.render_path(model, cams, bg, str(tmp_path / "a"))
    both = frames.render_path(model, cams, bg, str(tmp_path / "b"), video=(str(tmp_path), "s"))
    assert [os.path.basename(p) for p in both["png"]] == [os.path.basename(p) for p in plain] and len(plain) == 3 * len(cams)
    for p, q in zip(plain, both["png"]):
        assert open(p, "rb").read() == open(q, "rb").read()
    for i in (0, 8):                                        # ... which are the bytes png_bytes makes of the device frames
        for key, name in (("rgb", "{:05d}.png"), ("depth", "depth_{:05d}.png"), ("cdepth", "cdepth_{:05d}.png")):
            assert open(tmp_path / "b" / name.format(i), "rb").read() == frames.png_bytes(tensors[i][key].cpu())
    assert len(frames.avi_frames(both["video"][2])[3]) == len(cams)


def test_spiral_cli_writes_the_named_videos(tmp_path, capsys):
    from binocular3dgs_amd import frames, spiral, synth
    src = os.path.join(ROOT, "tests", "golden", "scene_llff")
    model = synth.synth_model(5000, seed=1, device="cuda", width=64, height=48)
    ply = tmp_path / "m" / "point_cloud" / "iteration_7" / "point_cloud.ply"
    os.makedirs(ply.parent)
    model.save_ply(str(ply))
    assert spiral.main(["-m", str(tmp_path / "m"), "-s", src, "-r", "8", "--frames", "8", "--video", "--no_png", "--fps", "10"]) == 0
    text = capsys.readouterr().out
    assert "ffmpeg" not in text and "out_depth_scene_llff.avi" in text
    names = sorted(n for n in os.listdir(tmp_path / "m") if n.endswith(".avi"))
    assert names == ["out_cdepth_scene_llff.avi", "out_depth_scene_llff.avi", "out_scene_llff.avi"]
    assert not os.path.exists(tmp_path / "m" / "render")
    for n in names:
        W, H, fps, got = frames.avi_frames(str(tmp_path / "m" / n))
        assert fps == 10.0 and len(got) == 8 and all(g[:2] == b"\xff\xd8" and g[-2:] == b"\xff\xd9" for g in got)
        assert got[0][:len(frames.jpeg_header(W, H, 90))] == frames.jpeg_header(W, H, 90)
    # with PNG files, through run(); without --video nothing changes: the ffmpeg lines are printed
    spiral.run(str(tmp_path / "m"), src, resolution=8, n_frames=8, video=True)
    assert len([f for f in os.listdir(tmp_path / "m" / "render" / "ours_7") if f.endswith(".png")]) == 24
    capsys.readouterr()
    spiral.run(str(tmp_path / "m"), src, resolution=8, n_frames=8)
    assert "video (not encoded here):" in capsys.readouterr().out
