"""CPU: the spiral path's host side against golden G13 (recorded from the reference's spiral.py / dataset_readers.py /
camera_utils.py): the cameras of both datasets at every resolution rule, the PNG writer, the turbo table, cfg_args."""
import os
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(ROOT, "tests", "golden", "spiral.npz"))


@pytest.mark.parametrize("name", ["llff", "dtu"])
def test_spiral_cameras_match_the_reference(g, name):
    from binocular3dgs_amd import camera_path
    pb = g[f"{name}_poses_bounds"]
    for res in g["resolutions"]:
        cams = camera_path.spiral_cameras(pb, dtu=name == "dtu", resolution=int(res), device="cpu")
        assert len(cams) == 180
        size = np.array([[c.image_width, c.image_height] for c in cams])
        assert np.array_equal(size, g[f"{name}_size_r{res}"]), (name, res, size[0], g[f"{name}_size_r{res}"][0])
        for key, got in (("R", np.stack([c.R for c in cams])), ("T", np.stack([c.T for c in cams])),
                         ("FovX", np.array([c.FoVx for c in cams])), ("FovY", np.array([c.FoVy for c in cams]))):
            ref = g[f"{name}_{key}"]
            assert np.allclose(got, ref, rtol=1e-9, atol=1e-12), (name, res, key, np.abs(got - ref).max())


def test_spiral_cameras_from_dir_picks_dtu_by_name(g, tmp_path):
    from binocular3dgs_amd import camera_path
    for name, sub in (("llff", "fern"), ("dtu", "scan8")):
        d = tmp_path / sub
        d.mkdir()
        np.save(str(d / "poses_bounds.npy"), g[f"{name}_poses_bounds"])
        cams = camera_path.spiral_cameras_from_dir(str(d), resolution=4, device="cpu", n_frames=180)
        assert np.allclose(np.stack([c.T for c in cams]), g[f"{name}_T"], rtol=1e-9, atol=1e-12)
        assert [cams[0].image_width, cams[0].image_height] == list(g[f"{name}_size_r4"][0])


def test_render_size_rules():
    from binocular3dgs_amd.camera_path import render_size
    assert render_size(504.0, 378.0, 8) == (63, 47)
    assert render_size(400.0, 300.0, 8) == (50, 38)          # round(37.5): half to even
    assert render_size(8000.0, 6000.0, -1) == (6400, 4800)
    assert render_size(504.0, 378.0, -1) == (504, 378)
    assert render_size(504.0, 378.0, 250) == (250, 187)


def _decode(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, ctype, comp, filt, inter) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3)


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (60, 80)])
def test_write_png_round_trips(tmp_path, shape):
    import torch
    from binocular3dgs_amd import frames
    img = np.random.default_rng(shape[1]).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    p = frames.write_png(str(tmp_path / "a.png"), img)
    assert np.array_equal(_decode(open(p, "rb").read()), img)
    frames.write_png(str(tmp_path / "b.png"), torch.from_numpy(img))
    assert open(str(tmp_path / "b.png"), "rb").read() == open(p, "rb").read()
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(p) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


def test_write_png_rejects_other_layouts(tmp_path):
    from binocular3dgs_amd import frames
    with pytest.raises(ValueError):
        frames.write_png(str(tmp_path / "x.png"), np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError):
        frames.write_png(str(tmp_path / "x.png"), np.zeros((4, 4, 3), np.float32))


def test_turbo_table(g):
    from binocular3dgs_amd import frames
    assert frames.TURBO_U8.shape == (256, 3) and frames.TURBO_U8.dtype == np.uint8
    assert np.array_equal(frames.TURBO_U8, g["turbo_u8"])
    try:
        from matplotlib import colormaps
    except ImportError:
        return
    cm = colormaps.get_cmap("turbo")
    lut = np.asarray(cm(np.arange(256) / 255.0)[:, :3], dtype=np.float64)
    assert np.array_equal(frames.TURBO_U8, np.clip(lut * 255 + 0.5, 0, 255).astype(np.uint8))


def test_cfg_args_are_read_without_evaluating(tmp_path):
    from binocular3dgs_amd.spiral import read_cfg_args
    (tmp_path / "cfg_args").write_text("Namespace(data_device='cuda', eval=True, resolution=-1, sh_degree=1, "
                                       "source_path='/data/scan8', white_background=False, images='images')")
    cfg = read_cfg_args(str(tmp_path))
    assert cfg["source_path"] == "/data/scan8" and cfg["resolution"] == -1 and cfg["white_background"] is False
    marker = tmp_path / "ran"
    (tmp_path / "cfg_args").write_text(f"Namespace(x=open({str(marker)!r}, 'w'), resolution=2)")
    assert read_cfg_args(str(tmp_path)) == {"resolution": 2}
    assert not marker.exists()
    (tmp_path / "cfg_args").write_text(f"__import__('os').mkdir({str(marker)!r})")
    assert read_cfg_args(str(tmp_path)) == {}
    assert not marker.exists()
