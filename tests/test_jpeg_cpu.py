"""CPU: the host side of the video path (binocular3dgs_amd/frames.py) and the JPEG yardstick (tests/jpeg_ref.py).

  * the yardstick against an independent decoder: Pillow opens every output at the right size, and at quality 90 the natural
    image at 64x48 loses no more against the source than Pillow's own baseline 4:2:0 encode of it.  Measured gap: 0.000 dB --
    with the IJG slow-integer definitions the scan bytes (and the header) are identical to Pillow 12.2 / libjpeg-turbo 3.1.4
    whenever the size is a multiple of 16 (other sizes differ by the padding rule only: edge replication here, dummy blocks
    there; the PSNR agrees to 0.001 dB).  The margin is that gap plus 0.1 dB.
  * jpeg_tables / jpeg_header of the product equal the yardstick's; segment lengths are self-consistent;
  * write_avi / avi_frames: round trip, padding byte, one frame, no frame, idx1 offsets, chunk sizes add up to the RIFF size."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_ref as J


def _psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize("name,W,H,q", [("natural", 64, 48, 90), ("natural", 37, 19, 90), ("noise", 40, 24, 100), ("sparse", 64, 48, 90),
                                        ("full_range", 17, 16, 100), ("constant", 1, 1, 90), ("natural", 160, 112, 50)])
def test_yardstick_decodes_with_pillow(name, W, H, q):
    Image = pytest.importorskip("PIL.Image")
    img = J.GENERATORS[name](W, H, 1)
    dec = np.asarray(Image.open(io.BytesIO(J.encode(img, q))).convert("RGB"))
    assert dec.shape == (H, W, 3)
    assert _psnr(img, dec) > (10.0 if name in ("noise", "full_range") else 30.0)


def test_yardstick_loses_no_more_than_pillow():
    Image = pytest.importorskip("PIL.Image")
    img = J.natural(64, 48, 1)
    ours = J.encode(img, 90)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=2, optimize=False)
    theirs = buf.getvalue()
    p_ours = _psnr(img, np.asarray(Image.open(io.BytesIO(ours)).convert("RGB")))
    p_theirs = _psnr(img, np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB")))
    same_scan = J.split(ours)[1] == J.split(theirs)[1]
    print(f"PSNR ours {p_ours:.4f} dB, Pillow {p_theirs:.4f} dB, gap {p_theirs - p_ours:.4f} dB, scan bytes identical: {same_scan}")
    assert p_ours >= p_theirs - (0.0 + 0.1)          # measured gap 0.000 dB (identical bytes), plus 0.1 dB


def test_yardstick_images_reach_every_coding_path():
    st = {}
    J.scan(J.noise(40, 24, 1), 100, st)              # long codes, nearly no EOB, stuffing
    assert st["stuffed"] > 0 and st["eob"] < st["blocks"] // 2 and st["max_size"] >= 8
    J.scan(J.sparse(40, 24, 1), 90, st)              # zero runs >= 16
    assert st["zrl"] > 0
    J.scan(J.full_range(40, 24, 1), 100, st)         # DC differences over the whole range
    assert st["max_size"] == 11
    J.scan(J.constant(40, 24, 1), 90, st)            # DC difference 0 and an immediate EOB in every block but the first ones
    assert st["eob"] == st["blocks"] and st["zrl"] == 0


def test_tables():
    from binocular3dgs_amd import frames
    l50, c50 = frames.jpeg_tables(50)
    assert np.array_equal(l50, J.LUMA_Q50) and np.array_equal(c50, J.CHROMA_Q50)
    assert l50[0, 1] == 11 and l50[1, 0] == 12 and c50[0, 3] == 47          # Annex K, row-major
    for t in frames.jpeg_tables(100):
        assert (t == 1).all()
    for q in (-5, 0, 1, 10, 49, 50, 51, 90, 99, 100, 300):
        for a, b in zip(frames.jpeg_tables(q), J.tables(q)):
            assert np.array_equal(a, b) and a.min() >= 1 and a.max() <= 255 and a.shape == (8, 8)
    assert frames.jpeg_tables(1)[0].max() == 255


def test_header_segments_are_self_consistent():
    from binocular3dgs_amd import frames
    for W, H, q in ((800, 600, 90), (1, 1, 100), (65535, 3, 5)):
        h = frames.jpeg_header(W, H, q)
        assert h == J.header(W, H, q)
        assert h[:2] == b"\xff\xd8"
        pos, seen = 2, []
        while pos < len(h):
            assert h[pos] == 0xFF
            marker, (n,) = h[pos + 1], struct.unpack(">H", h[pos + 2:pos + 4])
            seen.append((marker, h[pos + 4:pos + 2 + n]))
            pos += 2 + n
        assert pos == len(h)                                                 # the lengths tile the header exactly
        assert [m for m, _ in seen] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
        sof = seen[3][1]
        assert struct.unpack(">BHHB", sof[:6]) == (8, H, W, 3) and sof[6:9] == bytes([1, 0x22, 0])
        for _, body in seen[4:8]:                                            # DHT: 16 counts, then that many symbols
            assert len(body) == 17 + sum(body[1:17])
        for k, (_, body) in enumerate(seen[1:3]):                            # DQT in zigzag order
            assert body[0] == k and len(body) == 65
            assert [body[1 + i] for i in range(64)] == [int(frames.jpeg_tables(q)[k].reshape(-1)[z]) for z in J.ZIGZAG]
    with pytest.raises(ValueError):
        frames.jpeg_header(0, 4, 90)
    with pytest.raises(ValueError):
        frames.jpeg_header(4, 65536, 90)


def _walk_riff(data):
    """[(fourcc, offset of the body, size)] of the top-level chunks; checks that they tile the RIFF body."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    riff = struct.unpack("<I", data[4:8])[0]
    assert 8 + riff == len(data)
    pos, out = 12, []
    while pos < len(data):
        kind, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        out.append((kind if kind != b"LIST" else data[pos + 8:pos + 12], pos + 8, n))
        pos += 8 + n + (n & 1)
    assert pos == len(data)
    return out


def test_avi_round_trip(tmp_path):
    from binocular3dgs_amd import frames
    rng = np.random.default_rng(3)
    jpegs = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (101, 64, 1, 255, 30)]      # odd lengths: padding bytes
    path = frames.write_avi(str(tmp_path / "a.avi"), jpegs, (37, 19), fps=12.5)
    W, H, fps, got = frames.avi_frames(path)
    assert (W, H, fps) == (37, 19, 12.5) and got == jpegs
    data = open(path, "rb").read()
    chunks = _walk_riff(data)
    assert [c[0] for c in chunks] == [b"hdrl", b"movi", b"idx1"]
    (_, hdrl, hn), (_, movi, mn), (_, idx, inn) = chunks
    assert data[hdrl + 4:hdrl + 8] == b"avih" and struct.unpack("<I", data[hdrl + 8:hdrl + 12])[0] == 56
    avih = struct.unpack("<14I", data[hdrl + 12:hdrl + 68])
    assert avih[0] == 80000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (37, 19)
    assert data[hdrl + 68:hdrl + 72] == b"LIST" and data[hdrl + 76:hdrl + 80] == b"strl" and data[hdrl + 80:hdrl + 84] == b"strh"
    assert data[hdrl + 88:hdrl + 96] == b"vidsMJPG"
    strf = hdrl + 80 + 8 + 56
    assert data[strf:strf + 4] == b"strf" and struct.unpack("<I", data[strf + 4:strf + 8])[0] == 40
    bih = struct.unpack("<IiiHH4sI", data[strf + 8:strf + 32])
    assert bih == (40, 37, 19, 1, 24, b"MJPG", 37 * 19 * 3)
    assert strf + 8 + 40 == hdrl + hn                                       # hdrl holds exactly avih and the one strl
    # movi: one 00dc chunk per frame, word-aligned; idx1 offsets count from the 'movi' tag
    pos = movi + 4
    assert inn == 16 * len(jpegs)
    for k, j in enumerate(jpegs):
        assert pos % 2 == 0 and data[pos:pos + 4] == b"00dc" and struct.unpack("<I", data[pos + 4:pos + 8])[0] == len(j)
        ckid, flags, off, n = struct.unpack("<4sIII", data[idx + 16 * k:idx + 16 * k + 16])
        assert (ckid, flags, movi + off, n) == (b"00dc", 0x10, pos, len(j))
        if len(j) & 1:
            assert data[pos + 8 + len(j)] == 0
        pos += 8 + len(j) + (len(j) & 1)
    assert pos == movi + mn
    # one frame; no frame
    one = frames.write_avi(str(tmp_path / "one.avi"), jpegs[:1], (8, 8))
    assert frames.avi_frames(one) == (8, 8, 25.0, jpegs[:1])
    _walk_riff(open(one, "rb").read())
    with pytest.raises(ValueError):
        frames.write_avi(str(tmp_path / "none.avi"), [], (8, 8))
    assert not os.path.exists(tmp_path / "none.avi")
    with pytest.raises(ValueError):
        frames.avi_frames(__file__)


def test_avi_refuses_two_gib(tmp_path):
    from binocular3dgs_amd import frames

    class Big(bytes):                      # a frame that claims 1.5 GiB without holding it
        def __len__(self):
            return 3 << 29
    with pytest.raises(ValueError, match="2 GiB"):
        frames.write_avi(str(tmp_path / "big.avi"), [Big(b"x"), Big(b"y")], (8, 8))
    assert not os.path.exists(tmp_path / "big.avi")


def test_abi_argument_errors_without_a_device():
    import ctypes as C
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    assert L.b3gs_jpeg_workspace_bytes(0, 16, 16) == 0 and L.b3gs_jpeg_workspace_bytes(9, 16, 16) == 0
    assert L.b3gs_jpeg_workspace_bytes(1, 0, 16) == 0 and L.b3gs_jpeg_workspace_bytes(1, 16, 65536) == 0
    small, big = L.b3gs_jpeg_workspace_bytes(1, 16, 16), L.b3gs_jpeg_workspace_bytes(8, 600, 800)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert L.b3gs_jpeg_workspace_bytes(1, 65535, 65535) > 1 << 32
    imgs = (C.c_void_p * 8)(*([4096] * 8))
    p = C.c_void_p(4096)                    # never dereferenced: every call below fails its argument check
    ERR_ARG = -1
    for nv, H, W in ((0, 16, 16), (9, 16, 16), (1, 0, 16), (1, 16, 0), (1, 65536, 16), (1, 16, 65536)):
        assert L.b3gs_jpeg_encode_batch(nv, imgs, H, W, p, p, 100, p, p, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, None, 16, 16, p, p, 100, p, p, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, None, p, 100, p, p, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, p, None, 100, p, p, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, p, p, 100, None, p, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, p, p, 100, p, None, None) == ERR_ARG
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, p, p, 0, p, p, None) == ERR_ARG
    assert b"capacity" in L.b3gs_last_error()
    imgs[0] = None
    assert L.b3gs_jpeg_encode_batch(1, imgs, 16, 16, p, p, 100, p, p, None) == ERR_ARG
