"""Frames of a rendered path: the rgb, gray depth and colour-mapped depth images of the reference's spiral.py, encoded on the
device, and PNG files written without an imaging library.

    spiral.py:101-139   render_set: per view one render(), the gray depth map 1 - (1 - normalised depth) * alpha, the turbo
                        colour map of visualize_cmap (percentile bounds, -log(x + 1e-6) curve), three save_image calls
    render.py:24-35     render_set: renders/ and gt/ PNGs of the train / test views, the tree metrics.py reads

encode_frames() quantises all three images of up to 8 views of one W x H in one b3gs_encode_frames_batch call
(csrc/frames.hip): the same bits as save_image writes (uint8(clamp(x*255 + 0.5, 0, 255))), with the percentile bounds from
an exact radix select of the order statistics instead of a host sort.  render_path() renders through evaluation's batched
renderer (evaluate._batches: its own FusedRasterizer, 8 views per launch) and encodes every batch on the device; the host sees
the frames once per batch, only to write them.

jpeg_encode() turns such uint8 images into complete baseline JPEG files on the device (csrc/jpeg.hip: only the compressed bytes
reach the host), write_avi() puts them into a Motion-JPEG AVI file with `struct` alone, and render_path(video=...) does both
for the three streams of a path: the videos the reference's spiral.py makes with ffmpeg (there: H.264 in MP4).

Empty view (max depth == min depth, e.g. a frame that sees nothing): the reference divides 0 by 0; the NaN quantises to 0
and visualize_cmap's nan_to_num maps it to the first colour.  Here: gray 0 and cdepth TURBO_U8[0] everywhere, bounds NaN.
"""
from __future__ import annotations

import os
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

MAX_BATCH = 8           # views per b3gs_encode_frames_batch (B3GS_MAX_FRAME_VIEWS)
PNG_THREADS = 4         # PNG writers (zlib releases the GIL); fixed: the host may be shared

# matplotlib's "turbo" colormap (256 entries) quantised as save_image does: uint8(clamp(lut * 255 + 0.5, 0, 255)) in fp64
TURBO_U8 = np.frombuffer(bytes.fromhex(
    "30123b32154333184a341b51351e5836215f37246638276d392a733a2d793b2f803c32863d358b3e38913f3b973f3e9c"
    "4040a24143a74146ac4249b1424bb5434eba4451bf4454c34456c74559cb455ccf455ed34661d64664da4666dd4669e0"
    "466be3476ee64771e94773eb4776ee4778f0477bf2467df44680f64682f84685fa4687fb458afc458cfd448ffe4391fe"
    "4294ff4196ff4099ff3e9bfe3d9efe3ba0fd3aa3fc38a5fb37a8fa35abf833adf731aff52fb2f42eb4f22cb7f02ab9ee"
    "28bceb27bee925c0e723c3e422c5e220c7df1fc9dd1ecbda1ccdd81bd0d51ad2d21ad4d019d5cd18d7ca18d9c818dbc5"
    "18ddc218dec018e0bd19e2bb19e3b91ae4b61ce6b41de7b21fe9af20eaac22ebaa25eca727eea42aefa12cf09e2ff19b"
    "32f29835f39438f4913cf58e3ff68a43f78746f8844af8804ef97d52fa7a55fa7659fb735dfc6f61fc6c65fd6969fd66"
    "6dfe6271fe5f75fe5c79fe597dff5680ff5384ff5188ff4e8bff4b8fff4992ff4796fe4499fe429cfe409ffd3fa1fd3d"
    "a4fc3ca7fc3aa9fb39acfb38affa37b1f936b4f836b7f735b9f635bcf534bef434c1f334c3f134c6f034c8ef34cbed34"
    "cdec34d0ea34d2e935d4e735d7e535d9e436dbe236dde037dfdf37e1dd37e3db38e5d938e7d739e9d539ebd339ecd13a"
    "eecf3aefcd3af1cb3af2c93af4c73af5c53af6c33af7c13af8be39f9bc39faba39fbb838fbb637fcb336fcb136fdae35"
    "fdac34fea933fea732fea431fea130fe9e2ffe9b2dfe992cfe962bfe932afe9029fd8d27fd8a26fc8725fc8423fb8122"
    "fb7e21fa7b1ff9781ef9751df8721cf76f1af66c19f56918f46617f36315f26014f15d13f05b12ef5811ed5510ec530f"
    "eb500eea4e0de84b0ce7490ce5470be4450ae2430ae14109df3f08dd3d08dc3b07da3907d83706d63506d43305d23105"
    "d02f05ce2d04cc2b04ca2a04c82803c52603c32503c12302be2102bc2002b91e02b71d02b41b01b21a01af1801ac1701"
    "a91601a71401a41301a112019e10019b0f01980e01950d01920b018e0a018b09028808028507028106027e05027a0403"
), dtype=np.uint8).reshape(256, 3).copy()
TURBO_U8.setflags(write=False)

_luts: Dict[tuple, torch.Tensor] = {}


def _device_lut(lut, device) -> torch.Tensor:
    a = np.ascontiguousarray(np.asarray(lut, dtype=np.uint8).reshape(256, 3))
    key = (a.tobytes(), str(device))
    t = _luts.get(key)
    if t is None:
        t = _luts[key] = torch.from_numpy(a.copy()).to(device)
    return t


def encode_frames(renders: Sequence[torch.Tensor], depths: Sequence[torch.Tensor], alphas: Sequence[torch.Tensor], *,
                  percentile: float = 99., lut=TURBO_U8, bounds: bool = False):
    """-> {"rgb", "depth", "cdepth"}: per view a uint8 [H,W,3] device tensor (and "bounds": float64 [n, 2] device tensor of
    the percentile bounds lo_auto, hi_auto per view when `bounds`).  renders [3,H,W], depths / alphas [1,H,W]; one launch per
    8 views of the same W x H."""
    from . import _C
    n = len(renders)
    if len(depths) != n or len(alphas) != n:
        raise ValueError("one depth and one alpha per render")
    out = {"rgb": [None] * n, "depth": [None] * n, "cdepth": [None] * n}
    bnd = [None] * n
    groups: Dict[tuple, List[int]] = {}
    for i, r in enumerate(renders):
        groups.setdefault(tuple(r.shape), []).append(i)
    for shape, idx in groups.items():
        _, H, W = shape
        dev = renders[idx[0]].device
        l = _device_lut(lut, dev)
        for c0 in range(0, len(idx), MAX_BATCH):
            part = idx[c0:c0 + MAX_BATCH]
            k = len(part)
            imgs = torch.empty((3, k, H, W, 3), dtype=torch.uint8, device=dev)
            b = torch.empty((k, 2), dtype=torch.float64, device=dev) if bounds else None
            _C.encode_frames([renders[i] for i in part], [depths[i] for i in part], [alphas[i] for i in part], imgs[0],
                             imgs[1], imgs[2], float(percentile), l, b)
            for j, i in enumerate(part):
                out["rgb"][i], out["depth"][i], out["cdepth"][i] = imgs[0, j], imgs[1, j], imgs[2, j]
                if bounds:
                    bnd[i] = b[j]
    if bounds:
        out["bounds"] = torch.stack(bnd) if n else torch.empty((0, 2), dtype=torch.float64)
    return out


def quantize_rgb(images: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """save_image's uint8 [H,W,3] of [3,H,W] images (rgb only), on the device."""
    from . import _C
    out: List[Optional[torch.Tensor]] = [None] * len(images)
    groups: Dict[tuple, List[int]] = {}
    for i, r in enumerate(images):
        groups.setdefault(tuple(r.shape), []).append(i)
    for (_, H, W), idx in groups.items():
        dev = images[idx[0]].device
        for c0 in range(0, len(idx), MAX_BATCH):
            part = idx[c0:c0 + MAX_BATCH]
            q = torch.empty((len(part), H, W, 3), dtype=torch.uint8, device=dev)
            _C.encode_frames([images[i] for i in part], None, None, q, None, None, 99.0, _device_lut(TURBO_U8, dev))
            for j, i in enumerate(part):
                out[i] = q[j]
    return out


# ---- PNG ---------------------------------------------------------------------------------------------------------------
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(hwc_uint8, level: int = 6) -> bytes:
    """An 8-bit RGB PNG (filter 0 on every row) of a [H,W,3] uint8 array."""
    a = hwc_uint8.numpy() if isinstance(hwc_uint8, torch.Tensor) else np.asarray(hwc_uint8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_png expects a uint8 [H,W,3] image")
    H, W, _ = a.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    rows[:, 1:] = a.reshape(H, 3 * W)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))


def write_png(path: str, hwc_uint8, level: int = 6) -> str:
    """Writes a uint8 [H,W,3] host image (numpy or CPU tensor) as an RGB8 PNG; stdlib zlib + struct only."""
    data = png_bytes(hwc_uint8, level)
    with open(path, "wb") as fp:
        fp.write(data)
    return path


_PNG_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}      # colour type -> samples per pixel (3 = palette: not read)


def png_size(path: str):
    """(width, height) from the IHDR chunk of a PNG file."""
    with open(path, "rb") as fp:
        head = fp.read(24)
    if head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    return struct.unpack(">II", head[16:24])


def read_png(path: str) -> np.ndarray:
    """uint8 [H,W] (gray), [H,W,2] (gray + alpha), [H,W,3] or [H,W,4] of an 8-bit, non-interlaced PNG; stdlib zlib + struct and
    the five row filters.  Palette, 16-bit, sub-byte and interlaced files raise ValueError."""
    with open(path, "rb") as fp:
        data = fp.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, header = 8, [], None
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + n
    if header is None:
        raise ValueError(f"{path}: no IHDR chunk")
    W, H, depth, ctype, _comp, _filt, interlace = header
    if depth != 8 or ctype not in _PNG_CHANNELS or interlace != 0:
        raise ValueError(f"{path}: only 8-bit non-interlaced gray / gray+alpha / RGB / RGBA PNGs are read "
                         f"(bit depth {depth}, colour type {ctype}, interlace {interlace})")
    bpp = _PNG_CHANNELS[ctype]
    stride = W * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != H * (stride + 1):
        raise ValueError(f"{path}: {raw.size} bytes of image data for {H} rows of {stride + 1}")
    raw = raw.reshape(H, stride + 1)
    out = np.zeros((H, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    for y in range(H):
        f, line = int(raw[y, 0]), raw[y, 1:]
        up = out[y - 1] if y else zero
        if f == 0:
            out[y] = line
        elif f == 2:
            out[y] = line + up
        elif f == 1:                                   # left neighbour: a running sum per sample position (mod 256)
            out[y] = np.cumsum(line.reshape(W, bpp), axis=0, dtype=np.uint8).reshape(-1)
        elif f in (3, 4):                              # depend on the reconstructed left neighbour: pixel by pixel
            cur, ln, upl = [0] * stride, line.tolist(), up.tolist()
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = upl[i]
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    c = upl[i - bpp] if i >= bpp else 0
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (ln[i] + pred) & 255
            out[y] = cur
        else:
            raise ValueError(f"{path}: row filter {f}")
    return out.reshape(H, W) if bpp == 1 else out.reshape(H, W, bpp)


# ---- JPEG --------------------------------------------------------------------------------------------------------------
# ITU-T T.81 Annex K: the quantisation tables (row-major) and the "typical" Huffman tables (bits per code length, symbols)
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
           72, 92, 95, 98, 112, 100, 103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99) + (99,) * 36
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
           49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_DHT = (   # (table class << 4 | id, bits, symbols): DC luminance, AC luminance, DC chrominance, AC chrominance
    (0x00, bytes.fromhex("00010501010101010100000000000000"), bytes(range(12))),
    (0x10, bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")),
    (0x01, bytes.fromhex("00030101010101010101010000000000"), bytes(range(12))),
    (0x11, bytes.fromhex("00020102040403040705040400010277"), bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
        "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))

_qtabs: Dict[tuple, torch.Tensor] = {}
_jpeg_capacity: Dict[tuple, int] = {}     # (H, W, quality) -> bytes per frame the next batch is given room for


def jpeg_tables(quality: int = 90):
    """The luminance and chrominance quantisation tables (int64 [8,8], row-major) of a quality 1..100: Annex K scaled by the
    IJG rule (50: Annex K itself; 100: all ones), clamped to 1..255."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(t, dtype=np.int64) * scale + 50) // 100, 1, 255).reshape(8, 8) for t in (_Q_LUMA, _Q_CHROMA))


def jpeg_header(W: int, H: int, quality: int = 90) -> bytes:
    """Everything of a baseline 4:2:0 JPEG file before the scan: SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS."""
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError("a JPEG frame has 1..65535 pixels per side")

    def seg(marker, body):
        return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate(jpeg_tables(quality)):
        flat = t.reshape(-1)
        out += seg(0xDB, bytes([i]) + bytes(int(flat[k]) for k in _ZIGZAG))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for ident, bits, vals in _DHT:
        out += seg(0xC4, bytes([ident]) + bits + vals)
    return out + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def jpeg_scan_bound(W: int, H: int) -> int:
    """Bytes a scan of W x H cannot exceed: per coefficient a 16-bit code and 11 magnitude bits, every byte stuffed."""
    return ((W + 15) // 16) * ((H + 15) // 16) * 6 * 64 * 27 // 8 * 2 + 2


def _device_qtables(quality: int, device) -> torch.Tensor:
    key = (min(max(int(quality), 1), 100), str(device))
    t = _qtabs.get(key)
    if t is None:
        t = _qtabs[key] = torch.from_numpy(np.stack(jpeg_tables(quality)).reshape(2, 64).astype(np.int16)).to(device)
    return t


def _jpeg_scans(part: Sequence[torch.Tensor], qt: torch.Tensor, capacity: int):
    """One launch: -> (lengths int64 [k], scans uint8 [k, capacity]) on the host, from ONE device->host copy."""
    from . import _C
    k = len(part)
    buf = torch.empty(64 + k * capacity, dtype=torch.uint8, device=part[0].device)     # 8 lengths, then the frames
    _C.jpeg_encode(list(part), qt, buf[64:], capacity, buf[:64].view(torch.int64))
    host = buf.cpu()
    return host[:64].view(torch.int64)[:k].tolist(), host[64:].view(k, capacity).numpy()


def jpeg_encode(images: Sequence[torch.Tensor], quality: int = 90) -> List[bytes]:
    """One complete baseline JPEG file (4:2:0, Annex K Huffman tables, its own DHT segments) per uint8 [H,W,3] device tensor.
    Images of one size are encoded 8 per launch (csrc/jpeg.hip); the host receives one copy per launch: the lengths and the
    compressed bytes.  A launch starts from a modest room per frame (3 bits per pixel, or what earlier frames of this size
    and quality needed); a frame that does not fit comes back with length -1 and is encoded again at the bound."""
    out: List[Optional[bytes]] = [None] * len(images)
    groups: Dict[tuple, List[int]] = {}
    for i, im in enumerate(images):
        if im.dim() != 3 or im.shape[2] != 3 or im.dtype != torch.uint8:
            raise ValueError("jpeg_encode expects uint8 [H,W,3] images")
        groups.setdefault((tuple(im.shape), str(im.device)), []).append(i)
    for ((H, W, _), _dev), idx in groups.items():
        head = jpeg_header(W, H, quality)
        qt = _device_qtables(quality, images[idx[0]].device)
        key = (H, W, min(max(int(quality), 1), 100))
        bound = jpeg_scan_bound(W, H)
        for c0 in range(0, len(idx), MAX_BATCH):
            part = idx[c0:c0 + MAX_BATCH]
            cap = min(_jpeg_capacity.get(key, H * W * 3 // 8 + 1024), bound)
            lengths, scans = _jpeg_scans([images[i] for i in part], qt, cap)
            redo = [j for j, n in enumerate(lengths) if n < 0]
            for j, n in enumerate(lengths):
                if n >= 0:
                    out[part[j]] = head + scans[j, :n].tobytes() + b"\xff\xd9"
            if redo:
                lens2, scans2 = _jpeg_scans([images[part[j]] for j in redo], qt, bound)
                for j, n in zip(redo, lens2):
                    if n < 0:
                        raise RuntimeError("a JPEG scan exceeded its bound")
                    out[part[j]] = head + scans2[redo.index(j), :n].tobytes() + b"\xff\xd9"
                _jpeg_capacity[key] = min(bound, max(lens2) * 5 // 4 + 1024)
    return out


# ---- AVI ---------------------------------------------------------------------------------------------------------------
_AVI_MAX = (1 << 31) - 1            # one RIFF chunk, no OpenDML extension


def _fps_fraction(fps: float):
    from fractions import Fraction
    f = Fraction(float(fps)).limit_denominator(1001)
    if f <= 0:
        raise ValueError("fps must be positive")
    return f.numerator, f.denominator           # dwRate, dwScale


def write_avi(path: str, jpegs: Sequence[bytes], size, fps: float = 25.0) -> str:
    """A Motion-JPEG AVI file of complete JPEG frames of one size = (width, height): RIFF 'AVI ' with hdrl (avih, one strl: strh
    vids/MJPG, strf BITMAPINFOHEADER with compression MJPG), movi (one '00dc' chunk per frame, word-aligned) and idx1 (offsets
    from the 'movi' tag).  `struct` only; no frames, or a file of 2 GiB or more, raise ValueError."""
    W, H = int(size[0]), int(size[1])
    n = len(jpegs)
    if n < 1:
        raise ValueError("an AVI file needs at least one frame")
    rate, scale = _fps_fraction(fps)
    biggest = max(len(j) for j in jpegs)
    movi_bytes = 4 + sum(8 + len(j) + (len(j) & 1) for j in jpegs)
    strl = (b"strh" + struct.pack("<I", 56) + struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, n,
                                                            biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
            + b"strf" + struct.pack("<I", 40) + struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0))
    usec = int(round(1e6 * scale / rate))
    avih = b"avih" + struct.pack("<I", 56) + struct.pack("<14I", usec, int(biggest * rate / scale) & 0xFFFFFFFF, 0, 0x10, n, 0, 1,
                                                          biggest, W, H, 0, 0, 0, 0)
    hdrl = b"LIST" + struct.pack("<I", 4 + len(avih) + 8 + 4 + len(strl)) + b"hdrl" + avih \
        + b"LIST" + struct.pack("<I", 4 + len(strl)) + b"strl" + strl
    riff_bytes = 4 + len(hdrl) + 8 + movi_bytes + 8 + 16 * n
    if 8 + riff_bytes > _AVI_MAX:
        raise ValueError(f"{path}: {8 + riff_bytes} bytes do not fit one RIFF chunk (2 GiB; no OpenDML index is written)")
    index, off = [], 4
    with open(path, "wb") as fp:
        fp.write(b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi")
        for j in jpegs:
            fp.write(b"00dc" + struct.pack("<I", len(j)))
            fp.write(j)
            if len(j) & 1:
                fp.write(b"\0")
            index.append(struct.pack("<4sIII", b"00dc", 0x10, off, len(j)))
            off += 8 + len(j) + (len(j) & 1)
        fp.write(b"idx1" + struct.pack("<I", 16 * n) + b"".join(index))
    return path


def avi_frames(path: str):
    """(width, height, fps, [frame bytes, ...]) of an AVI file with one video stream, read back through idx1."""
    with open(path, "rb") as fp:
        data = fp.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError(f"{path}: not an AVI file")
    end = 8 + struct.unpack("<I", data[4:8])[0]
    pos, movi, idx, size, fps = 12, None, None, None, None
    while pos + 8 <= end:
        kind, n = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = pos + 8
        if kind == b"LIST" and data[body:body + 4] == b"hdrl":
            p = body + 4
            while p + 8 <= body + n:                      # avih, then LIST strl
                k2, n2 = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
                if k2 == b"avih":
                    size = struct.unpack("<II", data[p + 8 + 32:p + 8 + 40])
                elif k2 == b"LIST" and data[p + 8:p + 12] == b"strl":
                    q = p + 12
                    while q + 8 <= p + 8 + n2:
                        k3, n3 = data[q:q + 4], struct.unpack("<I", data[q + 4:q + 8])[0]
                        if k3 == b"strh":
                            scale, rate = struct.unpack("<II", data[q + 8 + 20:q + 8 + 28])
                            fps = rate / scale
                        q += 8 + n3 + (n3 & 1)
                p += 8 + n2 + (n2 & 1)
        elif kind == b"LIST" and data[body:body + 4] == b"movi":
            movi = body
        elif kind == b"idx1":
            idx = (body, n)
        pos = body + n + (n & 1)
    if movi is None or idx is None or size is None or fps is None:
        raise ValueError(f"{path}: hdrl, movi or idx1 is missing")
    frames = []
    for e in range(idx[0], idx[0] + idx[1], 16):
        ckid, _flags, off, n = struct.unpack("<4sIII", data[e:e + 16])
        if ckid != b"00dc" or data[movi + off:movi + off + 4] != b"00dc" or struct.unpack("<I", data[movi + off + 4:movi + off + 8])[0] != n:
            raise ValueError(f"{path}: index entry {len(frames)} does not point at a video chunk")
        frames.append(data[movi + off + 8:movi + off + 8 + n])
    return size[0], size[1], fps, frames


VIDEO_NAMES = ("out_{}.avi", "out_depth_{}.avi", "out_cdepth_{}.avi")     # the reference's names, the container's extension


# ---- drivers -----------------------------------------------------------------------------------------------------------
def render_path(model, cameras: Sequence, bg: torch.Tensor, out_dir: Optional[str] = None, *, batch: int = MAX_BATCH,
                percentile: float = 99., video=None, png: bool = True, fps: float = 25.0, quality: int = 90, source=None):
    """spiral.py's render_set: every camera rendered (up to `batch` <= 8 views of one W x H per launch, evaluation's renderer)
    and encoded on the device.
    out_dir None: -> per camera {"rgb", "depth", "cdepth"} uint8 [H,W,3] device tensors.
    out_dir set:  writes %05d.png, depth_%05d.png, cdepth_%05d.png (camera index) there, one device->host copy per batch
                  and at most PNG_THREADS writer threads; -> the written paths in camera order.
    video set:    (directory, stem), or "directory/stem": the three streams of every batch also go through jpeg_encode
                  straight from the device tensors, and <directory>/out_<stem>.avi, out_depth_<stem>.avi, out_cdepth_<stem>.avi
                  (Motion-JPEG, `fps`, `quality`) are written at the end; every camera must have the same size.
                  -> {"png": the PNG paths (empty without out_dir or with png=False), "video": the three AVI paths}.
                  png=False skips the PNG files and the raw host copy they need.
    source:       where the images come from: an iterable of (camera indices, per-view {"render", "rendered_depth",
                  "rendered_alpha"} on the device) per batch of at most 8 views of one size; default: the model through
                  evaluation's renderer (`model` is not used otherwise; mesh_render.batches is another source)."""
    from . import evaluate
    if source is None:
        source = evaluate._batches(model, cameras, bg, batch, full=True)
    want_png = out_dir is not None and png
    if video is not None:
        vdir, stem = os.path.split(video) if isinstance(video, str) else (video[0], video[1])
        if len(cameras) == 0:
            raise ValueError("a video needs at least one camera")
        sizes = {(int(c.image_width), int(c.image_height)) for c in cameras}
        if len(sizes) != 1:
            raise ValueError(f"a video holds frames of one size; the cameras have {sorted(sizes)}")
        jpegs = {k: [None] * len(cameras) for k in ("rgb", "depth", "cdepth")}
    frames: List[Optional[dict]] = [None] * len(cameras)
    pool = ThreadPoolExecutor(max_workers=PNG_THREADS) if want_png else None
    jobs = []
    if want_png:
        os.makedirs(out_dir, exist_ok=True)
    try:
        with torch.no_grad():
            for idx, outs in source:
                enc = encode_frames([o["render"] for o in outs], [o["rendered_depth"] for o in outs],
                                    [o["rendered_alpha"] for o in outs], percentile=percentile)
                if video is not None:
                    for k in ("rgb", "depth", "cdepth"):
                        for i, data in zip(idx, jpeg_encode(enc[k], quality)):
                            jpegs[k][i] = data
                elif out_dir is None:
                    for j, i in enumerate(idx):
                        frames[i] = {k: enc[k][j] for k in ("rgb", "depth", "cdepth")}
                if pool is None:
                    continue
                host = torch.stack([torch.stack(enc[k]) for k in ("rgb", "depth", "cdepth")]).cpu()   # one copy per batch
                for j, i in enumerate(idx):
                    for k, name in enumerate(("{:05d}.png", "depth_{:05d}.png", "cdepth_{:05d}.png")):
                        jobs.append(pool.submit(write_png, os.path.join(out_dir, name.format(i)), host[k, j]))
        paths = [j.result() for j in jobs]
        if video is not None:
            os.makedirs(vdir or ".", exist_ok=True)
            size = next(iter(sizes))
            vids = [write_avi(os.path.join(vdir, name.format(stem)), jpegs[k], size, fps)
                    for k, name in zip(("rgb", "depth", "cdepth"), VIDEO_NAMES)]
            return {"png": paths, "video": vids}
        if out_dir is None:
            return frames
        return paths
    finally:
        if pool is not None:
            pool.shutdown(wait=True)


def render_set(model_path: str, name: str, iteration, cameras: Sequence, model, bg: torch.Tensor, *,
               batch: int = MAX_BATCH) -> str:
    """render.py's render_set: <model_path>/<name>/ours_<iteration>/{renders,gt}/%05d.png (the tree metrics.py reads).
    Renders in batches on the device, quantises renders and ground truths there; -> the ours_<iteration> directory."""
    from . import evaluate
    base = os.path.join(model_path, name, "ours_{}".format(iteration))
    rdir, gdir = os.path.join(base, "renders"), os.path.join(base, "gt")
    os.makedirs(rdir, exist_ok=True)
    os.makedirs(gdir, exist_ok=True)
    jobs = []
    with ThreadPoolExecutor(max_workers=PNG_THREADS) as pool, torch.no_grad():
        for idx, imgs in evaluate._batches(model, cameras, bg, batch):
            q = quantize_rgb(list(imgs) + [cameras[i].original_image[0:3] for i in idx])
            host = torch.stack(q).cpu()
            for j, i in enumerate(idx):
                jobs.append(pool.submit(write_png, os.path.join(rdir, "{0:05d}.png".format(i)), host[j]))
                jobs.append(pool.submit(write_png, os.path.join(gdir, "{0:05d}.png".format(i)), host[len(idx) + j]))
        for j in jobs:
            j.result()
    return base
