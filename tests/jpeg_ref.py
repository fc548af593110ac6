"""The baseline JPEG encoder of csrc/jpeg.hip restated in numpy: the written definition of its integer arithmetic, and the
seeded images the JPEG tests use.  numpy only; nothing here imports the package.

One frame = header(W, H, quality) + scan(image, quality) + EOI, where the scan is what the device writes:

  colour   Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16                       (16-bit fixed point, the IJG constants)
           Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
           Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
  edges    the image is replicated to the right and downwards to a multiple of 16 (whole MCUs)
  chroma   2 x 2 average (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... along every output row (starting at 1)
  DCT      on sample - 128: the 13-bit Loeffler-Ligtenberg-Moschytz integer transform, rows then columns, 2 extra bits between
           the passes, output scaled by 8 ("slow integer" DCT)
  quantise sign(c) * ((|c| + 4 q) // (8 q)) with q the table entry: rounding division by the 8-times scaled entry
  tables   Annex K scaled by the IJG quality rule, clamped to 1..255
  entropy  Annex K "typical" Huffman tables, one interleaved scan (Y00 Y01 Y10 Y11 Cb Cr per MCU), no restart markers,
           0xFF stuffed with 0x00, the last byte padded with 1-bits
"""
import struct

import numpy as np

# ---- tables ------------------------------------------------------------------------------------------------------------
LUMA_Q50 = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA_Q50 = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99], dtype=np.int64).reshape(8, 8)


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, dtype=np.int64)


ZIGZAG = _zigzag()          # ZIGZAG[k] = row-major index of the k-th coefficient of the scan order

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
    "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))


def huff_codes(bits, vals):
    """symbol -> (code, length): the canonical assignment of Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
AC_CODES = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def tables(quality):
    """The two 8 x 8 quantisation tables (row-major) of a quality 1..100."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (LUMA_Q50, CHROMA_Q50))


def header(W, H, quality):
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, SOS."""
    seg = lambda marker, body: struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body  # noqa: E731
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate(tables(quality)):
        out += seg(0xDB, bytes([i]) + bytes(int(x) for x in t.reshape(-1)[ZIGZAG]))
    out += seg(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def ycbcr420(img):
    """uint8 [H,W,3] -> Y [H16,W16], Cb, Cr [H16/2,W16/2] (int64), edges replicated to whole MCUs."""
    H, W, _ = img.shape
    a = np.pad(np.asarray(img, dtype=np.int64), ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge")
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16

    def down(c):
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        bias = 1 + (np.arange(s.shape[1]) & 1)
        return (s + bias[None, :]) >> 2
    return y, down(cb), down(cr)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first):
    """One pass of the slow-integer DCT along the last axis of [..., 8]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15                          # CONST_BITS - PASS1_BITS, CONST_BITS + PASS1_BITS
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct(blocks):
    """[..., 8, 8] samples (already minus 128) -> coefficients scaled by 8."""
    rows = _dct_pass(np.asarray(blocks, dtype=np.int64), True)
    return np.swapaxes(_dct_pass(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantise(coef, table):
    q8 = 8 * np.asarray(table, dtype=np.int64)
    return np.sign(coef) * ((np.abs(coef) + (q8 >> 1)) // q8)


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)        # [by, bx, 8, 8]


def coefficients(img, quality):
    """-> int64 [n_mcu, 6, 64]: quantised coefficients in scan order (zigzag), MCUs row by row, Y00 Y01 Y10 Y11 Cb Cr."""
    ql, qc = tables(quality)
    y, cb, cr = ycbcr420(img)
    qy = quantise(fdct(_blocks(y - 128)), ql)
    qb, qr = quantise(fdct(_blocks(cb - 128)), qc), quantise(fdct(_blocks(cr - 128)), qc)
    mh, mw = qb.shape[:2]
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, :, j] = qy[dy::2, dx::2].reshape(mh, mw, 64)[..., ZIGZAG]
    out[:, :, 4] = qb.reshape(mh, mw, 64)[..., ZIGZAG]
    out[:, :, 5] = qr.reshape(mh, mw, 64)[..., ZIGZAG]
    return out.reshape(mh * mw, 6, 64)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.zrl = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def finish(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def _magnitude(v):
    """(size category, the `size` low bits that follow the code) of a value."""
    a = abs(v)
    nbits = a.bit_length()
    return nbits, (v if v >= 0 else v - 1) & ((1 << nbits) - 1)


def scan(img, quality, stats=None):
    """The entropy-coded, byte-stuffed scan of one image.  stats (a dict) receives counts of ZRL codes, EOB codes, the largest
    size category and the stuffed bytes."""
    coef = coefficients(img, quality)
    w = _Bits()
    last = [0, 0, 0]
    n_zrl = n_eob = max_size = 0
    for mcu in coef.tolist():
        for j, blk in enumerate(mcu):
            comp = 0 if j < 4 else j - 3
            tab = 0 if j < 4 else 1
            nbits, extra = _magnitude(blk[0] - last[comp])
            last[comp] = blk[0]
            w.put(*DC_CODES[tab][nbits])
            w.put(extra, nbits)
            max_size = max(max_size, nbits)
            run = 0
            for k in range(1, 64):
                v = blk[k]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    w.put(*AC_CODES[tab][0xF0])
                    n_zrl += 1
                    run -= 16
                nbits, extra = _magnitude(v)
                w.put(*AC_CODES[tab][(run << 4) | nbits])
                w.put(extra, nbits)
                max_size = max(max_size, nbits)
                run = 0
            if run:
                w.put(*AC_CODES[tab][0x00])
                n_eob += 1
    data = w.finish()
    if stats is not None:
        stats.update(zrl=n_zrl, eob=n_eob, max_size=max_size, stuffed=data.count(b"\xff\x00"), blocks=coef.shape[0] * 6)
    return data


def encode(img, quality=90):
    """A complete JPEG file of a uint8 [H,W,3] image."""
    H, W, _ = img.shape
    return header(W, H, quality) + scan(img, quality) + b"\xff\xd9"


def split(jpeg):
    """(header, scan, EOI) of a file `encode` (or the device path) made: the scan starts behind the SOS segment."""
    pos = 2
    while True:
        assert jpeg[pos] == 0xFF, "marker expected"
        marker, (n,) = jpeg[pos + 1], struct.unpack(">H", jpeg[pos + 2:pos + 4])
        pos += 2 + n
        if marker == 0xDA:
            break
    return jpeg[:pos], jpeg[pos:-2], jpeg[-2:]


# ---- seeded images -----------------------------------------------------------------------------------------------------------
def natural(W, H, seed=0):
    """A smooth gradient plus blobs plus mild noise."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([60 + 120 * xx / max(W - 1, 1), 40 + 150 * yy / max(H - 1, 1), 200 - 90 * (xx + yy) / max(W + H - 2, 1)], -1)
    for _ in range(6):
        cx, cy, s = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2.0, 0.2 * max(W, H) + 2.0)
        img += rng.uniform(-90, 90, 3) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))[..., None]
    img += rng.normal(0, 2.0, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def constant(W, H, seed=0):
    rng = np.random.default_rng(seed)
    return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)).copy()


def noise(W, H, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def sparse(W, H, seed=0):
    """Isolated high-frequency speckle on flat ground: some 8 x 8 blocks carry one DCT basis function of a high frequency
    (u, v in 5..7) on all three channels alike, so that a few late coefficients survive behind zero runs >= 16."""
    rng = np.random.default_rng(seed)
    img = np.full((H, W, 3), 128.0)
    k = np.arange(8)
    for by in range(0, H, 8):
        for bx in range(0, W, 8):
            if rng.random() < 0.6:
                u, v, amp = int(rng.integers(5, 8)), int(rng.integers(5, 8)), rng.uniform(40, 110)
                basis = np.outer(np.cos((2 * k + 1) * v * np.pi / 16), np.cos((2 * k + 1) * u * np.pi / 16)) * amp
                h, w = min(8, H - by), min(8, W - bx)
                img[by:by + h, bx:bx + w] += basis[:h, :w, None]
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def full_range(W, H, seed=0):
    """8 x 8 blocks of 0 or 255 per channel: DC differences span the range."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8, 3)).astype(np.uint8) * 255
    return np.repeat(np.repeat(b, 8, 0), 8, 1)[:H, :W].copy()


GENERATORS = {"constant": constant, "natural": natural, "noise": noise, "sparse": sparse, "full_range": full_range}
