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


# ---- drivers -----------------------------------------------------------------------------------------------------------
def render_path(model, cameras: Sequence, bg: torch.Tensor, out_dir: Optional[str] = None, *, batch: int = MAX_BATCH,
                percentile: float = 99.):
    """spiral.py's render_set: every camera rendered (up to `batch` <= 8 views of one W x H per launch, evaluation's renderer)
    and encoded on the device.
    out_dir None: -> per camera {"rgb", "depth", "cdepth"} uint8 [H,W,3] device tensors.
    out_dir set:  writes %05d.png, depth_%05d.png, cdepth_%05d.png (camera index) there, one device->host copy per batch
                  and at most PNG_THREADS writer threads; -> the written paths in camera order."""
    from . import evaluate
    frames: List[Optional[dict]] = [None] * len(cameras)
    pool = ThreadPoolExecutor(max_workers=PNG_THREADS) if out_dir is not None else None
    jobs = []
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    try:
        with torch.no_grad():
            for idx, outs in evaluate._batches(model, cameras, bg, batch, full=True):
                enc = encode_frames([o["render"] for o in outs], [o["rendered_depth"] for o in outs],
                                    [o["rendered_alpha"] for o in outs], percentile=percentile)
                if pool is None:
                    for j, i in enumerate(idx):
                        frames[i] = {k: enc[k][j] for k in ("rgb", "depth", "cdepth")}
                    continue
                host = torch.stack([torch.stack(enc[k]) for k in ("rgb", "depth", "cdepth")]).cpu()   # one copy per batch
                for j, i in enumerate(idx):
                    for k, name in enumerate(("{:05d}.png", "depth_{:05d}.png", "cdepth_{:05d}.png")):
                        jobs.append(pool.submit(write_png, os.path.join(out_dir, name.format(i)), host[k, j]))
        if pool is None:
            return frames
        return [j.result() for j in jobs]
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
