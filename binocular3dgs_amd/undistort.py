"""Undistort a COLMAP dataset on the device: a raw sparse model with SIMPLE_RADIAL, RADIAL, OPENCV, FULL_OPENCV, OPENCV_FISHEYE,
SIMPLE_RADIAL_FISHEYE or RADIAL_FISHEYE cameras plus its images -> a dataset folder dataset_readers.read_scene accepts.

    python -m binocular3dgs_amd.undistort -s SRC -o DST [--images images] [--blank B] [--max_scale S] [--size W H]

What COLMAP's image_undistorter does, with one difference that this code base needs: CameraInfo carries only FovX and FovY, so
the renderer puts the principal point at the image centre, and the cameras written here are exactly that: PINHOLE
(fx, fy, W'/2, H'/2).  The focal lengths are kept, the size follows from where the undistorted image border lies (pinhole_for).

On the device (csrc/undistort.hip, three entry points added to ABI 18): the camera models in fp64 (distort_points,
undistort_points: Newton's iteration with a per-point `converged` byte), the map from the output pinhole into the source as
int32 pairs with 8 fractional bits (undistort_map, one per distinct camera), and the integer bilinear resampling of up to 8
uint8 images per launch through one map (remap), with a `valid` plane.  On the host: reading and writing COLMAP's binary files,
decoding the sources and zlib for the PNG files.  tests/undistort_ref.py is the numpy statement of all of it.

2-D match files computed on the distorted images are not converted: compute them again on DST.
"""
from __future__ import annotations

import os
import shutil
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .dataset_readers import COLMAP_MODELS

MAX_BATCH = 8            # images per b3gs_remap_batch (B3GS_MAX_REMAP_VIEWS)
SUPPORTED_MODELS = ("SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE")
_MODEL_IDS = {name: (mid, n) for mid, (name, n) in COLMAP_MODELS.items()}


@dataclass(frozen=True)
class CameraModel:
    """One COLMAP camera: model name, image size, parameters in COLMAP's order (float64)."""
    name: str
    width: int
    height: int
    params: Tuple[float, ...]

    def __post_init__(self):
        if self.name not in SUPPORTED_MODELS:
            raise ValueError(f"camera model {self.name} cannot be undistorted: supported are {', '.join(SUPPORTED_MODELS)}")
        p = tuple(float(v) for v in np.asarray(self.params, dtype=np.float64).reshape(-1))
        if len(p) != _MODEL_IDS[self.name][1]:
            raise ValueError(f"camera model {self.name} has {_MODEL_IDS[self.name][1]} parameters, not {len(p)}")
        if int(self.width) < 1 or int(self.height) < 1:
            raise ValueError("the image size of a camera is at least 1 x 1")
        object.__setattr__(self, "params", p)
        object.__setattr__(self, "width", int(self.width))
        object.__setattr__(self, "height", int(self.height))

    @property
    def model_id(self) -> int:
        return _MODEL_IDS[self.name][0]

    @property
    def one_focal(self) -> bool:
        return len(self.params) in (4, 5)

    @property
    def focal(self) -> Tuple[float, float]:
        return (self.params[0], self.params[0]) if self.one_focal else (self.params[0], self.params[1])

    @property
    def principal(self) -> Tuple[float, float]:
        return (self.params[1], self.params[2]) if self.one_focal else (self.params[2], self.params[3])


def scaled_to(cam: CameraModel, width: int, height: int) -> CameraModel:
    """The camera of the same lens for images of another size (LLFF's images_4): fx, cx scale with the width, fy, cy with the
    height, the distortion coefficients stay.  The single focal length of a one-focal model scales with the width."""
    width, height = int(width), int(height)
    if (width, height) == (cam.width, cam.height):
        return cam
    sx, sy = width / cam.width, height / cam.height
    p = list(cam.params)
    if cam.one_focal:
        p[0], p[1], p[2] = p[0] * sx, p[1] * sx, p[2] * sy
    else:
        p[0], p[1], p[2], p[3] = p[0] * sx, p[1] * sy, p[2] * sx, p[3] * sy
    return CameraModel(cam.name, width, height, tuple(p))


# ---- the three launches ------------------------------------------------------------------------------------------------------
def _points(cam: CameraModel, xy, inverse: bool, device):
    from . import _C
    t = xy if isinstance(xy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(xy, dtype=np.float64)))
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("points are [n,2] pixel coordinates")
    if t.device.type != "cuda":
        t = t.to(torch.device(device or "cuda"))
    return _C.camera_points(cam.model_id, cam.width, cam.height, list(cam.params), t.to(torch.float64), bool(inverse))


def distort_points(cam: CameraModel, xy, device=None) -> torch.Tensor:
    """Pixel coordinates of the ideal pinhole (fx, fy, cx, cy of `cam`) -> where the lens puts them; float64 [n,2] on the device."""
    return _points(cam, xy, False, device)[0]


def undistort_points(cam: CameraModel, xy, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The inverse -> (float64 [n,2], converged uint8 [n]); a point that did not converge comes back unchanged."""
    return _points(cam, xy, True, device)


def _border_centres(width: int, height: int) -> List[np.ndarray]:
    ys, xs = np.arange(height, dtype=np.float64) + 0.5, np.arange(width, dtype=np.float64) + 0.5
    return [np.stack([np.full(height, 0.5), ys], axis=1), np.stack([np.full(height, width - 0.5), ys], axis=1),
            np.stack([xs, np.full(width, 0.5)], axis=1), np.stack([xs, np.full(width, height - 0.5)], axis=1)]


def pinhole_for(cam: CameraModel, blank: float = 0.0, max_scale: float = 2.0, size: Optional[Tuple[int, int]] = None,
                device="cuda") -> Tuple[int, int, float, float]:
    """(W', H', fx, fy) of the output pinhole, principal point at (W'/2, H'/2).  The focal lengths are the camera's.  Without
    `size`: the centres of all border pixels are undistorted (one launch, one host read); per side, `inner` is the bound all of
    them reach and `outer` the one the farthest of them reaches; blank = 0 keeps the inner rectangle (no blank pixel), blank = 1
    the outer one (no source pixel lost); the half extent about the optical axis is the smaller of the two sides' and the size is
    clamped to max_scale times the source's."""
    fx, fy = cam.focal
    cx, cy = cam.principal
    if size is not None:
        W, H = int(size[0]), int(size[1])
        if W < 1 or H < 1:
            raise ValueError("size is at least 1 x 1")
        return W, H, fx, fy
    sides = _border_centres(cam.width, cam.height)
    out, conv = undistort_points(cam, np.concatenate(sides), device)
    out, conv = out.cpu().numpy(), conv.cpu().numpy().astype(bool)        # (the default stream: this copy waits for the launch)
    bounds, start = [], 0
    for k, pts in enumerate(sides):
        sl = slice(start, start + len(pts))
        start += len(pts)
        if not conv[sl].any():
            raise ValueError("no border pixel of one side of the image can be undistorted: give size=(W, H)")
        p = out[sl][conv[sl]]
        bounds.append((p[:, 0] - cx) / fx if k < 2 else (p[:, 1] - cy) / fy)
    lu, ru, tv, bv = bounds
    left = (1 - blank) * lu.max() + blank * lu.min()
    right = (1 - blank) * ru.min() + blank * ru.max()
    top = (1 - blank) * tv.max() + blank * tv.min()
    bottom = (1 - blank) * bv.min() + blank * bv.max()
    half_u, half_v = min(-left, right), min(-top, bottom)
    if not (half_u > 0 and half_v > 0):
        raise ValueError("the undistorted image does not contain the optical axis: give size=(W, H)")
    W = min(max(int(np.floor(2 * fx * half_u)), 1), int(round(max_scale * cam.width)))
    H = min(max(int(np.floor(2 * fy * half_v)), 1), int(round(max_scale * cam.height)))
    return W, H, fx, fy


def undistort_map(cam: CameraModel, pinhole: Tuple[int, int, float, float], device="cuda") -> torch.Tensor:
    """int32 [H', W', 2] on the device: where the centre of every pixel of the pinhole lies in the source, pixel centres at
    integers, 8 fractional bits."""
    from . import _C
    W, H, fx, fy = pinhole
    return _C.undistort_map(cam.model_id, cam.width, cam.height, list(cam.params), int(W), int(H), float(fx), float(fy),
                            torch.device(device))


def _as_image(img) -> torch.Tensor:
    if not isinstance(img, torch.Tensor):
        a = np.ascontiguousarray(img)
        img = torch.from_numpy(a if a.flags.writeable else a.copy())
    t = img
    if t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError("an image is uint8 [H, W, C] or [H, W]")
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.shape[2] not in (1, 3, 4):
        raise ValueError(f"1, 3 or 4 channels, not {t.shape[2]}")
    return t


def remap(images: Sequence, map: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 images [Hs, Ws, C] of one size (numpy / CPU tensors are uploaded) through one map -> (uint8 [n, H', W', C], valid uint8
    [H', W']) on the map's device; more than 8 images go as several launches of 8."""
    from . import _C
    imgs = [_as_image(i) for i in images]
    if not imgs:
        raise ValueError("remap needs at least one image")
    if any(i.shape != imgs[0].shape for i in imgs):
        raise ValueError("the images of one remap call have one size")
    if not isinstance(map, torch.Tensor) or map.dtype != torch.int32 or map.dim() != 3 or map.shape[2] != 2:
        raise ValueError("the map is an int32 [H, W, 2] tensor")
    dev = map.device
    outs, valid = [], None
    for b in range(0, len(imgs), MAX_BATCH):
        part = [i if i.device == dev else i.to(dev, non_blocking=True) for i in imgs[b:b + MAX_BATCH]]
        out, v = _C.remap(part, map)
        outs.append(out)
        valid = v if valid is None else valid
    return (outs[0] if len(outs) == 1 else torch.cat(outs)), valid


# ---- COLMAP's binary files ------------------------------------------------------------------------------------------------------
def write_cameras_bin(path: str, cameras: Dict[int, tuple]) -> None:
    """{camera id: (model name, width, height, params)}, what dataset_readers.read_cameras_bin returns"""
    ids = {name: mid for mid, (name, _) in COLMAP_MODELS.items()}
    with open(path, "wb") as fp:
        fp.write(struct.pack("<Q", len(cameras)))
        for cid, (name, w, h, params) in cameras.items():
            p = [float(v) for v in np.asarray(params, dtype=np.float64).reshape(-1)]
            if name not in ids or len(p) != COLMAP_MODELS[ids[name]][1]:
                raise ValueError(f"camera {cid}: model {name} with {len(p)} parameters is not one of COLMAP's")
            fp.write(struct.pack("<iiQQ", int(cid), ids[name], int(w), int(h)) + struct.pack(f"<{len(p)}d", *p))


def write_images_bin(path: str, images: Dict[int, tuple]) -> None:
    """{image id: (qvec [4], tvec [3], camera id, name[, xys float64 [n,2], point3D ids int64 [n]])}: what
    dataset_readers.read_images_bin returns, optionally with the 2-D points it skips"""
    with open(path, "wb") as fp:
        fp.write(struct.pack("<Q", len(images)))
        for iid, rec in images.items():
            q, t, cid, name = rec[:4]
            xys = np.asarray(rec[4], dtype=np.float64).reshape(-1, 2) if len(rec) > 4 else np.zeros((0, 2))
            pid = np.asarray(rec[5], dtype=np.int64).reshape(-1) if len(rec) > 5 else np.full(len(xys), -1, dtype=np.int64)
            if len(pid) != len(xys):
                raise ValueError(f"image {iid}: one point3D id per 2-D point")
            fp.write(struct.pack("<i7di", int(iid), *[float(v) for v in q], *[float(v) for v in t], int(cid)))
            fp.write(name.encode("utf-8") + b"\x00")
            fp.write(struct.pack("<Q", len(xys)))
            pts = np.zeros(len(xys), dtype=[("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            pts["x"], pts["y"], pts["id"] = xys[:, 0], xys[:, 1], pid
            fp.write(pts.tobytes())


def read_images_bin_full(path: str) -> Dict[int, tuple]:
    """{image id: (qvec, tvec, camera id, name, xys [n,2], point3D ids [n])} in file order"""
    images = {}
    with open(path, "rb") as fp:
        for _ in range(struct.unpack("<Q", fp.read(8))[0]):
            rec = struct.unpack("<i7di", fp.read(64))
            name = bytearray()
            while True:
                ch = fp.read(1)
                if ch in (b"\x00", b""):
                    break
                name += ch
            n = struct.unpack("<Q", fp.read(8))[0]
            pts = np.frombuffer(fp.read(24 * n), dtype=[("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            images[rec[0]] = (np.array(rec[1:5]), np.array(rec[5:8]), rec[8], name.decode("utf-8"),
                              np.stack([pts["x"], pts["y"]], axis=1), pts["id"].copy())
    return images


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
def _read_sparse(sparse: str):
    from . import dataset_readers as dr
    try:
        return read_images_bin_full(os.path.join(sparse, "images.bin")), dr.read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    except (OSError, struct.error, KeyError):
        extr = {k: v + (np.zeros((0, 2)), np.zeros(0, dtype=np.int64)) for k, v in dr.read_images_txt(os.path.join(sparse, "images.txt")).items()}
        return extr, dr.read_cameras_txt(os.path.join(sparse, "cameras.txt"))


def undistort_dataset(src: str, dst: str, images: str = "images", blank: float = 0.0, max_scale: float = 2.0, device="cuda",
                      size: Optional[Tuple[int, int]] = None) -> Dict[int, Tuple[int, int, float, float]]:
    """Writes dst/<images>/<name>.png (RGB; gray is repeated, alpha is dropped), dst/sparse/0/cameras.bin (PINHOLE, principal
    point at the centre), dst/sparse/0/images.bin (same ids and poses, names ending in .png, 2-D points undistorted) and copies
    every other file of src/sparse/0 and the top-level files of src.  One map per distinct camera.  -> {camera id: pinhole}."""
    from . import dataset_readers as dr
    from .frames import write_png
    if os.path.abspath(src) == os.path.abspath(dst):
        raise ValueError("the output folder must not be the source folder")
    sparse = os.path.join(src, "sparse/0")
    extr, intr = _read_sparse(sparse)
    by_cam: Dict[int, List[int]] = {}
    for iid, rec in extr.items():
        by_cam.setdefault(rec[2], []).append(iid)
    cams = {cid: CameraModel(*intr[cid]) for cid in by_cam}               # (an unsupported model is refused by name here)
    os.makedirs(os.path.join(dst, images), exist_ok=True)
    os.makedirs(os.path.join(dst, "sparse/0"), exist_ok=True)
    pinholes: Dict[int, Tuple[int, int, float, float]] = {}
    new_cams, new_images = {}, {}
    for cid, ids in by_cam.items():
        cam = cams[cid]
        paths = [os.path.join(src, images, os.path.basename(extr[i][3])) for i in ids]
        wi, hi = dr.image_size(paths[0])
        scam = scaled_to(cam, wi, hi)
        W, H, fx, fy = pinholes[cid] = pinhole_for(scam, blank, max_scale, size, device)
        new_cams[cid] = ("PINHOLE", W, H, (fx, fy, W / 2, H / 2))
        m = undistort_map(scam, pinholes[cid], device)
        for b in range(0, len(ids), MAX_BATCH):
            part = []
            for p in paths[b:b + MAX_BATCH]:
                a = dr.read_image(p)
                if a.shape[:2] != (hi, wi):
                    raise ValueError(f"{p}: {a.shape[1]} x {a.shape[0]}, but the other images of camera {cid} are {wi} x {hi}")
                part.append(a if a.ndim == 3 else a[:, :, None])
            # (images of one camera with different channel counts go as separate launches)
            for C in sorted({a.shape[2] for a in part}):
                sel = [k for k, a in enumerate(part) if a.shape[2] == C]
                out = remap([part[k] for k in sel], m)[0].cpu().numpy()
                for k, o in zip(sel, out):
                    rgb = np.repeat(o, 3, axis=2) if C == 1 else o[:, :, :3]
                    name = os.path.splitext(os.path.basename(paths[b + k]))[0] + ".png"
                    write_png(os.path.join(dst, images, name), np.ascontiguousarray(rgb))
        # the 2-D points, in the units of cameras.bin -> the output pinhole
        (fxc, fyc), (cxc, cyc) = cam.focal, cam.principal
        counts = [len(extr[i][4]) for i in ids]
        allxy = np.concatenate([extr[i][4] for i in ids]) if sum(counts) else np.zeros((0, 2))
        if len(allxy):
            und = undistort_points(cam, allxy, device)[0].cpu().numpy()
            allxy = np.stack([(und[:, 0] - cxc) / fxc * fx + W / 2, (und[:, 1] - cyc) / fyc * fy + H / 2], axis=1)
        start = 0
        for i, n in zip(ids, counts):
            q, t, _, name = extr[i][:4]
            new_images[i] = (q, t, cid, os.path.splitext(name)[0] + ".png", allxy[start:start + n], extr[i][5])
            start += n
    write_cameras_bin(os.path.join(dst, "sparse/0/cameras.bin"), new_cams)
    write_images_bin(os.path.join(dst, "sparse/0/images.bin"), {i: new_images[i] for i in extr})
    for f in sorted(os.listdir(sparse)):
        if f not in ("cameras.bin", "images.bin", "cameras.txt", "images.txt") and os.path.isfile(os.path.join(sparse, f)):
            shutil.copyfile(os.path.join(sparse, f), os.path.join(dst, "sparse/0", f))
    for f in sorted(os.listdir(src)):
        if os.path.isfile(os.path.join(src, f)):
            shutil.copyfile(os.path.join(src, f), os.path.join(dst, f))
    return pinholes


def main(argv=None) -> int:
    import argparse
    p = argparse.ArgumentParser(prog="python -m binocular3dgs_amd.undistort", description=__doc__.split("\n")[0])
    p.add_argument("-s", "--source_path", required=True)
    p.add_argument("-o", "--output_path", required=True)
    p.add_argument("--images", default="images")
    p.add_argument("--blank", type=float, default=0.0, help="0: no blank pixel in the output; 1: no source pixel lost")
    p.add_argument("--max_scale", type=float, default=2.0, help="the output is at most this many times the source's size")
    p.add_argument("--size", type=int, nargs=2, metavar=("W", "H"), default=None, help="the output size, instead of the rule")
    p.add_argument("--device", default="cuda")
    a = p.parse_args(argv)
    pin = undistort_dataset(a.source_path, a.output_path, a.images, a.blank, a.max_scale, a.device, tuple(a.size) if a.size else None)
    for cid, (W, H, fx, fy) in pin.items():
        print(f"camera {cid}: PINHOLE {W} x {H}, fx {fx:.3f}, fy {fy:.3f}")
    print(f"wrote {a.output_path}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
