"""Dataset folders on the host (numpy + stdlib): what scene/dataset_readers.py and scene/colmap_loader.py of the reference read.

    COLMAP    <src>/sparse/0/{cameras,images,points3D}.bin (struct-packed), or the .txt files when a .bin cannot be read;
              SIMPLE_PINHOLE and PINHOLE cameras only
    Blender   <src>/transforms_train.json, transforms_test.json (NeRF synthetic)
    splits    LLFF: every 8th view (sorted by name) is a test view, `n_views` evenly spaced ones of the rest train;
              DTU: two fixed index lists; Blender: eight fixed train views, every 8th test frame
    extent    1.1 x the largest distance of a train camera from their mean centre (`cameras_extent`), `translate`
    points    the sparse-view rule of the reference reads keypoints_to_3d/<dataset>[_<suffix>]/<scene>_keypoints_to_3d.ply,
              relative to the working directory: the dense matcher's cloud, which keypoints_to_3d.py writes from a file of
              keypoint matches.  `init_points`: "matcher" (that rule), "sparse" (COLMAP's own points), or a path.

Images are only located and measured here; read_image() decodes one to uint8 [H, W, C] at its source size (PNG with the
stdlib reader of frames.py, anything else with Pillow when it is installed).  Nothing is resized on the host:
ground_truth.prepare_ground_truth does that on the device.
"""
from __future__ import annotations

import json
import os
import struct
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from .camera import focal2fov, fov2focal, world_to_view

LLFF_HOLD = 8
DTU_TRAIN = (25, 22, 28, 40, 44, 48, 0, 8, 13)
DTU_TEST = (1, 2, 9, 10, 11, 12, 14, 15, 23, 24, 26, 27, 29, 30, 31, 32, 33, 34, 35, 41, 42, 43, 45, 46, 47)
BLENDER_TRAIN = (2, 16, 26, 55, 73, 76, 86, 93)
BLENDER_HOLD = 8
# COLMAP's camera model ids -> (name, parameter count); only the first two can be used (undistorted images)
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
INIT_POINTS_HELP = ('init_points is "matcher" (keypoints_to_3d/<dataset>[_<suffix>]/<scene>_keypoints_to_3d.ply under the working '
                    'directory, the dense matcher\'s cloud), "sparse" (<source>/sparse/0/points3D.ply|.bin|.txt) or the path of a PLY file.  '
                    'The matcher cloud is written by `python -m binocular3dgs_amd.keypoints_to_3d --data_path <source> --matches FILE.npz`, '
                    'or without a match file by `... --data_path <source> --matcher sweep` (the plane-sweep matcher, not the reference\'s network)')


class CameraInfo(NamedTuple):
    uid: int
    R: np.ndarray            # camera-to-world rotation (the W2C rotation transposed)
    T: np.ndarray            # W2C translation
    FovY: float
    FovX: float
    image_path: str
    image_name: str
    width: int
    height: int


class SceneInfo(NamedTuple):
    points: Optional[np.ndarray]       # [P,3] float32
    colors: Optional[np.ndarray]       # [P,3] float32 in [0,1]
    train_cameras: List[CameraInfo]
    test_cameras: List[CameraInfo]
    radius: float
    translate: np.ndarray
    ply_path: str


class PointCloud(NamedTuple):
    points: np.ndarray
    colors: np.ndarray


# ---- COLMAP files --------------------------------------------------------------------------------------------------------
def _unpack(fp, fmt: str):
    return struct.unpack("<" + fmt, fp.read(struct.calcsize("<" + fmt)))


def read_cameras_bin(path: str) -> dict:
    """{camera id: (model name, width, height, params float64)}"""
    cams = {}
    with open(path, "rb") as fp:
        for _ in range(_unpack(fp, "Q")[0]):
            cid, model, w, h = _unpack(fp, "iiQQ")
            name, n = COLMAP_MODELS[model]
            cams[cid] = (name, w, h, np.array(_unpack(fp, "d" * n)))
    return cams


def read_cameras_txt(path: str) -> dict:
    cams = {}
    with open(path) as fp:
        for line in fp:
            line = line.strip()
            if line and not line.startswith("#"):
                t = line.split()
                cams[int(t[0])] = (t[1], int(t[2]), int(t[3]), np.array(tuple(map(float, t[4:]))))
    return cams


def read_images_bin(path: str) -> dict:
    """{image id: (qvec [4], tvec [3], camera id, name)} in file order (the 2D points are skipped)"""
    images = {}
    with open(path, "rb") as fp:
        for _ in range(_unpack(fp, "Q")[0]):
            rec = _unpack(fp, "idddddddi")
            name = bytearray()
            while True:
                ch = fp.read(1)
                if ch in (b"\x00", b""):
                    break
                name += ch
            fp.seek(24 * _unpack(fp, "Q")[0], os.SEEK_CUR)
            images[rec[0]] = (np.array(rec[1:5]), np.array(rec[5:8]), rec[8], name.decode("utf-8"))
    return images


def read_images_txt(path: str) -> dict:
    images = {}
    with open(path) as fp:
        while True:
            line = fp.readline()
            if not line:
                break
            line = line.strip()
            if line and not line.startswith("#"):
                t = line.split()
                images[int(t[0])] = (np.array(tuple(map(float, t[1:5]))), np.array(tuple(map(float, t[5:8]))), int(t[8]), t[9])
                fp.readline()                       # the 2D points of this image
    return images


def read_points3d_bin(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> xyz [P,3] float64, rgb [P,3] float64 (0..255)"""
    with open(path, "rb") as fp:
        n = _unpack(fp, "Q")[0]
        xyz, rgb = np.empty((n, 3)), np.empty((n, 3))
        for i in range(n):
            rec = _unpack(fp, "QdddBBBd")
            xyz[i], rgb[i] = rec[1:4], rec[4:7]
            fp.seek(8 * _unpack(fp, "Q")[0], os.SEEK_CUR)
    return xyz, rgb


def read_points3d_txt(path: str) -> Tuple[np.ndarray, np.ndarray]:
    xyz, rgb = [], []
    with open(path) as fp:
        for line in fp:
            line = line.strip()
            if line and not line.startswith("#"):
                t = line.split()
                xyz.append(tuple(map(float, t[1:4])))
                rgb.append(tuple(map(int, t[4:7])))
    return np.array(xyz, dtype=np.float64).reshape(-1, 3), np.array(rgb, dtype=np.float64).reshape(-1, 3)


def quaternion_to_rotation(q) -> np.ndarray:
    """COLMAP's (w, x, y, z) quaternion as a rotation matrix (float64)"""
    w, x, y, z = q
    return np.array([[1 - 2 * y**2 - 2 * z**2, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x**2 - 2 * z**2, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x**2 - 2 * y**2]])


# ---- point clouds ---------------------------------------------------------------------------------------------------------
def write_point_ply(path: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """x y z nx ny nz (float, normals zero) red green blue (uchar), binary little endian: the file the reference leaves next
    to points3D.bin the first time it opens a scene."""
    n = xyz.shape[0]
    rec = np.zeros(n, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, k]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    head += [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")]
    head += [f"property uchar {p}" for p in ("red", "green", "blue")] + ["end_header"]
    with open(path, "wb") as fp:
        fp.write(("\n".join(head) + "\n").encode("ascii"))
        fp.write(rec.tobytes())


def matcher_ply_path(source_path: str, dataset_name: str, suffix: Optional[str]) -> str:
    scene = os.path.basename(source_path)
    folder = f"{dataset_name}_{suffix}" if suffix is not None else dataset_name
    return f"keypoints_to_3d/{folder}/{scene}_keypoints_to_3d.ply"


def _colmap_points(source_path: str, init_points: str, sparse_view: bool, dataset_name: str, suffix) -> str:
    """The PLY file the initial points come from (written from points3D.bin / .txt when it is the sparse one and missing)."""
    sparse = os.path.join(source_path, "sparse/0/points3D.ply")
    if init_points == "matcher":
        path = matcher_ply_path(source_path, dataset_name, suffix) if sparse_view else sparse
    elif init_points == "sparse":
        path = sparse
    else:
        path = init_points
    if path == sparse and not os.path.exists(path):
        for name, reader in (("points3D.bin", read_points3d_bin), ("points3D.txt", read_points3d_txt)):
            src = os.path.join(source_path, "sparse/0", name)
            if os.path.exists(src):
                xyz, rgb = reader(src)
                write_point_ply(path, xyz, rgb)
                break
    if not os.path.exists(path):
        raise FileNotFoundError(f"initial points: {path} does not exist.  {INIT_POINTS_HELP}")
    return path


# ---- images ---------------------------------------------------------------------------------------------------------------
def image_size(path: str) -> Tuple[int, int]:
    """(width, height) without decoding the pixels"""
    if path.lower().endswith(".png"):
        from .frames import png_size
        return tuple(int(v) for v in png_size(path))
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError(f"{path}: only PNG files are read without Pillow, and Pillow is not installed") from e
    with Image.open(path) as im:
        return im.size


def read_image(path: str) -> np.ndarray:
    """uint8 [H,W] / [H,W,3] / [H,W,4] at the file's own size.  Gray + alpha is expanded to RGBA."""
    if path.lower().endswith(".png"):
        from .frames import read_png
        a = read_png(path)
    else:
        try:
            from PIL import Image
        except ImportError as e:
            raise RuntimeError(f"{path}: only PNG files are read without Pillow, and Pillow is not installed") from e
        with Image.open(path) as im:
            if im.mode not in ("L", "LA", "RGB", "RGBA"):
                im = im.convert("RGBA" if "A" in im.mode or "transparency" in im.info else "RGB")
            a = np.array(im)
    if a.ndim == 3 and a.shape[2] == 2:
        a = np.concatenate([np.repeat(a[..., :1], 3, axis=2), a[..., 1:]], axis=2)
    return np.ascontiguousarray(a)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def camera_extent(cams: List[CameraInfo]) -> Tuple[float, np.ndarray]:
    """-> (radius, translate): 1.1 x the largest distance of a camera centre from the mean centre, and minus that mean"""
    centers = np.hstack([np.linalg.inv(world_to_view(c.R, c.T))[:3, 3:4] for c in cams])
    mean = np.mean(centers, axis=1, keepdims=True)
    diagonal = np.max(np.linalg.norm(centers - mean, axis=0, keepdims=True))
    return diagonal * 1.1, -mean.flatten()


def _colmap_cameras(source_path: str, images: str) -> List[CameraInfo]:
    sparse = os.path.join(source_path, "sparse/0")
    try:
        extr = read_images_bin(os.path.join(sparse, "images.bin"))
        intr = read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    except (OSError, struct.error, KeyError):
        extr = read_images_txt(os.path.join(sparse, "images.txt"))
        intr = read_cameras_txt(os.path.join(sparse, "cameras.txt"))
    out = []
    for q, t, cam_id, name in extr.values():
        model, width, height, params = intr[cam_id]
        if model == "SIMPLE_PINHOLE":
            fx = fy = params[0]
        elif model == "PINHOLE":
            fx, fy = params[0], params[1]
        else:
            raise ValueError(f"COLMAP camera model {model} of camera {cam_id}: only undistorted datasets (SIMPLE_PINHOLE or "
                             "PINHOLE cameras) are supported.  `python -m binocular3dgs_amd.undistort -s SRC -o DST` writes one")
        path = os.path.join(source_path, images, os.path.basename(name))
        out.append(CameraInfo(uid=cam_id, R=np.transpose(quaternion_to_rotation(q)), T=np.array(t),
                              FovY=focal2fov(fy, height), FovX=focal2fov(fx, width), image_path=path,
                              image_name=os.path.basename(path).split(".")[0], width=width, height=height))
    return sorted(out, key=lambda c: c.image_name)


def read_colmap_scene(source_path: str, images: Optional[str] = "images", eval: bool = True, n_views: int = 3,
                      dataset_name: str = "LLFF", suffix: Optional[str] = None, init_points: str = "matcher") -> SceneInfo:
    cams = _colmap_cameras(source_path, "images" if images is None else images)
    sparse_view = bool(eval) and n_views > 0
    if sparse_view:
        if dataset_name == "DTU":
            train = [cams[i] for i in DTU_TRAIN][:n_views]
            test = [cams[i] for i in DTU_TEST]
        elif dataset_name == "LLFF":
            rest = [c for i, c in enumerate(cams) if i % LLFF_HOLD != 0]
            test = [c for i, c in enumerate(cams) if i % LLFF_HOLD == 0]
            keep = [round(i) for i in np.linspace(0, len(rest) - 1, n_views)]
            train = [c for i, c in enumerate(rest) if i in keep]
        else:
            raise NotImplementedError(dataset_name)
    else:
        train, test = cams, []
    radius, translate = camera_extent(train)
    ply = _colmap_points(source_path, init_points, sparse_view, dataset_name, suffix)
    from .init_points import fetch_point_cloud
    pts, rgb = fetch_point_cloud(ply)
    return SceneInfo(pts, rgb, train, test, radius, translate, ply)


def _blender_cameras(source_path: str, transforms: str, extension: str = ".png") -> List[CameraInfo]:
    with open(os.path.join(source_path, transforms)) as fp:
        meta = json.load(fp)
    fovx = meta["camera_angle_x"]
    out = []
    for idx, frame in enumerate(meta["frames"]):
        path = os.path.join(source_path, frame["file_path"] + extension)
        c2w = np.array(frame["transform_matrix"])
        c2w[:3, 1:3] *= -1                       # Blender / OpenGL axes (y up, z back) -> COLMAP's (y down, z forward)
        w2c = np.linalg.inv(c2w)
        width, height = image_size(path)
        out.append(CameraInfo(uid=idx, R=np.transpose(w2c[:3, :3]), T=w2c[:3, 3],
                              FovY=focal2fov(fov2focal(fovx, width), height), FovX=fovx, image_path=path,
                              image_name=os.path.splitext(os.path.basename(path))[0], width=width, height=height))
    return out


def read_blender_scene(source_path: str, eval: bool = True, n_views: int = 3, dataset_name: str = "Blender",
                       init_points: str = "matcher", extension: str = ".png") -> SceneInfo:
    train = _blender_cameras(source_path, "transforms_train.json", extension)
    test = _blender_cameras(source_path, "transforms_test.json", extension)
    if eval and n_views > 0:
        if dataset_name != "Blender":
            raise NotImplementedError(dataset_name)
        train = [train[i] for i in BLENDER_TRAIN]
        test = [c for i, c in enumerate(test) if i % BLENDER_HOLD == 0]
    if not eval:
        train, test = train + test, []
    radius, translate = camera_extent(train)
    ply = os.path.join(source_path, "points3d.ply") if init_points in ("matcher", "sparse") else init_points
    if init_points in ("matcher", "sparse") and not os.path.exists(ply):
        # no reconstruction comes with this dataset: random points inside the bounds of the synthetic scenes, dark colours
        n = 100_000
        xyz = np.random.random((n, 3)) * 2.6 - 1.3
        shs = np.random.random((n, 3)) / 255.0
        write_point_ply(ply, xyz, (shs * 0.28209479177387814 + 0.5) * 255)
    if not os.path.exists(ply):
        raise FileNotFoundError(f"initial points: {ply} does not exist.  {INIT_POINTS_HELP}")
    from .init_points import fetch_point_cloud
    pts, rgb = fetch_point_cloud(ply)
    return SceneInfo(pts, rgb, train, test, radius, translate, ply)


def read_scene(source_path: str, *, images: Optional[str] = "images", eval: bool = True, n_views: int = 3,
               dataset_name: str = "LLFF", suffix: Optional[str] = None, init_points: str = "matcher") -> SceneInfo:
    """COLMAP when <source>/sparse exists, Blender when transforms_train.json does (scene/__init__.py:44-50)."""
    if os.path.exists(os.path.join(source_path, "sparse")):
        return read_colmap_scene(source_path, images, eval, n_views, dataset_name, suffix, init_points)
    if os.path.exists(os.path.join(source_path, "transforms_train.json")):
        return read_blender_scene(source_path, eval, n_views, dataset_name, init_points)
    raise ValueError(f"{source_path}: neither a COLMAP (sparse/) nor a Blender (transforms_train.json) dataset")


def camera_json(idx: int, cam: CameraInfo) -> dict:
    """One entry of <model_path>/cameras.json (utils/camera_utils.py camera_to_JSON)"""
    Rt = np.zeros((4, 4))
    Rt[:3, :3] = cam.R.transpose()
    Rt[:3, 3] = cam.T
    Rt[3, 3] = 1.0
    c2w = np.linalg.inv(Rt)
    return {"id": idx, "img_name": cam.image_name, "width": cam.width, "height": cam.height,
            "position": c2w[:3, 3].tolist(), "rotation": [row.tolist() for row in c2w[:3, :3]],
            "fy": fov2focal(cam.FovY, cam.height), "fx": fov2focal(cam.FovX, cam.width)}
