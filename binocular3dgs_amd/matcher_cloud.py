"""The matcher cloud: from keypoint matches to keypoints_to_3d/<dataset>/<scene>_keypoints_to_3d.ply, the initial points of the
sparse-view rule (`--init_points matcher`).  This is what submodules/dense_matcher/triangulate.py of the reference does once
its dense matcher has produced `kp_source` / `kp_target` for a view pair:

    triangulate_pair   DLT of every match, reprojection filter (< 2 px in both views), frame filter, bilinear colour
    background_sheet   DTU: the world points of depth 10 behind the (near-)white pixels of a view, colour 255
    grow_cloud         LLFF: 1000 rounds that draw 100 seeds x 200 Gaussian-perturbed candidates, keep those whose 11x11
                       patches in two views agree (SSIM >= 0.95) and whose rounded pixel holds at most two points of the cloud
    build_cloud        the whole script for a dataset folder and a matches file
    write_cloud_ply    x y z float, red green blue uchar, binary little endian

All three hot paths are HIP kernels (csrc/cloud.hip) behind `_C`; there is no CPU path.  The matcher network itself is not
part of this build: matches come from a file, or from the plane-sweep matcher of sweep_matcher.py (`matcher="sweep"`), which
is a classical stand-in and not the reference's network.

Matches file: a plain .npz with, for every ordered pair (ref, src) of selected views that has matches, two float32 [N, 2]
arrays of pixel coordinates (x, y) AT THE WORKING RESOLUTION (the image size divided by `resolution`):

    kp_<ref stem>_<src stem>_source    keypoints in the reference view  (the matcher's kp_source)
    kp_<ref stem>_<src stem>_target    the matching keypoints in the source view (kp_target)

where a stem is the image file name up to its first dot.  A pair that is missing (or empty) is skipped, as the reference
skips a pair without matches.
"""
from __future__ import annotations

import os
from math import exp
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dataset_readers as dr

LLFF_HOLD = dr.LLFF_HOLD
DTU_SPARSE_INDICES = tuple(dr.DTU_TRAIN)
WINDOW_SIZE = 11
SHEET_DEPTH = 10.0


class PinholeView(NamedTuple):
    intrinsic: np.ndarray      # [3,3] float32
    c2w: np.ndarray            # [4,4] float32


class DatasetViews(NamedTuple):
    names: List[str]           # image file names, in the order of the COLMAP image ids (the reference's order here)
    paths: List[str]
    intrinsics: np.ndarray     # [n,3,3] float32, divided by `resolution`
    c2ws: np.ndarray           # [n,4,4] float32
    width: int                 # working size
    height: int


# ---- host rules -----------------------------------------------------------------------------------------------------------
def ssim_window() -> torch.Tensor:
    """The 11x11 Gaussian window (sigma 1.5) of the patch SSIM, float32 [121], with the arithmetic of the usual
    create_window: a normalised 1-D float32 Gaussian and its outer product."""
    g = torch.Tensor([exp(-(x - WINDOW_SIZE // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(WINDOW_SIZE)])
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).reshape(-1).contiguous()


def select_views(n_images: int, dataset_name: str, n_views: int, dtu_sparse_indices: Sequence[int] = DTU_SPARSE_INDICES) -> List[int]:
    if dataset_name == "LLFF":
        train_idx = [idx for idx in range(n_images) if idx % LLFF_HOLD != 0]
        return [round(i) for i in np.linspace(0, len(train_idx) - 1, n_views)]
    if dataset_name == "DTU":
        return list(dtu_sparse_indices[:n_views])
    raise NotImplementedError(dataset_name)


def source_views(ref_indices: Sequence[int]) -> Dict[int, List[int]]:
    out = {}
    for idx in ref_indices:
        rest = list(ref_indices)
        rest.remove(idx)
        out[idx] = rest
    return out


def view_pairs(ref_indices: Sequence[int]) -> List[Tuple[int, int]]:
    srcs = source_views(ref_indices)
    return [(r, s) for r in ref_indices for s in srcs[r]]


def grid_margin(W: int, H: int) -> int:
    """Cells of margin the count grids need around the frame.  A count is read only where the bilinear lookup of an all-ones
    mask at (uv / (W-1, H-1)) * 2 - 1 is non-zero, i.e. where the unnormalised coordinate u * W / (W - 1) - 0.5 lies in
    (-1, W): u in (-0.5 + 1/(2W), W - 0.5 - 1/(2W)), whose rounding lies in [0, W - 1].  One cell covers fp32 slack."""
    for n in (W, H):
        if n < 2:
            raise ValueError("images of at least 2 x 2 pixels")
        lo, hi = (-1.0 + 0.5) * (n - 1) / n, (n + 0.5) * (n - 1) / n
        assert -0.5 < lo and hi < n - 0.5 and round(lo) >= 0 and round(hi) <= n - 1, (n, lo, hi)
    return 1


def stem(name: str) -> str:
    return os.path.basename(name).split(".")[0]


def match_keys(ref_name: str, src_name: str) -> Tuple[str, str]:
    base = f"kp_{stem(ref_name)}_{stem(src_name)}"
    return base + "_source", base + "_target"


def load_matches(path_or_map) -> Dict[str, np.ndarray]:
    """{key: float32 [N,2]} of a matches file (or of a mapping that already holds the arrays)"""
    if isinstance(path_or_map, (str, os.PathLike)):
        with np.load(path_or_map) as z:
            src = {k: z[k] for k in z.files}
    else:
        src = dict(path_or_map)
    out = {}
    for k, a in src.items():
        if not (k.startswith("kp_") and (k.endswith("_source") or k.endswith("_target"))):
            continue
        a = np.asarray(a, dtype=np.float32)
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"matches: {k} has shape {a.shape}, not [N, 2]")
        out[k] = np.ascontiguousarray(a)
    for k in out:
        if k.endswith("_source"):
            other = k[:-len("_source")] + "_target"
            if other not in out or out[other].shape != out[k].shape:
                raise ValueError(f"matches: {k} needs {other} of the same shape")
        elif k[:-len("_target")] + "_source" not in out:
            raise ValueError(f"matches: {k} without its _source array")
    return out


def pair_matches(matches: Dict[str, np.ndarray], ref_name: str, src_name: str) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    a, b = match_keys(ref_name, src_name)
    if a not in matches or len(matches[a]) == 0:
        return None
    return matches[a], matches[b]


def read_views(source_path: str, resolution: int = 1, images: str = "images") -> DatasetViews:
    """Cameras of <source>/sparse/0 in the order of their image ids, intrinsics divided by `resolution`; a SIMPLE_PINHOLE camera
    has its centre at (width / 2, height / 2), as the reference's script has it."""
    sparse = os.path.join(source_path, "sparse/0")
    try:
        extr = dr.read_images_bin(os.path.join(sparse, "images.bin"))
        intr = dr.read_cameras_bin(os.path.join(sparse, "cameras.bin"))
    except (OSError, KeyError):
        extr = dr.read_images_txt(os.path.join(sparse, "images.txt"))
        intr = dr.read_cameras_txt(os.path.join(sparse, "cameras.txt"))
    names, paths, ks, c2ws = [], [], [], []
    width = height = 0
    for key in sorted(extr.keys()):
        q, t, cam_id, name = extr[key]
        model, width, height, params = intr[cam_id]
        if model == "SIMPLE_PINHOLE":
            fx = fy = params[0]
            cx, cy = width / 2, height / 2
        elif model == "PINHOLE":
            fx, fy, cx, cy = params[:4]
        else:
            raise NotImplementedError(model)
        Rt = np.zeros((4, 4))
        Rt[:3, :3] = dr.quaternion_to_rotation(q)
        Rt[:3, 3] = np.array(t)
        Rt[3, 3] = 1.0
        c2ws.append(np.float32(np.linalg.inv(Rt)))
        k = np.zeros((3, 3))
        k[0, 0], k[1, 1], k[0, 2], k[1, 2], k[2, 2] = fx / resolution, fy / resolution, cx / resolution, cy / resolution, 1.0
        ks.append(k)
        names.append(name)
        paths.append(os.path.join(source_path, images, name))
    if resolution > 1:
        width, height = width // resolution, height // resolution
    return DatasetViews(names, paths, np.stack(ks).astype(np.float32), np.stack(c2ws).astype(np.float32), int(width), int(height))


def write_cloud_ply(path: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """x y z (float) red green blue (uchar), binary little endian: init_points.fetch_point_cloud and the reference's fetchPly
    (plyfile) both read it."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb).reshape(-1, 3)
    if len(xyz) != len(rgb):
        raise ValueError("one colour per point")
    rec = np.zeros(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = xyz[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        rec[name] = rgb[:, k].astype(np.uint8)
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}"]
    head += [f"property float {p}" for p in ("x", "y", "z")] + [f"property uchar {p}" for p in ("red", "green", "blue")] + ["end_header"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fp:
        fp.write(("\n".join(head) + "\n").encode("ascii"))
        fp.write(rec.tobytes())


# ---- device ---------------------------------------------------------------------------------------------------------------
def _f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


def _w2c(c2w) -> np.ndarray:
    return np.linalg.inv(_f32(c2w)).astype(np.float32)


def _dev_image(image, dev) -> torch.Tensor:
    """uint8 [H,W,3] on the device (a host tensor is NOT moved: there is no CPU path, _C refuses it)"""
    t = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image)).to(dev)
    if t.dim() == 3 and t.shape[2] > 3:
        t = t[..., :3]
    return t.contiguous()


def _up(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def triangulate_pair(ref_cam: PinholeView, src_cam: PinholeView, kp_ref, kp_src, ref_image, *, reproj_threshold: float = 2.0,
                     device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (points [K,3] float32, colors [K,3] uint8) on the device: the matches that survive both filters, in input order.
    The intrinsic matrix of `ref_cam` serves both views (the reference uses one matrix for every view)."""
    from . import _C
    img = ref_image if isinstance(ref_image, torch.Tensor) else _dev_image(ref_image, device)
    dev = img.device
    k34 = np.concatenate([_f32(ref_cam.intrinsic), np.zeros((3, 1), np.float32)], axis=1)
    w_ref, w_src = _w2c(ref_cam.c2w), _w2c(src_cam.c2w)
    as_kp = lambda k: k if isinstance(k, torch.Tensor) else _up(np.asarray(k, np.float32).reshape(-1, 2), dev)  # noqa: E731
    pts, col, count = _C.triangulate_matches(_up(k34 @ w_ref, dev), _up(k34 @ w_src, dev), _up(ref_cam.intrinsic, dev), _up(w_ref, dev),
                                             _up(w_src, dev), as_kp(kp_ref), as_kp(kp_src), _dev_image(img, dev),
                                             float(reproj_threshold))
    n = int(count.item())
    return pts[:n], col[:n]


def background_sheet(image, intrinsic, c2w, depth: float = SHEET_DEPTH, device="cuda") -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (points [K,3] float32, colors [K,3] uint8 = 255) of the pixels whose largest channel is >= 254, in pixel order"""
    from . import _C
    img = image if isinstance(image, torch.Tensor) else _dev_image(image, device)
    dev = img.device
    inv_kt = np.linalg.inv(_f32(intrinsic).T).astype(np.float32)
    back = np.linalg.inv(_w2c(c2w)).astype(np.float32)         # inverse(inverse(c2w)), as depth2point_world is called
    pts, col, count = _C.background_sheet(_dev_image(img, dev), _up(inv_kt, dev), _up(back, dev), float(depth))
    n = int(count.item())
    return pts[:n], col[:n]


class CloudOverflow(RuntimeError):
    def __init__(self, needed: int):
        super().__init__(f"the cloud needs {needed} rows")
        self.needed = needed


class CloudGrower:
    """The device state of a growth run: the cloud in buffers of a fixed capacity, its length and overflow words, one count
    grid per view.  round() launches and never reads the device; result() is the one read."""

    def __init__(self, points, colors, images, intrinsic, c2ws, *, capacity: Optional[int] = None, alpha: float = 10.0,
                 ssim_threshold: float = 0.95, h_patch_size: int = 5):
        from . import _C
        self._C = _C
        if not isinstance(points, torch.Tensor):
            raise TypeError("points is a device tensor")
        dev = points.device
        self.n_start = int(points.shape[0])
        if self.n_start < 1:
            raise ValueError("growth needs a non-empty starting cloud")
        imgs = images if isinstance(images, torch.Tensor) else torch.stack([_dev_image(i, dev) for i in images])
        self.images = imgs.contiguous()
        V, H, W = (int(s) for s in self.images.shape[:3])
        grid_margin(W, H)
        k = _f32(intrinsic)
        self.focal_center = (float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2]))
        self.w2c = _up(np.stack([_w2c(m) for m in _f32(c2ws)]), dev) if dev.type == "cuda" else torch.from_numpy(
            np.stack([_w2c(m) for m in _f32(c2ws)]))
        self.window = ssim_window().to(dev)
        self.capacity = max(int(capacity) if capacity is not None else self.n_start + 65536, self.n_start)
        self.points = torch.zeros((self.capacity, 3), dtype=torch.float32, device=dev)
        self.colors = torch.zeros((self.capacity, 3), dtype=torch.float32, device=dev)
        self.points[:self.n_start] = points.to(torch.float32)
        self.colors[:self.n_start] = colors.to(torch.float32)
        self.length = torch.full((1,), self.n_start, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.grids = torch.zeros((V, H + 2, W + 2), dtype=torch.int32, device=dev)
        self.alpha, self.ssim_threshold, self.h_patch_size = float(alpha), float(ssim_threshold), int(h_patch_size)
        self.rounds = 0

    def round(self, ref: int, src: int, seed_idx: torch.Tensor, noise: torch.Tensor, debug_ssim=None, debug_mask=None) -> None:
        """ref, src: slots of `images`; seed_idx int32 [seeds] and noise float32 [seeds, samples, 3] on the device"""
        fx, fy, cx, cy = self.focal_center
        self._C.cloud_grow_round(self.images, self.w2c, self.window, seed_idx, noise, self.points, self.colors, self.length,
                                 self.overflow, self.grids, int(ref), int(src), self.n_start, self.h_patch_size, self.rounds == 0,
                                 fx, fy, cx, cy, self.alpha, self.ssim_threshold, debug_ssim, debug_mask)
        self.rounds += 1

    def result(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (points [n,3], colors [n,3] float32 0..255); CloudOverflow when the buffers were too small"""
        n, flags = int(self.length.item()), int(self.overflow.item())
        if flags & 2:
            raise RuntimeError("a count was read outside the count grid: the margin rule of grid_margin() does not hold")
        if flags & 1 or n > self.capacity:
            raise CloudOverflow(n)
        return self.points[:n], self.colors[:n]


def default_draws(ref_indices: Sequence[int], n_start: int, iterations: int, seeds: int, samples: int, device) -> Iterable:
    """The reference's draws, in its order: host randperm for the reference view, host randperm for the source view, host
    randperm over the STARTING cloud for the seeds, device randn for the noise."""
    srcs = source_views(ref_indices)
    for _ in range(iterations):
        ref = ref_indices[int(torch.randperm(len(ref_indices))[0])]
        src = srcs[ref][int(torch.randperm(len(srcs[ref]))[0])]
        seed_idx = torch.randperm(n_start)[:seeds]
        noise = torch.randn(size=(seeds, samples, 3), device=device)
        yield ref, src, seed_idx, noise


def grow_cloud(points, colors, images, intrinsic, c2ws, ref_indices: Sequence[int], *, iterations: int = 1000, seeds: int = 100,
               samples: int = 200, alpha: float = 10.0, ssim_threshold: float = 0.95, h_patch_size: int = 5, draws=None,
               capacity: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (points, colors float32 0..255) after the growth rounds.  images / c2ws are indexed by view, ref_indices are the
    selected views; draws: an iterable of (ref, src, seed_indices, noise), or None for torch's generators.  The device is
    read once, at the end; a run whose buffers were too small is replayed with buffers of the size it reported."""
    ref_indices = [int(i) for i in ref_indices]
    dev = points.device
    n_start = int(points.shape[0])
    if draws is None and n_start < seeds:
        raise ValueError(f"{n_start} starting points cannot seed {seeds} candidates rows per round")
    slot = {v: k for k, v in enumerate(ref_indices)}
    sel_images = [images[i] for i in ref_indices]
    sel_c2ws = np.stack([_f32(c2ws[i]) for i in ref_indices])
    recorded = list(draws) if draws is not None else None
    if recorded is None:
        cpu_state = torch.get_rng_state()
        dev_state = torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None
    while True:
        g = CloudGrower(points, colors, sel_images, intrinsic, sel_c2ws, capacity=capacity, alpha=alpha, ssim_threshold=ssim_threshold,
                        h_patch_size=h_patch_size)
        run = recorded if recorded is not None else default_draws(ref_indices, n_start, iterations, seeds, samples, dev)
        for ref, src, seed_idx, noise in run:
            si = torch.as_tensor(seed_idx).to(device=dev, dtype=torch.int32, non_blocking=True)
            nz = torch.as_tensor(noise).to(device=dev, dtype=torch.float32, non_blocking=True)
            g.round(slot[int(ref)], slot[int(src)], si, nz)
        try:
            return g.result()
        except CloudOverflow as e:
            capacity = e.needed
            if recorded is None:
                torch.set_rng_state(cpu_state)
                if dev_state is not None:
                    torch.cuda.set_rng_state(dev_state, dev)


def plan_pairs(views: DatasetViews, ref_indices: Sequence[int]) -> List[Tuple[int, int, PinholeView, PinholeView]]:
    """The ordered view pairs in the reference's order, each with its two cameras.  Every camera carries the intrinsic matrix
    of camera 0, as the reference triangulates (and grows) with intrinsics_all[0] whatever the view."""
    k0 = views.intrinsics[0]
    return [(r, s, PinholeView(k0, views.c2ws[r]), PinholeView(k0, views.c2ws[s])) for r, s in view_pairs(ref_indices)]


def load_images(views: DatasetViews, resolution: int, device) -> List[torch.Tensor]:
    """uint8 [H,W,3] device tensors at the working size (resolution > 1: the project's device resize, ground_truth.py)"""
    out = []
    for p in views.paths:
        a = dr.read_image(p)
        if a.ndim == 2:
            a = np.repeat(a[..., None], 3, axis=2)
        a = np.ascontiguousarray(a[..., :3])
        if (a.shape[1], a.shape[0]) != (views.width, views.height):
            from .ground_truth import prepare_ground_truth
            img = prepare_ground_truth([a], (views.width, views.height), device=device)[0][0]
            out.append((img * 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous())
        else:
            out.append(torch.from_numpy(a).to(device))
    return out


def build_cloud(source_path: str, matches=None, *, dataset_name: str = "LLFF", n_views: int = 3, resolution: int = 4,
                dtu_sparse_indices: Sequence[int] = DTU_SPARSE_INDICES, device="cuda", matcher: str = "file", sweep=None,
                save_matches: Optional[str] = None, **grow) -> Tuple[np.ndarray, np.ndarray]:
    """-> (xyz float32 [P,3], rgb uint8 [P,3]) of a dataset folder and its matches.  matcher="file": `matches` is a file or a
    mapping (see the module's docstring).  matcher="sweep": the matches come from the plane-sweep matcher (sweep_matcher.py,
    `sweep`: its SweepParams) on the images loaded here, and are also written to `save_matches` when that is given.
    `grow`: keyword arguments of grow_cloud (LLFF only)."""
    if matcher not in ("file", "sweep"):
        raise ValueError(f'matcher is "file" or "sweep", not {matcher!r}')
    if matcher == "file":
        if matches is None:
            raise ValueError('matcher="file" needs the matches (a file or a mapping)')
        matches = load_matches(matches)
    elif matches is not None:
        raise ValueError('matcher="sweep" computes the matches itself: give no `matches`')
    views = read_views(source_path, resolution)
    ref_indices = select_views(len(views.names), dataset_name, n_views, dtu_sparse_indices)
    images = load_images(views, resolution, device)
    if matcher == "sweep":
        from . import sweep_matcher as sm
        params = sweep if sweep is not None else sm.SweepParams()
        near, far = sm.resolve_range(source_path, views, ref_indices, params)
        found = sm.match_images(views, images, ref_indices, near, far, params)
        if save_matches:
            sm.write_matches(save_matches, found)
        matches = load_matches(found)
    k0 = views.intrinsics[0]
    pts, cols = [], []
    plan = plan_pairs(views, ref_indices)
    for ref in ref_indices:
        for _, src, ref_cam, src_cam in (p for p in plan if p[0] == ref):
            m = pair_matches(matches, views.names[ref], views.names[src])
            if m is None:
                continue
            p, c = triangulate_pair(ref_cam, src_cam, m[0], m[1], images[ref], device=device)
            pts.append(p)
            cols.append(c)
        if dataset_name == "DTU":
            p, c = background_sheet(images[ref], views.intrinsics[ref], views.c2ws[ref], SHEET_DEPTH, device=device)
            pts.append(p)
            cols.append(c)
    if not pts:
        raise ValueError("no view pair has matches: nothing to triangulate")
    points, colors = torch.cat(pts), torch.cat(cols)
    if dataset_name == "LLFF" and len(points) > 0:
        points, fcol = grow_cloud(points, colors, images, k0, views.c2ws, ref_indices, **grow)
        colors = fcol.to(torch.uint8)                              # truncation, as astype(np.uint8)
    return points.cpu().numpy(), colors.cpu().numpy()
