"""A triangle mesh of a trained scene: TSDF fusion of rendered depth and marching tetrahedra, on the device.

    vol = TsdfVolume(bounds_min, bounds_max, voxel_size)       # tsdf, weight, rgb: 20 bytes per voxel
    vol.integrate(cameras, depths, alphas, colours)            # any number of views, 8 of one size per launch
    vertices, colours, faces = vol.extract(min_weight=1.0)     # float32 [V,3], uint8 [V,3], int32 [F,3], on the device
    write_mesh_ply(path, vertices, colours, faces)

    vertices, colours, faces = fuse_model(model, cameras, bg, resolution=256)

The arithmetic is stated in include/b3gs_raster.h (ABI 17) and restated in numpy by tests/mesh_ref.py: csrc/mesh.hip is one
pass over the volume per 8 views, and six launches per extraction.  The rendered depth is the alpha-weighted sum of the
camera-space z (csrc/render.hip), so depth / alpha is compared with the z of a voxel centre.  The host reads the device once
per extraction: the vertex and triangle totals, between count and emit.

Policy that is not hot lives here in torch: the bounds of a scene (scene_bounds), the split of views into calls.
"""
from __future__ import annotations

import math
import struct
from typing import Optional, Sequence

import numpy as np
import torch

MAX_VIEWS = 8          # views per integrate launch (B3GS_MAX_TSDF_VIEWS)
MAX_DIM = 1024         # voxels per axis (B3GS_MAX_TSDF_DIM)
DEPTHS = ("mean", "median")   # the depth of a pixel that fuse_model fuses
METHODS = ("tsdf", "poisson")  # how fuse_model turns the views into a surface
NEAR = 0.2             # the renderer's near plane (B3GS_NEAR): a voxel nearer to a camera than this is not seen by it


def camera_table(cameras: Sequence) -> np.ndarray:
    """float32 [n, 14]: world -> camera rotation (9, row-major), translation (3), focal lengths in pixels (2) of
    camera.Camera objects.  Reads each camera's matrices once (Camera._host_matrices caches them)."""
    rows = np.empty((len(cameras), 14), dtype=np.float32)
    for k, cam in enumerate(cameras):
        w2c = cam._host_matrices()["wvt"].T            # the stored matrix is the transpose (row-vector convention)
        fx, fy = cam.get_focal()
        rows[k, :9] = w2c[:3, :3].reshape(9)
        rows[k, 9:12] = w2c[:3, 3]
        rows[k, 12], rows[k, 13] = fx, fy
    return rows


class TsdfVolume:
    """nx x ny x nz voxels of `voxel_size` over [bounds_min, bounds_max] (the last voxel may reach past bounds_max); the
    centre of voxel (i, j, k) is bounds_min + (i + 0.5, j + 0.5, k + 0.5) * voxel_size.  tsdf is in units of the truncation."""

    def __init__(self, bounds_min, bounds_max, voxel_size: float, truncation: Optional[float] = None, device="cuda"):
        lo = [float(v) for v in bounds_min]
        hi = [float(v) for v in bounds_max]
        voxel_size = float(voxel_size)
        if len(lo) != 3 or len(hi) != 3 or not voxel_size > 0.0 or any(not h > l for l, h in zip(lo, hi)):
            raise ValueError("TsdfVolume: bounds_min < bounds_max per axis and a positive voxel size are needed")
        dims = [max(2, int(math.ceil((h - l) / voxel_size - 1e-4))) for l, h in zip(lo, hi)]
        if max(dims) > MAX_DIM:
            raise ValueError(f"TsdfVolume: {dims[0]} x {dims[1]} x {dims[2]} voxels; at most {MAX_DIM} per axis (use a larger voxel)")
        self._allocate(lo, voxel_size, dims, truncation, device)

    @classmethod
    def from_dims(cls, origin, dims, voxel_size: float, truncation: Optional[float] = None, device="cuda") -> "TsdfVolume":
        """A volume of exactly nx x ny x nz voxels (any size from 1; the bounds constructor rounds up to at least 2 per axis)."""
        dims = [int(d) for d in dims]
        voxel_size = float(voxel_size)
        if len(dims) != 3 or len(origin) != 3 or min(dims) < 1 or max(dims) > MAX_DIM or not voxel_size > 0.0:
            raise ValueError(f"TsdfVolume.from_dims: three sizes of 1 .. {MAX_DIM}, an origin and a positive voxel size are needed")
        self = cls.__new__(cls)
        self._allocate([float(v) for v in origin], voxel_size, dims, truncation, device)
        return self

    def _allocate(self, origin, voxel_size, dims, truncation, device):
        self.origin, self.voxel_size, self.dims = origin, voxel_size, tuple(dims)
        self.truncation = 4.0 * voxel_size if truncation is None else float(truncation)
        if not self.truncation > 0.0:
            raise ValueError("TsdfVolume: the truncation is positive")
        self.device = torch.device(device)
        nx, ny, nz = dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.rgb = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=self.device)
        self._workspace = None

    def reset(self):
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        self.rgb.zero_()

    def integrate(self, cameras, depths: Sequence[torch.Tensor], alphas: Sequence[torch.Tensor],
                  colours: Sequence[torch.Tensor], alpha_min: float = 0.5, near: float = NEAR):
        """Fuses views into the volume.  cameras: camera.Camera objects, or a float32 [n, 14] table (camera_table).  Per
        view: the renderer's depth ([H,W] or [1,H,W]), alpha (likewise) and colour [3,H,W], on the device.  Views are taken
        in order, 8 of one W x H per launch; the result is that of one pass over all of them."""
        from . import _C
        table = cameras if isinstance(cameras, np.ndarray) else camera_table(cameras)
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
        n = table.shape[0]
        if not (len(depths) == len(alphas) == len(colours) == n):
            raise ValueError("integrate: one depth, alpha and colour image per camera")
        start = 0
        while start < n:
            end = start + 1
            while end < n and end - start < MAX_VIEWS and colours[end].shape == colours[start].shape:
                end += 1
            _C.tsdf_integrate(self.tsdf, self.weight, self.rgb, self.origin, self.voxel_size, list(depths[start:end]),
                              list(alphas[start:end]), list(colours[start:end]), table[start:end], self.truncation, near, alpha_min)
            start = end

    def count(self, min_weight: float = 1.0) -> torch.Tensor:
        """The first half of extract(): -> int64 [2] on the device, {vertices, triangles}.  No host read (capturable)."""
        from . import _C
        self._workspace, totals = _C.mesh_count(self.tsdf, self.weight, self.rgb, self.origin, self.voxel_size, min_weight,
                                                self._workspace)
        return totals

    def extract(self, min_weight: float = 1.0):
        """-> (vertices float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) on the device.  A cell takes part when its 8
        corners have weight >= min_weight."""
        from . import _C
        nverts, ntris = self.count(min_weight).tolist()        # the one host read of the path
        return _C.mesh_emit(self.tsdf, self.weight, self.rgb, self.origin, self.voxel_size, self._workspace, nverts, ntris)


def scene_bounds(model, quantile: float = 0.01, pad: float = 0.0):
    """Per-axis [q, 1 - q] quantiles of the Gaussian centres, widened by `pad` (the truncation) -> (min [3], max [3]) lists."""
    xyz = model.get_xyz.detach().float()
    q = torch.tensor([quantile, 1.0 - quantile], dtype=torch.float32, device=xyz.device)
    # (torch.quantile refuses more than 16M elements: a strided subset keeps the quantiles of a larger cloud)
    step = max(1, xyz.shape[0] // (1 << 22))
    lohi = torch.quantile(xyz[::step], q, dim=0).cpu()
    return (lohi[0] - pad).tolist(), (lohi[1] + pad).tolist()


def fuse_model(model, cameras: Sequence, bg: torch.Tensor, *, resolution: Optional[int] = None, voxel_size: Optional[float] = None,
               bounds=None, truncation_voxels: float = 4.0, alpha_min: float = 0.5, min_weight: float = 1.0, quantile: float = 0.01,
               batch: int = MAX_VIEWS, return_volume: bool = False, depth: str = "mean", method: str = "tsdf", screen: Optional[float] = None,
               poisson_iters: Optional[int] = None, poisson_tol: Optional[float] = None, sample_stride: int = 1, spread: int = 1,
               trim: float = 0.0, info: Optional[dict] = None):
    """Renders `cameras` and fuses depth, alpha and colour into a volume, batch by batch out of the renderer's slot buffers
    (no clones, no host copies), then extracts the mesh.  At most one of resolution (voxels along the longest axis of the
    bounds; default 256) and voxel_size; bounds = (min [3], max [3]), default scene_bounds(), which is then widened by the
    truncation on every side (2 x truncation_voxels more voxels per axis).
    depth: which depth of a pixel is fused.  "mean" (the default): the renderer's alpha-weighted mean, rendered_depth /
    rendered_alpha -- between the surfaces where a semi-transparent Gaussian hangs in front of one.  "median": the depth at
    which the transmittance crosses one half (pixel_maps.py), always a depth at which a Gaussian sits.  The integration
    kernel divides its depth input by alpha, so it is handed median_depth * alpha: what it fuses is the median to one float32
    rounding (x * a / a is within one unit in the last place of x).
    method: "tsdf" (the default, described above) or "poisson": every sample_stride-th pixel of the same renders becomes an
    oriented sample (poisson.oriented_points; the median depth is handed over as it is), a screened Poisson fit over the same
    grid gives one smooth function (screen, poisson_iters, poisson_tol: poisson.PoissonVolume.solve's defaults when None) and
    its level set is extracted: closed wherever it stays inside the grid, also behind what the views saw.  `trim` then plays
    min_weight's part (0: every cell; W > 0: only cells whose corners have that much sample weight within `spread` nodes), the
    vertex colours are those of the nearest sample, the volume returned is the one the extractor read, and `info` (a dict)
    receives the solver's iteration count and residual."""
    from .evaluate import _batches
    if depth not in DEPTHS:
        raise ValueError(f"fuse_model: depth is one of {DEPTHS}")
    if method not in METHODS:
        raise ValueError(f"fuse_model: method is one of {METHODS}")
    if resolution is not None and voxel_size is not None:
        raise ValueError("fuse_model: resolution or voxel_size, not both")
    if bounds is None:
        lo, hi = scene_bounds(model, quantile)
    else:
        lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
    if voxel_size is None:
        res = 256 if resolution is None else int(resolution)
        if res < 2:
            raise ValueError("fuse_model: resolution >= 2")
        voxel_size = max(h - l for l, h in zip(lo, hi)) / res
    truncation = truncation_voxels * voxel_size
    if bounds is None:
        lo, hi = [v - truncation for v in lo], [v + truncation for v in hi]
    table = camera_table(cameras)
    if method == "poisson":
        return _fuse_poisson(model, cameras, table, bg, lo, hi, voxel_size, alpha_min, batch, return_volume, depth, screen, poisson_iters,
                             poisson_tol, sample_stride, spread, trim, info)
    vol = TsdfVolume(lo, hi, voxel_size, truncation, device=model.get_xyz.device)
    if depth == "median":
        from .pixel_maps import plane_batches
        for idx, outs, raws in plane_batches(model, cameras, bg, ("median_depth",), batch=batch):
            vol.integrate(table[idx], [r["median_depth"] * o["rendered_alpha"].reshape(r["median_depth"].shape) for o, r in zip(outs, raws)],
                          [o["rendered_alpha"] for o in outs], [o["render"] for o in outs], alpha_min=alpha_min)
    else:
        for idx, outs in _batches(model, cameras, bg, batch, full=True):
            vol.integrate(table[idx], [o["rendered_depth"] for o in outs], [o["rendered_alpha"] for o in outs],
                          [o["render"] for o in outs], alpha_min=alpha_min)
    mesh = vol.extract(min_weight)
    return mesh + (vol,) if return_volume else mesh


def _fuse_poisson(model, cameras, table, bg, lo, hi, voxel_size, alpha_min, batch, return_volume, depth, screen, iters, tol, stride, spread,
                  trim, info):
    from . import poisson
    from .evaluate import _batches
    parts = []
    if depth == "median":
        from .pixel_maps import plane_batches
        for idx, outs, raws in plane_batches(model, cameras, bg, ("median_depth",), batch=batch):
            parts.append(poisson.oriented_points(table[idx], [r["median_depth"] for r in raws], [o["rendered_alpha"] for o in outs],
                                                 [o["render"] for o in outs], stride=stride, alpha_min=alpha_min, median=True))
    else:
        for idx, outs in _batches(model, cameras, bg, batch, full=True):
            parts.append(poisson.oriented_points(table[idx], [o["rendered_depth"] for o in outs], [o["rendered_alpha"] for o in outs],
                                                 [o["render"] for o in outs], stride=stride, alpha_min=alpha_min))
    points, normals, weights, colours = (torch.cat([p[k] for p in parts]) for k in range(4))
    vol = poisson.PoissonVolume(lo, hi, voxel_size, device=model.get_xyz.device)
    vol.splat(points, normals, weights)
    res = vol.solve(poisson.SCREEN if screen is None else screen, iters, poisson.TOL if tol is None else tol)
    if info is not None:
        info.update(res)
    vertices, _, faces = vol.extract(trim, spread)
    vcol = poisson.sample_colours(vertices, points, colours, max(2.0 * (spread + 1), 4.0) * voxel_size)
    mesh = (vertices, vcol, faces)
    return mesh + (vol.volume,) if return_volume else mesh


# ---- PLY ---------------------------------------------------------------------------------------------------------------
_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_VERTEX_N = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                      ("red", "u1"), ("green", "u1"), ("blue", "u1")])                       # with vertex normals
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_PROPS = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
          "property uchar blue", "property list uchar int vertex_indices"]
_PROPS_N = _PROPS[:3] + ["property float nx", "property float ny", "property float nz"] + _PROPS[3:]


def _host(a, dtype):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_mesh_ply(path: str, vertices, colours, faces, normals=None) -> None:
    """Binary little-endian PLY: x y z (float32) red green blue (uint8) per vertex, `list uchar int vertex_indices` per face.
    With normals (float32 [V, 3]) the vertex also carries nx ny nz (float32) after x y z; without them the bytes are unchanged."""
    v, c, f = _host(vertices, np.float32).reshape(-1, 3), _host(colours, np.uint8).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    if len(v) != len(c):
        raise ValueError("write_mesh_ply: one colour per vertex")
    nrm = None if normals is None else _host(normals, np.float32).reshape(-1, 3)
    if nrm is not None and len(nrm) != len(v):
        raise ValueError("write_mesh_ply: one normal per vertex")
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(v)}\nproperty float x\nproperty float y\nproperty float z\n"
              + ("" if nrm is None else "property float nx\nproperty float ny\nproperty float nz\n") +
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {len(f)}\nproperty list uchar int vertex_indices\nend_header\n")
    vr = np.empty(len(v), dtype=_VERTEX if nrm is None else _VERTEX_N)
    vr["x"], vr["y"], vr["z"] = v[:, 0], v[:, 1], v[:, 2]
    if nrm is not None:
        vr["nx"], vr["ny"], vr["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    vr["red"], vr["green"], vr["blue"] = c[:, 0], c[:, 1], c[:, 2]
    fr = np.empty(len(f), dtype=_FACE)
    fr["n"] = 3
    fr["v"] = f
    with open(path, "wb") as fp:
        fp.write(struct.pack(f"<{len(header)}s", header.encode("ascii")))
        fp.write(vr.tobytes())
        fp.write(fr.tobytes())


def read_mesh_ply(path: str, return_normals: bool = False):
    """The files write_mesh_ply writes -> (vertices float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) numpy arrays, with or
    without vertex normals in the file; return_normals adds a fourth item, the normals float32 [V,3] or None when the file has
    none."""
    with open(path, "rb") as fp:
        data = fp.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    if props not in (_PROPS, _PROPS_N):
        raise ValueError(f"{path}: not the layout write_mesh_ply writes")
    vertex = _VERTEX_N if props == _PROPS_N else _VERTEX
    nv, nf = counts["vertex"], counts["face"]
    vr = np.frombuffer(data, dtype=vertex, count=nv, offset=end)
    fr = np.frombuffer(data, dtype=_FACE, count=nf, offset=end + nv * vertex.itemsize)
    if nf and not (fr["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    vertices = np.stack([vr["x"], vr["y"], vr["z"]], axis=1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    colours = np.stack([vr["red"], vr["green"], vr["blue"]], axis=1).astype(np.uint8) if nv else np.zeros((0, 3), np.uint8)
    faces = np.array(fr["v"], dtype=np.int32).reshape(-1, 3)
    if not return_normals:
        return vertices, colours, faces
    normals = None
    if vertex is _VERTEX_N:
        normals = np.stack([vr["nx"], vr["ny"], vr["nz"]], axis=1).astype(np.float32) if nv else np.zeros((0, 3), np.float32)
    return vertices, colours, faces, normals
