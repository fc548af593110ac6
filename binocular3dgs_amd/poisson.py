"""A watertight mesh of a trained scene: screened Poisson reconstruction of oriented samples, on the device.

    points, normals, weights, colours = oriented_points(cameras, depths, alphas, colours, stride=2)
    vol = PoissonVolume(bounds_min, bounds_max, voxel_size)
    vol.splat(points, normals, weights)                          # density and normal field on the node grid
    info = vol.solve(screen=4.0)                                 # conjugate gradients: two launches per iteration, no host read
    tsdf = vol.to_tsdf(spread=1)                                 # a mesh.TsdfVolume: level x - iso, weight = support of the samples
    vertices, colours, faces = vol.extract(min_weight=0.0)       # marching tetrahedra, unchanged; 0 keeps every cell: closed

    vertices, colours, faces = reconstruct(points, normals, weights, colours, resolution=128)      # any oriented cloud
    vertices, colours, faces = mesh.fuse_model(model, cameras, bg, method="poisson")

The arithmetic is stated in include/b3gs_raster.h and restated in numpy by tests/poisson_ref.py; csrc/poisson.hip agrees with it
bit for bit.  TSDF fusion (mesh.py) only has a surface where a view looked; the Poisson fit is one smooth function over the
whole grid, so its level set is closed wherever it stays inside the grid.  The host reads the device once per stage: the sample
count between the two halves of oriented_points, the solver's status words after solve, the two totals of the extraction.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np
import torch

from .mesh import MAX_VIEWS, TsdfVolume, camera_table

SCREEN = 4.0           # the weight of the samples against the smoothness term (PoissonRecon's point weight)
TOL = 1e-4             # relative residual |r| / |b| at which the solver stops
REL_JUMP = 0.05        # a neighbour whose depth differs by more than this share of the pixel's is across a depth edge
MIN_COS = 0.1          # a sample seen at a flatter angle than acos(MIN_COS) is dropped
SPREAD = 1             # nodes around a node over which the support (the volume's weight) is summed


def default_iters(dims) -> int:
    """4 * the longest axis: on the analytic shapes the residual falls below TOL between 2 and 4 times the axis"""
    return 4 * int(max(dims))


def oriented_points(cameras, depths: Sequence[torch.Tensor], alphas: Sequence[torch.Tensor], colours: Sequence[torch.Tensor], *,
                    stride: int = 1, alpha_min: float = 0.5, rel_jump: float = REL_JUMP, min_cos: float = MIN_COS, median: bool = False):
    """Back-projects every stride-th pixel whose four axis neighbours are opaque and at a similar depth, with the normal of its
    neighbours' cross and the cosine to the viewing ray as weight.  cameras: camera.Camera objects or a float32 [n, 14] table
    (mesh.camera_table).  Per view the renderer's depth and alpha ([H,W] or [1,H,W]) and colour [3,H,W]; median: `depths` holds a
    depth as it is (pixel_maps' median depth), not the renderer's depth * alpha.  Views go 8 of one size per launch.
    -> points [n,3], normals [n,3], weights [n], colours [n,3], float32 on the device, in (view, row, column) order."""
    from . import _C
    table = cameras if isinstance(cameras, np.ndarray) else camera_table(cameras)
    table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
    n = table.shape[0]
    if not (len(depths) == len(alphas) == len(colours) == n):
        raise ValueError("oriented_points: one depth, alpha and colour image per camera")
    outs, start = [], 0
    while start < n:
        end = start + 1
        while end < n and end - start < MAX_VIEWS and colours[end].shape == colours[start].shape:
            end += 1
        args = (list(depths[start:end]), list(alphas[start:end]), list(colours[start:end]), table[start:end], int(stride), float(alpha_min),
                float(rel_jump), float(min_cos), bool(median))
        ws, count = _C.oriented_points_count(*args)
        outs.append(_C.oriented_points_emit(*args, ws, int(count.item())))              # the one host read of the batch
        start = end
    if len(outs) == 1:
        return outs[0]
    if not outs:
        raise ValueError("oriented_points: no views")
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


class PoissonVolume:
    """The node grid of a mesh.TsdfVolume over [bounds_min, bounds_max] (nodes at the voxel centres) with the density and normal
    field of the samples, the solution and the workspace of the solver."""

    def __init__(self, bounds_min, bounds_max, voxel_size: float, device="cuda"):
        self._init(TsdfVolume(bounds_min, bounds_max, voxel_size, device=device))

    @classmethod
    def from_dims(cls, origin, dims, voxel_size: float, device="cuda") -> "PoissonVolume":
        """A grid of exactly nx x ny x nz nodes (any size from 1; the bounds constructor rounds up to at least 2)."""
        tv = TsdfVolume.from_dims(origin, dims, voxel_size, device=device)
        self = cls.__new__(cls)
        self._init(tv)
        return self

    def _init(self, tv: TsdfVolume):
        self.volume = tv
        self.origin, self.voxel_size, self.dims, self.device = tv.origin, tv.voxel_size, tv.dims, tv.device
        self.density = self.vector = self.x = self.rhs = self._ws = self._state = None
        self.nsamples = 0

    def splat(self, points: torch.Tensor, normals: torch.Tensor, weights: torch.Tensor):
        """Trilinear splat of the samples: density [nz,ny,nx] = sum(w t) and vector [3,nz,ny,nx] = sum(w t n) per node.  Samples
        whose 8 surrounding nodes are not all inside the grid are dropped (solve reports how many)."""
        from . import _C
        self.nsamples = int(points.shape[0])
        need = _C.poisson_workspace_bytes(*self.dims, self.nsamples)
        ws = self._ws if self._ws is not None and self._ws.numel() >= need else None
        self.density, self.vector, self._ws = _C.poisson_splat(points, normals, weights, list(self.dims), list(self.origin), self.voxel_size, ws)
        self.x = self.rhs = self._state = None

    def solve(self, screen: float = SCREEN, iters: Optional[int] = None, tol: float = TOL, *, max_blocks: int = 0) -> dict:
        """Conjugate gradients on (Laplacian + screen * density) x = -div vector from x = 0: `iters` iterations (default
        default_iters) unless |r| <= tol |b| earlier.  -> {"iterations", "residual" (|r| / |b|), "dropped", "samples"}; a grid
        no sample reached is an error.  max_blocks bounds the workgroups of a launch (the result does not depend on it)."""
        from . import _C
        from ._lib import B3gsError
        if self.density is None:
            raise ValueError("PoissonVolume.solve: splat first")
        iters = default_iters(self.dims) if iters is None else int(iters)
        self.x, self.rhs, self._state = _C.poisson_solve(self.density, self.vector, float(screen), iters, float(tol), self._ws, int(max_blocks))
        state = self._state.cpu()                                                          # the one host read of the stage
        dropped, samples, status, iterations = state[:4].tolist()
        rr, bb = state[5:7].view(torch.float64).tolist()
        if status & 1:
            raise B3gsError(f"PoissonVolume.solve: none of the {samples} samples has its 8 nodes inside the {self.dims[0]} x {self.dims[1]} x "
                            f"{self.dims[2]} grid ({dropped} dropped)")
        return {"iterations": iterations, "residual": math.sqrt(rr / bb) if bb > 0.0 else 0.0, "dropped": dropped, "samples": samples}

    def iterations(self) -> torch.Tensor:
        """The solver's iteration word, int64 [1] on the device (no host read)."""
        return self._state[3:4]

    def to_tsdf(self, spread: int = SPREAD) -> TsdfVolume:
        """Fills the mesh.TsdfVolume: tsdf = x - iso with iso the density-weighted mean of x (positive in free space), weight =
        the density summed over the (2 spread + 1)^3 nodes around, rgb = 0."""
        from . import _C
        if self.x is None:
            raise ValueError("PoissonVolume.to_tsdf: solve first")
        tv = self.volume
        _C.poisson_volume(tv.tsdf, tv.weight, tv.rgb, self.density, self.x, int(spread), self._ws)
        return tv

    def extract(self, min_weight: float = 0.0, spread: int = SPREAD):
        """-> (vertices float32 [V,3], colours uint8 [V,3] (zero), faces int32 [F,3]).  min_weight = 0 keeps every cell: the mesh is
        closed wherever the surface stays inside the grid; a positive value trims what fewer samples than that support."""
        return self.to_tsdf(spread).extract(min_weight)


def sample_colours(vertices: torch.Tensor, points: torch.Tensor, colours: torch.Tensor, max_dist: float) -> torch.Tensor:
    """uint8 [V,3]: the colour (float32 in [0, 1]) of every vertex's nearest sample within max_dist (black beyond it)"""
    from .mesh_tools import NearestGrid
    if vertices.shape[0] == 0 or points.shape[0] == 0:
        return torch.zeros((vertices.shape[0], 3), dtype=torch.uint8, device=vertices.device)
    _, index = NearestGrid(points.contiguous(), float(max_dist)).query_index(vertices.contiguous())
    found = (index >= 0).unsqueeze(1)
    col = colours.float()[index.clamp(min=0).long()]
    return torch.where(found, (col.clamp(0.0, 1.0) * 255.0).round(), torch.zeros_like(col)).to(torch.uint8)


def reconstruct(points: torch.Tensor, normals: torch.Tensor, weights: Optional[torch.Tensor] = None, colours: Optional[torch.Tensor] = None, *,
                resolution: Optional[int] = None, voxel_size: Optional[float] = None, bounds=None, pad_voxels: int = 4,
                screen: float = SCREEN, iters: Optional[int] = None, tol: float = TOL, spread: int = SPREAD, min_weight: float = 0.0,
                return_volume: bool = False):
    """A mesh of any oriented cloud (a mesh's vertices with mesh_tools.vertex_normals included).  points, normals float32 [n,3];
    weights [n] (default 1); colours float32 [n,3] in [0,1] (default: black vertices).  The grid: `bounds` or the cloud's box,
    widened by pad_voxels voxels on every side, at `voxel_size` or `resolution` (default 128) voxels along the longest axis.
    -> (vertices, colours uint8, faces) and, with return_volume, the PoissonVolume and solve()'s dict."""
    if resolution is not None and voxel_size is not None:
        raise ValueError("reconstruct: resolution or voxel_size, not both")
    if points.shape[0] < 1:
        raise ValueError("reconstruct: no samples")
    if bounds is None:
        lo, hi = points.min(dim=0).values.tolist(), points.max(dim=0).values.tolist()
    else:
        lo, hi = [float(v) for v in bounds[0]], [float(v) for v in bounds[1]]
    if voxel_size is None:
        res = 128 if resolution is None else int(resolution)
        if res < 2:
            raise ValueError("reconstruct: resolution >= 2")
        voxel_size = max(max(h - l for l, h in zip(lo, hi)) / res, 1e-12)
    pad = pad_voxels * voxel_size
    vol = PoissonVolume([v - pad for v in lo], [v + pad for v in hi], voxel_size, device=points.device)
    if weights is None:
        weights = torch.ones(points.shape[0], dtype=torch.float32, device=points.device)
    vol.splat(points.float(), normals.float(), weights.float())
    info = vol.solve(screen, iters, tol)
    vertices, vcol, faces = vol.extract(min_weight, spread)
    if colours is not None:
        vcol = sample_colours(vertices, points.float(), colours, max(2.0 * (spread + 1), 4.0) * voxel_size)
    out = (vertices, vcol, faces)
    return out + (vol, info) if return_volume else out
