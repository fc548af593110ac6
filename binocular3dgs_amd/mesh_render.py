"""Rendering an extracted mesh on the device: a triangle rasterizer (csrc/meshraster.hip, entry points added to ABI 18,
INTEGRATION.md section 15).

    outs, rejected = render_mesh(vertices, colours, faces, cameras, bg, shading="colour")
    outs, rejected = render_mesh_shaded(vertices, normals, faces, cameras, bg, mode="lit")     # vertex normals: "smooth" or "lit"
    counts = face_pixels(vertices, faces, cameras)                       # int32 [F]: pixels each triangle wins, no host read
    vertices, colours, faces = cull_unseen(vertices, colours, faces, cameras, min_pixels=1)
    stats = depth_agreement(model, vertices, faces, cameras, bg)         # the mesh against the model's own rendered depth

Per view and pixel the nearest triangle: its index, the perspective-correct camera-space z (the quantity depth / alpha of the
splat renderer estimates), alpha 1 and a colour -- the interpolated vertex colours, or the face normal as a colour.  These
are the shapes frames.encode_frames takes, so a mesh goes through the same PNG and video tail as the model (spiral --mesh).
The arithmetic is stated in include/b3gs_raster.h and restated in numpy by tests/meshraster_ref.py; the outputs agree bit for
bit.  There is no clipping: a triangle with a vertex behind the near plane (0.2) or far outside the image is rejected and
counted, not drawn.

Policy that is not hot lives here in torch: the split of the cameras into calls, the face mask of cull_unseen, the sums of
depth_agreement.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

MAX_VIEWS = 8              # views per launch (B3GS_MAX_MESH_VIEWS)
MAX_IMAGE = 16384          # pixels per side (B3GS_MAX_MESH_IMAGE)
SMALL_BOX = 32             # a clamped box of at most this many pixels is walked by one lane (B3GS_MESH_SMALL_BOX)
WAVE_BOX = 4096            # ... of at most this many by one wave, beyond by one workgroup (B3GS_MESH_WAVE_BOX)
SHADINGS = {"colour": 0, "normal": 1}      # B3GS_MESH_SHADE_COLOUR / _NORMAL
SHADED = {"smooth": 2, "lit": 3}           # B3GS_MESH_SHADE_SMOOTH / _LIT: the modes of render_mesh_shaded (vertex normals)
INT32_MAX = 2 ** 31 - 1


def _check_mesh(vertices, colours, faces, what):
    if not isinstance(vertices, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise ValueError(f"{what}: vertices and faces are torch tensors")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices are float32 [V, 3]")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces are int32 [F, 3]")
    if vertices.shape[0] > INT32_MAX or faces.shape[0] > INT32_MAX:
        raise ValueError(f"{what}: more than 2^31 - 1 vertices or triangles")
    if faces.device != vertices.device:
        raise ValueError(f"{what}: faces are on {faces.device}, vertices on {vertices.device}")
    if colours is not None:
        if not isinstance(colours, torch.Tensor) or colours.dtype != torch.uint8 or tuple(colours.shape) != tuple(vertices.shape):
            raise ValueError(f"{what}: colours are uint8 [V, 3], one per vertex")
        if colours.device != vertices.device:
            raise ValueError(f"{what}: colours are on {colours.device}, vertices on {vertices.device}")


def _camera_runs(cameras, size, what):
    """-> (float32 [n, 14] table, [(start, end, W, H)]: runs of at most 8 consecutive cameras of one size)"""
    from .mesh import camera_table
    if isinstance(cameras, (np.ndarray, torch.Tensor)):
        if size is None:
            raise ValueError(f"{what}: a camera table needs size=(W, H)")
        table = np.ascontiguousarray(np.asarray(cameras, dtype=np.float32))
        if table.ndim != 2 or table.shape[1] != 14:
            raise ValueError(f"{what}: a camera table is float32 [n, 14]")
        sizes = [(int(size[0]), int(size[1]))] * len(table)
    else:
        cameras = list(cameras)
        table = camera_table(cameras)
        sizes = [(int(c.image_width), int(c.image_height)) for c in cameras] if size is None else [(int(size[0]), int(size[1]))] * len(cameras)
    for W, H in set(sizes):
        if not (1 <= W <= MAX_IMAGE and 1 <= H <= MAX_IMAGE):
            raise ValueError(f"{what}: an image has 1 .. {MAX_IMAGE} pixels per side, not {W} x {H}")
    runs, start, n = [], 0, len(sizes)
    while start < n:
        end = start + 1
        while end < n and end - start < MAX_VIEWS and sizes[end] == sizes[start]:
            end += 1
        runs.append((start, end) + sizes[start])
        start = end
    return table, runs


def raster_views(vertices, colours, faces, table, W, H, bg=None, *, shading="colour", cull_backface=False, face_pixels=None,
                 images=True, small_box=-1, wave_box=-1):
    """One launch pair: at most 8 views (rows of the host float32 [n, 14] `table`) of one W x H -> (triangle_id int32 [n,H,W],
    depth [n,1,H,W], alpha [n,1,H,W], colour [n,3,H,W], counts int32 [9] = rejected per view and, last, the faces that name
    no vertex).  images=False: only face_pixels is written.  small_box / wave_box move triangles between the three paths and
    never change an output (the tests use them).  No host read."""
    from . import _C
    if shading not in SHADINGS:
        raise ValueError(f"mesh_render: shading is one of {sorted(SHADINGS)}")
    table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
    if not 1 <= table.shape[0] <= MAX_VIEWS:
        raise ValueError(f"mesh_render: 1 .. {MAX_VIEWS} views per launch")
    ws, counts = _C.mesh_raster(vertices, faces, table, W, H, bool(cull_backface), int(small_box), int(wave_box))
    tid, depth, alpha, colour = _C.mesh_resolve(vertices, colours, faces, table, W, H, ws, bg, SHADINGS[shading], face_pixels, bool(images))
    return tid, depth, alpha, colour, counts


def render_mesh(vertices: torch.Tensor, colours: Optional[torch.Tensor], faces: torch.Tensor, cameras, bg: Optional[torch.Tensor] = None, *,
                shading: str = "colour", cull_backface: bool = False, face_pixels: Optional[torch.Tensor] = None, size=None):
    """Renders the mesh into every camera.  cameras: camera.Camera objects, or a float32 [n, 14] table (mesh.camera_table)
    with size=(W, H).  bg: float32 [3] on the device (None: black).  shading "colour": the vertex colours, interpolated
    perspective-correctly; "normal": the unit face normal in camera space, turned to the camera, as (n + 1) / 2 (colours may be
    None).  Views are taken in order, 8 of one size per launch.
    -> (per view {"render" [3,H,W], "rendered_depth" [1,H,W], "rendered_alpha" [1,H,W], "triangle_id" int32 [H,W]}: views of
        the batch tensors, the keys evaluation's renderer uses; rejected: int32 [n + 1] on the device: per view the triangles
        not drawn because a vertex lies behind the near plane, beyond the guard band of 2^14 pixels, or is not finite, or
        because an index is outside 0 .. V-1 -- and, last, the number of such faces.)
    face_pixels: an int32 [F] device tensor that takes + 1 per pixel a triangle wins.  No host read."""
    _check_mesh(vertices, colours, faces, "render_mesh")
    if shading not in SHADINGS:
        raise ValueError(f"render_mesh: shading is one of {sorted(SHADINGS)}")
    if shading == "colour" and colours is None:
        raise ValueError("render_mesh: colour shading needs the vertex colours")
    table, runs = _camera_runs(cameras, size, "render_mesh")
    outs: List[dict] = []
    rejected = torch.zeros(len(table) + 1, dtype=torch.int32, device=vertices.device)
    for start, end, W, H in runs:
        tid, depth, alpha, colour, counts = raster_views(vertices, colours, faces, table[start:end], W, H, bg, shading=shading,
                                                         cull_backface=cull_backface, face_pixels=face_pixels)
        rejected[start:end] = counts[:end - start]
        rejected[-1:] = counts[MAX_VIEWS:]
        for k in range(end - start):
            outs.append({"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]})
    return outs, rejected


def batches(vertices, colours, faces, cameras, bg=None, *, shading="colour", cull_backface=False, size=None):
    """Yields (camera indices, per-view output dicts) per launch, 8 views of one size at a time: the per-batch source
    frames.render_path takes in place of the model's renderer."""
    _check_mesh(vertices, colours, faces, "mesh_render.batches")
    table, runs = _camera_runs(cameras, size, "mesh_render.batches")
    for start, end, W, H in runs:
        tid, depth, alpha, colour, _ = raster_views(vertices, colours, faces, table[start:end], W, H, bg, shading=shading,
                                                    cull_backface=cull_backface)
        yield list(range(start, end)), [{"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]}
                                        for k in range(end - start)]


# ---- shading from vertex normals (csrc/meshsmooth.hip) -------------------------------------------------
def _check_normals(vertices, normals, mode, what):
    if mode not in SHADED:
        raise ValueError(f"{what}: mode is one of {sorted(SHADED)}")
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float32 or tuple(normals.shape) != tuple(vertices.shape):
        raise ValueError(f"{what}: normals are float32 [V, 3], one per vertex")
    if normals.device != vertices.device:
        raise ValueError(f"{what}: normals are on {normals.device}, vertices on {vertices.device}")


def raster_views_shaded(vertices, normals, faces, table, W, H, bg=None, *, mode="smooth", cull_backface=False, face_pixels=None,
                        small_box=-1, wave_box=-1):
    """raster_views with the colour taken from the vertex normals (mesh_tools.vertex_normals), interpolated perspective-correctly:
    "smooth" shows the unit normal in camera space, turned to the camera, as (n + 1) / 2; "lit" a grey headlight,
    0.15 + 0.85 max(-n_z, 0).  The other outputs are those of raster_views, bit for bit.  No host read."""
    from . import _C
    if mode not in SHADED:
        raise ValueError(f"mesh_render: mode is one of {sorted(SHADED)}")
    table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
    if not 1 <= table.shape[0] <= MAX_VIEWS:
        raise ValueError(f"mesh_render: 1 .. {MAX_VIEWS} views per launch")
    ws, counts = _C.mesh_raster(vertices, faces, table, W, H, bool(cull_backface), int(small_box), int(wave_box))
    tid, depth, alpha, colour = _C.mesh_resolve_shaded(normals, faces, table, W, H, ws, bg, SHADED[mode], face_pixels)
    return tid, depth, alpha, colour, counts


def render_mesh_shaded(vertices: torch.Tensor, normals: torch.Tensor, faces: torch.Tensor, cameras, bg: Optional[torch.Tensor] = None, *,
                       mode: str = "smooth", cull_backface: bool = False, size=None):
    """render_mesh with the shading of raster_views_shaded -> (per view output dicts, rejected), the shapes of render_mesh."""
    _check_mesh(vertices, None, faces, "render_mesh_shaded")
    _check_normals(vertices, normals, mode, "render_mesh_shaded")
    table, runs = _camera_runs(cameras, size, "render_mesh_shaded")
    outs: List[dict] = []
    rejected = torch.zeros(len(table) + 1, dtype=torch.int32, device=vertices.device)
    for start, end, W, H in runs:
        tid, depth, alpha, colour, counts = raster_views_shaded(vertices, normals, faces, table[start:end], W, H, bg, mode=mode,
                                                                cull_backface=cull_backface)
        rejected[start:end] = counts[:end - start]
        rejected[-1:] = counts[MAX_VIEWS:]
        for k in range(end - start):
            outs.append({"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]})
    return outs, rejected


def batches_shaded(vertices, normals, faces, cameras, bg=None, *, mode="smooth", cull_backface=False, size=None):
    """batches with the shading of raster_views_shaded: the per-batch source frames.render_path takes."""
    _check_mesh(vertices, None, faces, "mesh_render.batches_shaded")
    _check_normals(vertices, normals, mode, "mesh_render.batches_shaded")
    table, runs = _camera_runs(cameras, size, "mesh_render.batches_shaded")
    for start, end, W, H in runs:
        tid, depth, alpha, colour, _ = raster_views_shaded(vertices, normals, faces, table[start:end], W, H, bg, mode=mode,
                                                           cull_backface=cull_backface)
        yield list(range(start, end)), [{"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]}
                                        for k in range(end - start)]


def _face_pixels(vertices, faces, cameras, size, what):
    _check_mesh(vertices, None, faces, what)
    table, runs = _camera_runs(cameras, size, what)
    counts = torch.zeros(faces.shape[0], dtype=torch.int32, device=vertices.device)
    bad = torch.zeros(1, dtype=torch.int32, device=vertices.device)
    for start, end, W, H in runs:
        c = raster_views(vertices, None, faces, table[start:end], W, H, face_pixels=counts, images=False)[4]
        bad = c[MAX_VIEWS:]
    return counts, bad


def face_pixels(vertices: torch.Tensor, faces: torch.Tensor, cameras, size=None) -> torch.Tensor:
    """int32 [F] on the device: the pixels each triangle wins, summed over the cameras.  No host read; a face that names no
    vertex wins none (cull_unseen and depth_agreement raise for it)."""
    return _face_pixels(vertices, faces, cameras, size, "face_pixels")[0]


def cull_unseen(vertices: torch.Tensor, colours: torch.Tensor, faces: torch.Tensor, cameras, min_pixels: int = 1, size=None):
    """Drops the triangles that win fewer than `min_pixels` pixels over all the cameras -- the geometry no camera sees, e.g.
    blobs inside or behind the observed surface -- and the vertices no kept triangle names (mesh_tools.clean)
    -> (vertices, colours, faces), order and winding preserved."""
    from . import mesh_tools
    if min_pixels < 1:
        raise ValueError("cull_unseen: min_pixels is at least 1")
    _check_mesh(vertices, colours, faces, "cull_unseen")
    counts, bad = _face_pixels(vertices, faces, cameras, size, "cull_unseen")
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"cull_unseen: {nbad} triangles name a vertex outside 0 .. {vertices.shape[0] - 1}")
    return mesh_tools.clean(vertices, colours, faces[counts >= int(min_pixels)].contiguous(), 0, 0)


def depth_agreement(model, vertices: torch.Tensor, faces: torch.Tensor, cameras: Sequence, bg: torch.Tensor, alpha_min: float = 0.5,
                    depth: str = "mean") -> dict:
    """How far the mesh is from the model's own rendered depth in `cameras`: the model is rendered through evaluation's batched
    renderer, the mesh into the same cameras.  With d = |z_mesh - depth / alpha| (fp64) over the pixels where the model's
    alpha >= alpha_min and the mesh covers: mean and median of d (the median is the element of rank (n - 1) // 2),
    model_missed = the share of the model's pixels (alpha >= alpha_min) the mesh does not cover, mesh_uncovered = the share of
    the mesh's pixels where the model's alpha is below alpha_min.  Sums on the device, one host read at the end.
    depth="median" compares with the model's median depth (pixel_maps.py; the choice of mesh.fuse_model) in place of
    depth / alpha: d = |z_mesh - median_depth|."""
    from .evaluate import _batches
    from .mesh import DEPTHS, camera_table
    if depth not in DEPTHS:
        raise ValueError(f"depth_agreement: depth is one of {DEPTHS}")
    _check_mesh(vertices, None, faces, "depth_agreement")
    cameras = list(cameras)
    table = camera_table(cameras)
    dev = vertices.device
    sums = torch.zeros(4, dtype=torch.float64, device=dev)          # sum d, both, model, mesh
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    diffs = []
    if depth == "median":
        from .pixel_maps import plane_batches
        source = plane_batches(model, cameras, bg, ("median_depth",), batch=MAX_VIEWS)
    else:
        source = ((idx, outs, None) for idx, outs in _batches(model, cameras, bg, MAX_VIEWS, full=True))
    for idx, outs, raws in source:
        W, H = int(cameras[idx[0]].image_width), int(cameras[idx[0]].image_height)
        _, z, cover, _, counts = raster_views(vertices, None, faces, table[idx], W, H, shading="normal")
        bad = counts[MAX_VIEWS:]
        alpha = torch.stack([o["rendered_alpha"].reshape(1, H, W) for o in outs])
        if raws is None:
            zmodel = torch.stack([o["rendered_depth"].reshape(1, H, W) for o in outs]).double() / alpha.double()
        else:
            zmodel = torch.stack([r["median_depth"].reshape(1, H, W) for r in raws]).double()
        m_model, m_mesh = alpha >= alpha_min, cover > 0
        both = m_model & m_mesh
        d = torch.where(both, (z.double() - zmodel).abs(), torch.full_like(zmodel, float("inf")))
        sums += torch.stack([torch.where(both, d, torch.zeros_like(d)).sum(), both.sum().double(), m_model.sum().double(), m_mesh.sum().double()])
        diffs.append(d.reshape(-1))
    if not diffs:
        raise ValueError("depth_agreement: no cameras")
    ordered = torch.sort(torch.cat(diffs)).values
    rank = ((sums[1] - 1.0).clamp(min=0.0) / 2.0).floor().long().reshape(1)
    total, both, nmodel, nmesh, median, nbad = torch.cat([sums, ordered[rank], bad.double()]).tolist()     # the one host read
    if nbad:
        raise ValueError(f"depth_agreement: {int(nbad)} triangles name a vertex outside 0 .. {vertices.shape[0] - 1}")
    out = {"mean": total / both if both else float("nan"), "median": median if both else float("nan"),
           "model_missed": (nmodel - both) / nmodel if nmodel else float("nan"),
           "mesh_uncovered": (nmesh - both) / nmesh if nmesh else float("nan"),
           "pixels": int(both), "model_pixels": int(nmodel), "mesh_pixels": int(nmesh), "views": len(cameras), "alpha_min": float(alpha_min)}
    if depth != "mean":          # (the default's dict stays as it was)
        out["model_depth"] = depth
    return out
