"""Texturing an extracted mesh on the device: atlas bake, textured render, OBJ files (csrc/texture.hip, entry points added to
ABI 18).

    cell, width = atlas_for(F, max_side=4096)
    texture, coverage = bake_texture(vertices, colours, faces, cameras, images, cell=cell, width=width, slack=voxel)
    outs, rejected = render_textured(vertices, faces, texture, cell, cameras, bg)
    write_textured_obj("mesh.obj", vertices, faces, texture, cell)       # mesh.obj, mesh.mtl, mesh.png

There are no charts and no unwrapping: every triangle owns a right-angled patch of one atlas, two triangles to a cell of
(cell + 1) x cell texels.  A texel is a point of its triangle's plane; it takes the pictures of the cameras that see the point
(the mesh rasterizer's resolved triangle and depth at the nearest pixel, `slack` deep), weighted by the squared cosine between
the face normal and the direction to the camera, and where no camera sees it, the interpolated vertex colours.  The legs of a
patch are cell - 2 texels, so a bilinear fetch inside a triangle reads that triangle's own texels only.  The arithmetic is
stated in include/b3gs_raster.h and restated in numpy by tests/texture_ref.py; the outputs agree bit for bit.

Policy that is not hot lives here: the split of the cameras into calls, the atlas arithmetic, the files.
"""
from __future__ import annotations

import math
import os
import re
from typing import List, Optional, Sequence

import numpy as np
import torch

from .mesh_render import MAX_VIEWS, _camera_runs, _check_mesh

MIN_CELL = 4               # B3GS_TEXTURE_MIN_CELL
MAX_CELL = 256             # B3GS_TEXTURE_MAX_CELL
MAX_SIDE = 16384           # texels per side of the atlas (B3GS_MAX_ATLAS_SIDE)


# ---- the atlas: integer arithmetic, the same in csrc/texture_layout.h -----------------------------------------------------
def _height(F: int, n: int, Wt: int) -> int:
    """the atlas height, 0 when there is no such atlas"""
    if F < 1 or F > 2 ** 31 - 1 or not MIN_CELL <= n <= MAX_CELL or not n + 1 <= Wt <= MAX_SIDE:
        return 0
    cpr = Wt // (n + 1)
    Ht = n * -(-((F + 1) // 2) // cpr)
    return Ht if Ht <= MAX_SIDE else 0


def largest_cell(F: int, Wt: int) -> int:
    """the largest cell whose atlas of width Wt holds F triangles (0: none)"""
    return next((n for n in range(MAX_CELL, MIN_CELL - 1, -1) if _height(F, n, Wt)), 0)


def atlas_size(F: int, n: int, Wt: int):
    """(Wt, Ht) of the atlas of F triangles with cell parameter n and width Wt: Wt // (n + 1) cells of (n + 1) x n texels per
    row, two triangles per cell.  Raises ValueError, naming the largest n that fits, when 4 <= n <= 256, one cell per row and
    Wt, Ht <= 16384 do not all hold."""
    F, n, Wt = int(F), int(n), int(Wt)
    Ht = _height(F, n, Wt)
    if not Ht:
        raise ValueError(f"no atlas of cell {n} and width {Wt} for {F} triangles (4 <= cell <= 256, cell + 1 <= width, width and "
                         f"height <= {MAX_SIDE}); the largest cell that fits this width is {largest_cell(F, Wt)}")
    return Wt, Ht


def atlas_for(F: int, max_side: int = 4096):
    """(n, Wt): the largest cell parameter whose atlas of F triangles fits a square of max_side texels, and its width, trimmed
    to whole cells."""
    F, max_side = int(F), int(max_side)
    if F < 1 or not 1 <= max_side <= MAX_SIDE:
        raise ValueError(f"atlas_for: F >= 1 and 1 <= max_side <= {MAX_SIDE}")
    for n in range(MAX_CELL, MIN_CELL - 1, -1):
        Wt = max_side // (n + 1) * (n + 1)
        if 0 < _height(F, n, Wt) <= max_side:
            return n, Wt
    raise ValueError(f"atlas_for: {F} triangles do not fit a square of {max_side} texels at the smallest cell, {MIN_CELL}")


def face_corners(F: int, n: int, Wt: int) -> np.ndarray:
    """float32 [F, 3, 2]: the corners of every triangle in texel-centre coordinates (x, y), whole numbers"""
    atlas_size(F, n, Wt)
    cpr = Wt // (n + 1)
    f = np.arange(F, dtype=np.int64)
    c = f // 2
    x0, y0 = (c % cpr) * (n + 1), (c // cpr) * n
    even = np.stack([np.stack([x0, y0], 1), np.stack([x0 + n - 2, y0], 1), np.stack([x0, y0 + n - 2], 1)], 1)
    odd = np.stack([np.stack([x0 + n, y0 + n - 1], 1), np.stack([x0 + 2, y0 + n - 1], 1), np.stack([x0 + n, y0 + 1], 1)], 1)
    return np.where((f % 2 == 1)[:, None, None], odd, even).astype(np.float32)


def face_uvs(F: int, n: int, Wt: int, Ht: int) -> np.ndarray:
    """float32 [F, 3, 2]: OBJ texture coordinates, u = (x + 0.5) / Wt, v = 1 - (y + 0.5) / Ht (computed in float64)"""
    if atlas_size(F, n, Wt)[1] != int(Ht):
        raise ValueError(f"face_uvs: the atlas of {F} triangles, cell {n} and width {Wt} has {atlas_size(F, n, Wt)[1]} rows, not {Ht}")
    xy = face_corners(F, n, Wt).astype(np.float64)
    return np.stack([(xy[..., 0] + 0.5) / Wt, 1.0 - (xy[..., 1] + 0.5) / Ht], axis=-1).astype(np.float32)


# ---- bake ----------------------------------------------------------------------------------------------------------------
def _check_images(images, runs, device, what):
    images = list(images)
    ncams = runs[-1][1] if runs else 0
    if len(images) != ncams:
        raise ValueError(f"{what}: {len(images)} images for {ncams} cameras")
    for start, end, W, H in runs:
        for k in range(start, end):
            im = images[k]
            if not isinstance(im, torch.Tensor) or im.dtype != torch.float32 or im.dim() != 3 or im.shape[0] != 3:
                raise ValueError(f"{what}: image {k} is not a float32 [3, H, W] tensor")
            if tuple(im.shape[1:]) != (H, W):
                raise ValueError(f"{what}: image {k} is {im.shape[2]} x {im.shape[1]}, its camera {W} x {H}")
            if im.device != device:
                raise ValueError(f"{what}: image {k} is on {im.device}, vertices on {device}")
    return images


def _check_slack(slack, what):
    slack = float(slack)
    if not (slack >= 0.0 and math.isfinite(slack)):
        raise ValueError(f"{what}: slack is at least 0 and finite")
    return slack


def accumulate_views(vertices, faces, table, W, H, images, accum, *, cell, slack, two_sided=False):
    """One rasterizer launch pair and one accumulate call: at most 8 views (rows of the host float32 [n, 14] `table`) of one
    W x H, `images` float32 [n, 3, H, W], added into accum float32 [Ht, Wt, 4] in place -> int32 [1] on the device: the
    triangles that name a vertex outside 0 .. V-1.  No host read."""
    from . import _C
    from .mesh_render import raster_views
    tid, depth, _, _, _ = raster_views(vertices, None, faces, table, W, H, shading="normal")
    table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
    return _C.mesh_texture_accumulate(vertices, faces, table, W, H, int(cell), accum.shape[1], tid, depth, images, float(slack), bool(two_sided), accum)


def bake_texture(vertices: torch.Tensor, colours: Optional[torch.Tensor], faces: torch.Tensor, cameras, images: Sequence[torch.Tensor], *,
                 cell: int, width: int, slack: float, two_sided: bool = False, size=None):
    """Bakes the pictures `images` (one float32 [3, H, W] device tensor per camera) into the atlas of the mesh.
    cameras: camera.Camera objects, or a float32 [n, 14] table with size=(W, H).  cell, width: the atlas (atlas_for).
    slack: how far behind the nearest surface at its pixel a texel may lie and still count as seen, in scene units: the
    resolution of whatever made the mesh (extract_mesh passes one voxel, or the simplification cell).  two_sided: a texel also
    takes the views that look at its triangle's back.  colours (uint8 [V, 3] or None): what an unseen texel falls back to.
    -> (texture uint8 [Ht, Wt, 3], coverage int32 [2] = owned texels coloured from the images, owned texels), on the device.
    Per run of at most 8 cameras of one size: the rasterizer (mesh_render.raster_views), then the accumulate call; one finalise at
    the end.  No host read."""
    from . import _C
    what = "bake_texture"
    _check_mesh(vertices, colours, faces, what)
    Wt, Ht = atlas_size(faces.shape[0], cell, width)
    slack = _check_slack(slack, what)
    table, runs = _camera_runs(cameras, size, what)
    images = _check_images(images, runs, vertices.device, what)
    accum = torch.zeros(Ht, Wt, 4, dtype=torch.float32, device=vertices.device)
    for start, end, W, H in runs:
        accumulate_views(vertices, faces, table[start:end], W, H, torch.stack(images[start:end]), accum, cell=cell, slack=slack, two_sided=two_sided)
    return _C.mesh_texture_finalize(vertices.shape[0], colours, faces, int(cell), Wt, accum)


# ---- render --------------------------------------------------------------------------------------------------------------
def _check_texture(texture, vertices, faces, cell, what):
    if not isinstance(texture, torch.Tensor) or texture.dtype != torch.uint8 or texture.dim() != 3 or texture.shape[2] != 3:
        raise ValueError(f"{what}: the texture is uint8 [Ht, Wt, 3]")
    if texture.device != vertices.device:
        raise ValueError(f"{what}: the texture is on {texture.device}, vertices on {vertices.device}")
    if atlas_size(faces.shape[0], cell, texture.shape[1])[1] != texture.shape[0]:
        raise ValueError(f"{what}: a texture of {texture.shape[0]} rows is not the atlas of {faces.shape[0]} triangles at cell {cell}")


def raster_views_textured(vertices, faces, texture, cell, table, W, H, bg=None, *, cull_backface=False, face_pixels=None):
    """mesh_render.raster_views with the colour fetched from the atlas -> (triangle_id, depth, alpha, colour, counts)"""
    from . import _C
    table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 14))
    if not 1 <= table.shape[0] <= MAX_VIEWS:
        raise ValueError(f"mesh_texture: 1 .. {MAX_VIEWS} views per launch")
    ws, counts = _C.mesh_raster(vertices, faces, table, W, H, bool(cull_backface), -1, -1)
    tid, depth, alpha, colour = _C.mesh_resolve_textured(vertices, faces, table, W, H, ws, bg, texture, int(cell), face_pixels)
    return tid, depth, alpha, colour, counts


def batches_textured(vertices, faces, texture, cell, cameras, bg=None, *, cull_backface=False, size=None):
    """Yields (camera indices, per-view output dicts) per launch, 8 views of one size at a time: the per-batch source
    frames.render_path takes (mesh_render.batches for a textured mesh)."""
    _check_mesh(vertices, None, faces, "batches_textured")
    _check_texture(texture, vertices, faces, cell, "batches_textured")
    table, runs = _camera_runs(cameras, size, "batches_textured")
    for start, end, W, H in runs:
        tid, depth, alpha, colour, _ = raster_views_textured(vertices, faces, texture, cell, table[start:end], W, H, bg, cull_backface=cull_backface)
        yield list(range(start, end)), [{"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]}
                                        for k in range(end - start)]


def render_textured(vertices: torch.Tensor, faces: torch.Tensor, texture: torch.Tensor, cell: int, cameras, bg: Optional[torch.Tensor] = None,
                    size=None):
    """mesh_render.render_mesh with the colour of a pixel fetched bilinearly from the atlas `texture` (uint8 [Ht, Wt, 3], cell
    parameter `cell`) -> (per view {"render", "rendered_depth", "rendered_alpha", "triangle_id"}, rejected int32 [n + 1])."""
    _check_mesh(vertices, None, faces, "render_textured")
    _check_texture(texture, vertices, faces, cell, "render_textured")
    table, runs = _camera_runs(cameras, size, "render_textured")
    outs: List[dict] = []
    rejected = torch.zeros(len(table) + 1, dtype=torch.int32, device=vertices.device)
    for start, end, W, H in runs:
        tid, depth, alpha, colour, counts = raster_views_textured(vertices, faces, texture, cell, table[start:end], W, H, bg)
        rejected[start:end] = counts[:end - start]
        rejected[-1:] = counts[MAX_VIEWS:]
        for k in range(end - start):
            outs.append({"render": colour[k], "rendered_depth": depth[k], "rendered_alpha": alpha[k], "triangle_id": tid[k]})
    return outs, rejected


# ---- files ---------------------------------------------------------------------------------------------------------------
def _host(a, dtype):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=dtype)


def write_textured_obj(path: str, vertices, faces, texture, cell: int) -> str:
    """Writes NAME.obj (a comment line `# b3gs_atlas cell <n> width <Wt>`, mtllib, v, 3 F vt, usemtl, f a/ta b/tb c/tc),
    NAME.mtl (map_Kd NAME.png) and NAME.png (frames.write_png) for path = NAME.obj; stdlib only.  Floats are written with
    repr(), which reads back to the same float32.  -> path"""
    from .frames import write_png
    stem, ext = os.path.splitext(path)
    if ext.lower() != ".obj":
        raise ValueError(f"write_textured_obj: {path} does not end in .obj")
    v, f, tex = _host(vertices, np.float32), _host(faces, np.int32), _host(texture, np.uint8)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or tex.ndim != 3 or tex.shape[2] != 3:
        raise ValueError("write_textured_obj: vertices [V, 3], faces [F, 3], texture [Ht, Wt, 3]")
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"write_textured_obj: a triangle names a vertex outside 0 .. {len(v) - 1}")
    Ht, Wt = tex.shape[:2]
    uv = face_uvs(len(f), cell, Wt, Ht).reshape(-1, 2)
    name = os.path.basename(stem)
    fmt = lambda x: repr(float(x))
    lines = [f"# b3gs_atlas cell {int(cell)} width {Wt}", f"mtllib {name}.mtl"]
    lines += ["v " + " ".join(fmt(x) for x in row) for row in v]
    lines += ["vt " + " ".join(fmt(x) for x in row) for row in uv]
    lines.append("usemtl atlas")
    lines += [f"f {a + 1}/{3 * k + 1} {b + 1}/{3 * k + 2} {c + 1}/{3 * k + 3}" for k, (a, b, c) in enumerate(f.tolist())]
    with open(path, "w", newline="\n") as fp:
        fp.write("\n".join(lines) + "\n")
    with open(stem + ".mtl", "w", newline="\n") as fp:
        fp.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {name}.png\n")
    write_png(stem + ".png", tex)
    return path


_ATLAS_LINE = re.compile(r"# b3gs_atlas cell (\d+) width (\d+)")


def read_textured_obj(path: str):
    """Reads what write_textured_obj writes -> (vertices float32 [V, 3], faces int32 [F, 3], texture uint8 [Ht, Wt, 3], cell).
    Anything else -- another line order, other texture coordinates than the atlas's, a texture of another size -- raises
    ValueError."""
    from .frames import read_png
    stem = os.path.splitext(path)[0]
    name = os.path.basename(stem)
    with open(path) as fp:
        lines = fp.read().split("\n")
    m = _ATLAS_LINE.fullmatch(lines[0]) if lines else None
    if m is None or len(lines) < 4 or lines[1] != f"mtllib {name}.mtl" or lines[-1] != "":
        raise ValueError(f"{path}: not a textured OBJ of write_textured_obj (no b3gs_atlas line)")
    cell, Wt = int(m.group(1)), int(m.group(2))
    body = lines[2:-1]
    nv = next((k for k, ln in enumerate(body) if not ln.startswith("v ")), len(body))
    nt = next((k for k, ln in enumerate(body[nv:]) if not ln.startswith("vt ")), len(body) - nv)
    if nt % 3 or nv + nt >= len(body) or body[nv + nt] != "usemtl atlas" or len(body) != nv + nt + 1 + nt // 3:
        raise ValueError(f"{path}: expected v lines, 3 vt lines per triangle, usemtl atlas and one f line per triangle")
    try:
        v = np.array([[float(x) for x in ln.split()[1:]] for ln in body[:nv]], dtype=np.float32).reshape(nv, 3)
        uv = np.array([[float(x) for x in ln.split()[1:]] for ln in body[nv:nv + nt]], dtype=np.float32).reshape(nt, 2)
        faces = []
        for k, ln in enumerate(body[nv + nt + 1:]):
            tag, *corners = ln.split()
            pairs = [tuple(int(x) for x in c.split("/")) for c in corners]
            if tag != "f" or len(pairs) != 3 or [p[1] for p in pairs] != [3 * k + 1, 3 * k + 2, 3 * k + 3]:
                raise ValueError("face line")
            faces.append([p[0] - 1 for p in pairs])
    except (ValueError, IndexError) as e:
        raise ValueError(f"{path}: line not understood ({e})") from None
    f = np.array(faces, dtype=np.int32).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= nv):
        raise ValueError(f"{path}: a triangle names a vertex outside 1 .. {nv}")
    with open(stem + ".mtl") as fp:
        if f"map_Kd {name}.png" not in fp.read().split("\n"):
            raise ValueError(f"{stem}.mtl: no map_Kd {name}.png")
    tex = read_png(stem + ".png")
    if tex.ndim != 3 or tex.shape[2] != 3 or tex.shape[1] != Wt or (tex.shape[1], tex.shape[0]) != atlas_size(len(f), cell, Wt):
        raise ValueError(f"{stem}.png: not the atlas of {len(f)} triangles at cell {cell}, width {Wt}")
    if not np.array_equal(uv.reshape(-1, 3, 2), face_uvs(len(f), cell, Wt, tex.shape[0])):
        raise ValueError(f"{path}: the texture coordinates are not those of the atlas")
    return v, f, np.ascontiguousarray(tex), cell
