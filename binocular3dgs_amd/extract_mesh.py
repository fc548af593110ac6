"""python -m binocular3dgs_amd.extract_mesh -m MODEL_PATH [-s SOURCE_PATH] [--iteration -1] [--views train|test|all]
                                            [--resolution 256 | --voxel_size S] [--truncation_voxels 4] [--alpha_min 0.5]
                                            [--min_weight 1] [--depth mean|median] [--bounds x0 y0 z0 x1 y1 z1]
                                            [--method tsdf|poisson [--screen 4] [--poisson_iters K] [--poisson_tol 1e-4]
                                             [--sample_stride 1] [--spread 1] [--trim 0]]
                                            [--keep_largest 0] [--min_triangles 0] [--cull_unseen [--min_pixels 1]]
                                            [--smooth N [--smooth_lambda 0.5] [--smooth_mu -0.53] [--free_boundary]] [--normals]
                                            [--simplify K | --target_triangles N] [--placement quadric|mean]
                                            [--texture [--texel_cell N | --atlas_side S] [--texture_from render|gt]
                                             [--texture_slack X] [--two_sided]]

A triangle mesh of a trained model: the point cloud <model_path>/point_cloud/iteration_<it>/point_cloud.ply is rendered from
the chosen cameras, depth, alpha and colour are fused into a TSDF volume and the zero level set is extracted, all on the
device (mesh.fuse_model).  Writes <model_path>/mesh/iteration_<it>/mesh.ply (binary PLY, coloured vertices) and prints the
voxel, vertex and triangle counts.  --depth median fuses the depth at which a pixel's transmittance crosses one half
(pixel_maps.py) in place of the alpha-weighted mean, which lies between the surfaces where a semi-transparent Gaussian hangs in
front of one.  --method poisson fits one smooth function to oriented samples of the same renders (poisson.py: screened Poisson
reconstruction, conjugate gradients on the device) in place of the TSDF, whose surface only exists where a view looked: the mesh
is closed also behind what the views saw.  --screen weighs the samples against smoothness, --poisson_iters and --poisson_tol
bound the solver (default: four times the longest axis, relative residual 1e-4), --sample_stride takes every S-th pixel, --trim W > 0
keeps only the cells whose corners have W of sample weight within --spread nodes (0: every cell, the watertight mesh).  It
composes with --depth median and every step below, and prints the iterations done, the final relative residual and the
topology line of the extracted mesh.  --keep_largest K keeps the K components with the most triangles (ties at the K-th
all survive), --min_triangles M the components with at least M (mesh_tools.clean); with both at 0 the step is not run.
--cull_unseen renders the mesh into the cameras of --views (mesh_render.cull_unseen) and drops the triangles that win fewer
than --min_pixels pixels over all of them, e.g. blobs inside or behind the observed surface; it runs after the cleaning step
and before the simplification.
--smooth N runs N iterations of Taubin's filter on the vertices (mesh_tools.smooth: pairs of steps with --smooth_lambda and
--smooth_mu, mu < -lambda, or mu = 0 for a plain Laplacian filter); it runs after --cull_unseen and before the simplification,
keeps the ends of boundary and non-manifold edges in place unless --free_boundary is given, and prints the vertex count, the
step count and the topology line (mesh_tools.topology).  --normals computes area-weighted vertex normals of the final mesh
(mesh_tools.vertex_normals) and writes them into mesh.ply as nx ny nz.
--simplify K clusters the vertices on a grid of K voxels (mesh_tools.simplify), --target_triangles N searches the smallest
such grid that leaves at most N triangles (mesh_tools.simplify_to); either runs after the cleaning step and prints the counts
before and after.  --placement says where a cluster's vertex goes: the minimiser of its faces' quadric, or the members' mean.
--texture bakes the pictures of the cameras of --views into a texture atlas (mesh_texture.bake_texture) and writes mesh.obj,
mesh.mtl and mesh.png next to mesh.ply; it runs last, on the mesh that mesh.ply holds, and prints the atlas size and the share of
its texels coloured from the pictures (the others keep the vertex colours).  The pictures are the model's renders
(--texture_from render, the default) or the cameras' own images (gt, which needs the dataset).  --texel_cell N gives every
triangle a patch with legs of N - 2 texels; the default is the largest N whose atlas fits a square of --atlas_side (4096)
texels.  --texture_slack is how far behind the nearest surface a texel may lie and still be seen; the default is one voxel of
the fusion, or the simplification cell when that is larger: neither resolves two surfaces closer than that.

The model and the cameras are found the way spiral.py finds them: source path, images folder, image resolution, background,
SH degree, dataset name and view count come from <model_path>/cfg_args; the command line wins.  A model folder whose dataset
is not at hand still works with --views all: the cameras are then those of <model_path>/cameras.json, at the size it records.
--resolution is the number of voxels along the longest axis of the bounds (NOT the image resolution, which is cfg_args').
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="extract a triangle mesh from a trained model (TSDF fusion of rendered depth)")
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--views", choices=("train", "test", "all"), default="train")
    size = p.add_mutually_exclusive_group()
    size.add_argument("--resolution", type=int, default=None, help="voxels along the longest axis of the bounds (default 256)")
    size.add_argument("--voxel_size", type=float, default=None)
    p.add_argument("--truncation_voxels", type=float, default=4.0)
    p.add_argument("--alpha_min", type=float, default=0.5)
    p.add_argument("--min_weight", type=float, default=1.0)
    p.add_argument("--depth", choices=("mean", "median"), default="mean",
                   help="the depth of a pixel that is fused: the alpha-weighted mean, or the depth at which the transmittance crosses 1/2")
    p.add_argument("--method", choices=("tsdf", "poisson"), default="tsdf", help="TSDF fusion, or a screened Poisson fit of oriented samples (watertight)")
    p.add_argument("--screen", type=_positive_float, default=None, metavar="A", help="with --method poisson: weight of the samples (default 4)")
    p.add_argument("--poisson_iters", type=_positive_int, default=None, metavar="K", help="with --method poisson: CG iterations (default 4 x longest axis)")
    p.add_argument("--poisson_tol", type=float, default=None, metavar="T", help="with --method poisson: relative residual that stops the solver (default 1e-4)")
    p.add_argument("--sample_stride", type=_positive_int, default=None, metavar="S", help="with --method poisson: every S-th pixel is a sample (default 1)")
    p.add_argument("--spread", type=int, default=None, metavar="R", help="with --method poisson: nodes around a node whose sample weight supports it (default 1)")
    p.add_argument("--trim", type=float, default=None, metavar="W", help="with --method poisson: drop cells with less support than W (default 0: watertight)")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    p.add_argument("--keep_largest", type=int, default=0, help="keep the K largest connected components (0: all)")
    p.add_argument("--min_triangles", type=int, default=0, help="drop the components with fewer triangles (0: none)")
    simp = p.add_mutually_exclusive_group()
    simp.add_argument("--simplify", type=_positive_float, default=None, metavar="K",
                      help="cluster the vertices on a grid whose cell is K voxels (K > 0)")
    simp.add_argument("--target_triangles", type=_positive_int, default=None, metavar="N",
                      help="search the smallest cell that leaves at most N triangles")
    p.add_argument("--placement", choices=("quadric", "mean"), default="quadric", help="where a cluster's vertex goes")
    p.add_argument("--cull_unseen", action="store_true", help="drop the triangles no camera of --views sees")
    p.add_argument("--min_pixels", type=_positive_int, default=1, help="with --cull_unseen: pixels a triangle must win to stay")
    p.add_argument("--smooth", type=_positive_int, default=None, metavar="N", help="N iterations of Taubin's filter before the simplification")
    p.add_argument("--smooth_lambda", type=float, default=None, metavar="L", help="with --smooth: the shrinking factor, in (0, 1] (default 0.5)")
    p.add_argument("--smooth_mu", type=float, default=None, metavar="M",
                   help="with --smooth: the inflating factor, below -lambda, or 0 for a plain Laplacian filter (default -0.53)")
    p.add_argument("--free_boundary", action="store_true", help="with --smooth: boundary and non-manifold vertices move too")
    p.add_argument("--normals", action="store_true", help="write area-weighted vertex normals into mesh.ply")
    p.add_argument("--texture", action="store_true", help="also write mesh.obj, mesh.mtl and mesh.png: a texture atlas baked from the views")
    atlas = p.add_mutually_exclusive_group()
    atlas.add_argument("--texel_cell", type=_positive_int, default=None, metavar="N", help="with --texture: the cell parameter, 4 .. 256")
    atlas.add_argument("--atlas_side", type=_positive_int, default=None, metavar="S",
                       help="with --texture: the largest cell whose atlas fits S x S texels (default 4096)")
    p.add_argument("--texture_from", choices=("render", "gt"), default="render", help="with --texture: the model's renders or the dataset's images")
    p.add_argument("--texture_slack", type=float, default=None, metavar="X",
                   help="with --texture: depth tolerance of the visibility test (default: one voxel, or the simplification cell)")
    p.add_argument("--two_sided", action="store_true", help="with --texture: a texel also takes the views that see its triangle from behind")
    return p


def _positive_float(text: str) -> float:
    v = float(text)
    if not (v > 0.0 and v < float("inf")):
        raise argparse.ArgumentTypeError("a positive, finite number is needed")
    return v


def _positive_int(text: str) -> int:
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError("at least 1")
    return v


def cameras_from_json(path: str, device="cuda"):
    """The cameras of a cameras.json (dataset_readers.camera_json / the reference's camera_to_JSON), without images."""
    from .camera import Camera, focal2fov
    with open(path) as fp:
        entries = json.load(fp)
    cams = []
    for e in entries:
        R = np.asarray(e["rotation"], dtype=np.float64)                 # camera -> world
        T = -R.T @ np.asarray(e["position"], dtype=np.float64)          # world -> camera translation
        W, H = int(e["width"]), int(e["height"])
        cams.append(Camera(R, T, focal2fov(e["fx"], W), focal2fov(e["fy"], H), W, H, uid=int(e["id"]), device=device,
                           image_name=e.get("img_name")))
    return cams


def load_cameras(model_path: str, cfg: dict, source_path, views: str, device="cuda"):
    source_path = source_path or cfg.get("source_path")
    if source_path and os.path.isdir(source_path):
        from .scene import Scene
        scene = Scene.from_dataset(source_path, None, images=cfg.get("images", "images"), eval=bool(cfg.get("eval", False)),
                                   n_views=int(cfg.get("n_views", 3)), dataset_name=cfg.get("dataset_name", "LLFF"),
                                   suffix=cfg.get("suffix"), resolution=cfg.get("resolution", -1),
                                   white_background=bool(cfg.get("white_background", False)),
                                   init_points=cfg.get("init_points", "matcher"), shuffle=False, device=device)
        train, test = scene.getTrainCameras(), scene.getTestCameras()
        return {"train": train, "test": test, "all": train + test}[views]
    path = os.path.join(model_path, "cameras.json")
    if views != "all" or not os.path.exists(path):
        raise ValueError("no dataset folder: pass -s, or use --views all next to the model's cameras.json")
    return cameras_from_json(path, device)


def run(model_path: str, source_path=None, iteration: int = -1, views: str = "train", resolution=None, voxel_size=None,
        truncation_voxels: float = 4.0, alpha_min: float = 0.5, min_weight: float = 1.0, bounds=None,
        keep_largest: int = 0, min_triangles: int = 0, simplify=None, target_triangles=None, placement: str = "quadric",
        cull_unseen: bool = False, min_pixels: int = 1, texture: bool = False, texel_cell=None, atlas_side=None,
        texture_from: str = "render", texture_slack=None, two_sided: bool = False, smooth=None, smooth_lambda: float = 0.5,
        smooth_mu: float = -0.53, free_boundary: bool = False, normals: bool = False, depth: str = "mean", method: str = "tsdf",
        screen=None, poisson_iters=None, poisson_tol=None, sample_stride: int = 1, spread: int = 1, trim: float = 0.0) -> str:
    from . import mesh
    from .gaussian_model import GaussianModel
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it), "point_cloud.ply"))
    cams = load_cameras(model_path, cfg, source_path, views)
    if not cams:
        raise ValueError(f"no {views} cameras")
    white = bool(cfg.get("white_background", False))
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    t0 = time.perf_counter()
    solver = {}
    vertices, colours, faces, vol = mesh.fuse_model(
        model, cams, bg, resolution=resolution, voxel_size=voxel_size, bounds=None if bounds is None else (bounds[:3], bounds[3:]),
        truncation_voxels=truncation_voxels, alpha_min=alpha_min, min_weight=min_weight, return_volume=True, depth=depth, method=method,
        screen=screen, poisson_iters=poisson_iters, poisson_tol=poisson_tol, sample_stride=sample_stride, spread=spread, trim=trim, info=solver)
    if method == "poisson":
        from . import mesh_tools
        print(f"poisson: {solver['samples']} samples ({solver['dropped']} outside the grid), {solver['iterations']} iterations, "
              f"relative residual {solver['residual']:.3e}")
        if faces.shape[0]:
            print(mesh_tools.topology_line(mesh_tools.topology(vertices, faces)))
    if keep_largest or min_triangles:
        from . import mesh_tools
        vertices, colours, faces, st = mesh_tools.clean(vertices, colours, faces, keep_largest, min_triangles, return_stats=True)
        print(f"{st['components']} components, {st['kept']} kept: dropped {st['vertices_dropped']} vertices, "
              f"{st['triangles_dropped']} triangles")
    if cull_unseen:
        from . import mesh_render
        before = (vertices.shape[0], faces.shape[0])
        vertices, colours, faces = mesh_render.cull_unseen(vertices, colours, faces, cams, min_pixels)
        print(f"culled: {before[1] - faces.shape[0]} of {before[1]} triangles seen by no camera, {before[0] - vertices.shape[0]} vertices")
    if smooth is not None:
        from . import mesh_tools
        adj = mesh_tools.adjacency(vertices, faces)
        vertices = mesh_tools.smooth(vertices, faces, smooth, smooth_lambda, smooth_mu, not free_boundary, adjacency=adj)
        steps = smooth * (2 if smooth_mu != 0.0 else 1)
        print(f"smoothed: {vertices.shape[0]} vertices, {steps} steps (lambda {smooth_lambda:g}, mu {smooth_mu:g}, "
              f"boundary {'free' if free_boundary else 'pinned'})")
        print(mesh_tools.topology_line(mesh_tools.topology(vertices, faces, adjacency=adj)))
    simplify_cell = 0.0
    if simplify is not None or target_triangles is not None:
        from . import mesh_tools
        before = (vertices.shape[0], faces.shape[0])
        if simplify is not None:
            cell = float(simplify) * vol.voxel_size
            vertices, colours, faces = mesh_tools.simplify(vertices, colours, faces, cell, placement)
        else:
            vertices, colours, faces, cell = mesh_tools.simplify_to(vertices, colours, faces, target_triangles, placement)
        print(f"simplified ({placement}, cell {cell:g} = {cell / vol.voxel_size:g} voxels): {before[0]} vertices, {before[1]} triangles "
              f"-> {vertices.shape[0]} vertices, {faces.shape[0]} triangles")
        simplify_cell = float(cell)
    out_dir = os.path.join(model_path, "mesh", "iteration_{}".format(it))
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "mesh.ply")
    if normals:
        from . import mesh_tools
        mesh.write_mesh_ply(out, vertices, colours, faces, mesh_tools.vertex_normals(vertices, faces))
    else:
        mesh.write_mesh_ply(out, vertices, colours, faces)
    dt = time.perf_counter() - t0
    nx, ny, nz = vol.dims
    print(f"{len(cams)} views -> {nx} x {ny} x {nz} voxels of {vol.voxel_size:g}: {vertices.shape[0]} vertices, "
          f"{faces.shape[0]} triangles -> {out} in {dt:.2f} s")
    if texture:
        slack = max(vol.voxel_size, simplify_cell) if texture_slack is None else texture_slack
        _write_texture(os.path.join(out_dir, "mesh.obj"), model, cams, bg, vertices, colours, faces, texel_cell, atlas_side, texture_from,
                       slack, two_sided)
    return out


def _write_texture(path, model, cams, bg, vertices, colours, faces, texel_cell, atlas_side, texture_from, slack, two_sided):
    from . import mesh_texture
    t0 = time.perf_counter()
    if faces.shape[0] == 0:
        raise ValueError("--texture: the mesh has no triangles")
    if texture_from == "gt":
        images = [c.original_image for c in cams]
        if any(im is None for im in images):
            raise ValueError("--texture_from gt needs the dataset's images: pass -s")
        images = [im[:3].float().contiguous() for im in images]
    else:
        from .evaluate import render_views
        images = render_views(model, cams, bg)
    if texel_cell is not None:                                        # about as many cells per row as rows of cells
        cell, cells = int(texel_cell), (faces.shape[0] + 1) // 2
        width = min(math.isqrt(cells - 1) + 1, mesh_texture.MAX_SIDE // (cell + 1)) * (cell + 1)
    else:
        cell, width = mesh_texture.atlas_for(faces.shape[0], 4096 if atlas_side is None else int(atlas_side))
    tex, coverage = mesh_texture.bake_texture(vertices, colours, faces, cams, images, cell=cell, width=width, slack=slack, two_sided=two_sided)
    seen, owned = coverage.tolist()
    mesh_texture.write_textured_obj(path, vertices, faces, tex, cell)
    print(f"texture ({texture_from}, slack {slack:g}): cell {cell}, atlas {tex.shape[1]} x {tex.shape[0]}, {seen} of {owned} texels "
          f"({100.0 * seen / max(owned, 1):.1f} %) coloured from {len(cams)} views -> {path} in {time.perf_counter() - t0:.2f} s")


def main(argv=None) -> int:
    p = parser()
    a = p.parse_args(argv)
    if not a.texture and (a.texel_cell is not None or a.atlas_side is not None or a.texture_from != "render" or a.texture_slack is not None or a.two_sided):
        p.error("--texel_cell, --atlas_side, --texture_from, --texture_slack and --two_sided need --texture")
    if a.smooth is None and (a.smooth_lambda is not None or a.smooth_mu is not None or a.free_boundary):
        p.error("--smooth_lambda, --smooth_mu and --free_boundary need --smooth")
    lam = 0.5 if a.smooth_lambda is None else a.smooth_lambda
    mu = -0.53 if a.smooth_mu is None else a.smooth_mu
    if not (0.0 < lam <= 1.0):
        p.error("--smooth_lambda is in (0, 1]")
    if not (mu == 0.0 or mu < -lam):
        p.error("--smooth_mu is below -lambda, or 0")
    if a.method != "poisson" and any(v is not None for v in (a.screen, a.poisson_iters, a.poisson_tol, a.sample_stride, a.spread, a.trim)):
        p.error("--screen, --poisson_iters, --poisson_tol, --sample_stride, --spread and --trim need --method poisson")
    if a.poisson_tol is not None and not (a.poisson_tol >= 0.0 and a.poisson_tol < float("inf")):
        p.error("--poisson_tol is at least 0 and finite")
    if a.spread is not None and not 0 <= a.spread <= 1024:
        p.error("--spread is 0 .. 1024")
    if a.trim is not None and not (a.trim >= 0.0 and a.trim < float("inf")):
        p.error("--trim is at least 0 and finite")
    if a.texture_slack is not None and not (a.texture_slack >= 0.0 and a.texture_slack < float("inf")):
        p.error("--texture_slack is at least 0 and finite")
    run(a.model_path, a.source_path, a.iteration, a.views, a.resolution, a.voxel_size, a.truncation_voxels, a.alpha_min,
        a.min_weight, a.bounds, a.keep_largest, a.min_triangles, a.simplify, a.target_triangles, a.placement, a.cull_unseen, a.min_pixels,
        a.texture, a.texel_cell, a.atlas_side, a.texture_from, a.texture_slack, a.two_sided, a.smooth, lam, mu, a.free_boundary, a.normals, a.depth,
        a.method, a.screen, a.poisson_iters, a.poisson_tol, 1 if a.sample_stride is None else a.sample_stride, 1 if a.spread is None else a.spread,
        0.0 if a.trim is None else a.trim)
    return 0


if __name__ == "__main__":
    sys.exit(main())
