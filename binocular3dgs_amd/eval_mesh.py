"""python -m binocular3dgs_amd.eval_mesh --mesh MESH.ply --gt CLOUD.ply --spacing S --max_dist D --tau T
                                         [--keep_largest K] [--min_triangles M] [--align [--align_scale] [--align_iters K]]
                                         [-m MODEL_PATH [-s SOURCE_PATH] [--iteration -1] [--views train|test|all] [--depth mean|median]]

Scores a triangle mesh (the files mesh.write_mesh_ply writes) against a reference point cloud (any PLY whose vertex element
has x, y, z), on the device: the mesh is optionally cleaned (mesh_tools.clean), sampled at `spacing` (the vertices plus a
lattice per triangle) and compared with the cloud both ways by nearest point-to-point distance capped at `max_dist`:
accuracy, completeness, chamfer, and precision, recall and F-score at `tau`.  Prints the topology line of the mesh as read
(mesh_tools.topology: edges, boundary and non-manifold edges, Euler characteristic), then the dict, and writes
mesh_results.json next to the mesh.

With -m the mesh is also rendered into the model's cameras (extract_mesh's way of finding them) and compared with the model's
own rendered depth there (mesh_render.depth_agreement): the dict goes into the result as "depth_agreement".  --depth median
compares with the model's median depth (pixel_maps.py), the depth extract_mesh --depth median fuses.

--align registers the points sampled on the mesh to the cloud first (edit.register: trimmed point-to-point ICP with pairs
within max_dist, --align_scale also fits the scale), moves the mesh by the similarity found and scores it there; the result
then holds the similarity ("align") and the scores in the mesh's own frame ("before_align").  Without the flag nothing changes.

This is the measure of the DTU surface benchmark WITHOUT its protocol: the 0.2 mm thinning of both clouds, the observation
mask and the ground plane belong to the caller, who owns those files (mesh_tools.score_clouds takes the masks).  The numbers
printed here are not DTU numbers.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="score a triangle mesh against a reference point cloud (point-to-point, both ways)")
    p.add_argument("--mesh", required=True)
    p.add_argument("--gt", required=True)
    p.add_argument("--spacing", type=float, required=True, help="lattice spacing of the points sampled on the mesh")
    p.add_argument("--max_dist", type=float, required=True, help="distances are capped here")
    p.add_argument("--tau", type=float, required=True, help="threshold of precision / recall / F-score")
    p.add_argument("--keep_largest", type=int, default=0)
    p.add_argument("--min_triangles", type=int, default=0)
    p.add_argument("--align", action="store_true", help="register the mesh to the cloud (ICP) before scoring")
    p.add_argument("--align_scale", action="store_true", help="with --align: fit the scale as well")
    p.add_argument("--align_iters", type=int, default=30)
    p.add_argument("-m", "--model_path", default=None, help="also compare the mesh with this model's rendered depth")
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("--views", choices=("train", "test", "all"), default="test")
    p.add_argument("--depth", choices=("mean", "median"), default="mean", help="with -m: the model's depth the mesh is compared with")
    return p


def run(mesh_path: str, gt_path: str, spacing: float, max_dist: float, tau: float, keep_largest: int = 0, min_triangles: int = 0,
        device="cuda", model_path=None, source_path=None, iteration: int = -1, views: str = "test", depth: str = "mean",
        align: bool = False, align_scale: bool = False, align_iters: int = 30) -> dict:
    from . import mesh, mesh_tools
    from .init_points import read_ply_vertices
    v, c, f = mesh.read_mesh_ply(mesh_path)
    rows = read_ply_vertices(gt_path)
    gt = torch.from_numpy(np.stack([rows["x"], rows["y"], rows["z"]], axis=1).astype(np.float32)).to(device)
    vertices, colours, faces = torch.from_numpy(v).to(device), torch.from_numpy(c).to(device), torch.from_numpy(f).to(device)
    print(mesh_tools.topology_line(mesh_tools.topology(vertices, faces)))
    if keep_largest or min_triangles:
        vertices, colours, faces = mesh_tools.clean(vertices, colours, faces, keep_largest, min_triangles)
    if align:
        from . import edit
        before = mesh_tools.score_mesh(vertices, faces, gt, spacing, max_dist, tau)
        T, hist = edit.register(mesh_tools.sample_surface(vertices, faces, spacing), gt, max_dist=max_dist, iterations=align_iters,
                                with_scale=align_scale)
        aligned = {"matrix": T.matrix().tolist(), "s": T.s, "iterations": len(hist), "pairs": hist[-1][0], "rms": hist[-1][1]}
        print("align: " + json.dumps(aligned))
        print("before: " + json.dumps(before))
        model_vertices, vertices = vertices, edit.transform_points(vertices, T)     # (now in the cloud's frame, the frame of spacing)
    result = mesh_tools.score_mesh(vertices, faces, gt, spacing, max_dist, tau)
    if align:
        result.update({"align": aligned, "before_align": before})
        vertices = model_vertices          # (the model's cameras see the mesh in its own frame)
    result.update({"mesh": os.path.abspath(mesh_path), "gt": os.path.abspath(gt_path), "spacing": spacing,
                   "vertices": int(vertices.shape[0]), "triangles": int(faces.shape[0]), "keep_largest": keep_largest,
                   "min_triangles": min_triangles})
    if model_path is not None:
        result["depth_agreement"] = model_depth_agreement(model_path, vertices, faces, source_path, iteration, views, device, depth)
    with open(os.path.join(os.path.dirname(os.path.abspath(mesh_path)), "mesh_results.json"), "w") as fp:
        json.dump(result, fp, indent=2)
    return result


def model_depth_agreement(model_path: str, vertices, faces, source_path=None, iteration: int = -1, views: str = "test", device="cuda",
                          depth: str = "mean") -> dict:
    """mesh_render.depth_agreement against the trained model of `model_path` in its own cameras"""
    from . import mesh_render
    from .extract_mesh import load_cameras
    from .gaussian_model import GaussianModel
    from .spiral import max_iteration, read_cfg_args
    cfg = read_cfg_args(model_path)
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(int(cfg.get("sh_degree", 1)))
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it), "point_cloud.ply"))
    cams = load_cameras(model_path, cfg, source_path, views, device)
    if not cams:
        raise ValueError(f"no {views} cameras")
    white = bool(cfg.get("white_background", False))
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device=device)
    out = mesh_render.depth_agreement(model, vertices, faces, cams, bg, depth=depth)
    out.update({"model": os.path.abspath(model_path), "iteration": it, "camera_set": views})
    return out


def main(argv=None) -> int:
    a = parser().parse_args(argv)
    print(json.dumps(run(a.mesh, a.gt, a.spacing, a.max_dist, a.tau, a.keep_largest, a.min_triangles,
                         model_path=a.model_path, source_path=a.source_path, iteration=a.iteration, views=a.views, depth=a.depth,
                         align=a.align, align_scale=a.align_scale, align_iters=a.align_iters)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
