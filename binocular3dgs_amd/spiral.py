"""python -m binocular3dgs_amd.spiral -m MODEL_PATH [-s SOURCE_PATH] [--iteration -1] [--resolution R] [--white_background]
                                      [--video] [--no_png] [--fps 25] [--quality 90] [--mesh MESH.ply|MESH.obj [--shading colour|normal|smooth|lit|texture]]
                                      [--maps median,std,id]

The reference's spiral.py: the trained point cloud <model_path>/point_cloud/iteration_<it>/point_cloud.ply, rendered along the
180-frame spiral of <source_path>/poses_bounds.npy (DTU when the source path contains 'scan'), written as %05d.png,
depth_%05d.png and cdepth_%05d.png to <model_path>/render/ours_<it>/.  Renders and frame encoding run in batches on the
device (frames.render_path).  --video also encodes the three streams as baseline JPEG on the device and writes
<model_path>/out_<scene>.avi, out_depth_<scene>.avi and out_cdepth_<scene>.avi (Motion-JPEG in AVI; the reference makes H.264
MP4 files of these names with ffmpeg); --no_png then skips the PNG files.  Without --video the ffmpeg lines are printed.

--mesh renders a triangle mesh (the files extract_mesh writes) along the same spiral in place of the model
(mesh_render.render_mesh; --shading normal shows the face normals), through the same frame and video encoders, into
<model_path>/render/mesh_<scene>/ and out_mesh_<scene>.avi, out_depth_mesh_<scene>.avi, out_cdepth_mesh_<scene>.avi: the
model's own outputs are never overwritten, and its point cloud is not read.  A MESH.obj is the textured mesh
extract_mesh --texture writes (with its .mtl and .png); it is rendered through its atlas (mesh_texture.batches_textured):
--shading texture is implied by the extension, and is an error for a .ply.  --shading smooth and lit shade a .ply from its
vertex normals (mesh_render.batches_shaded: the interpolated normal as a colour, or a grey headlight); the normals are those of
the file (extract_mesh --normals) and are computed on load (mesh_tools.vertex_normals) when it has none.

--maps also writes pictures of the per-pixel geometry maps (pixel_maps.py) of every frame into the same folder: median_%05d.png
and cmedian_%05d.png (the depth at which the transmittance crosses one half, gray and turbo, encoded as depth_ and cdepth_
are), std_%05d.png and cstd_%05d.png (the spread of the depth along the ray), id_%05d.png (the Gaussian with the largest
weight, hashed to a colour); with --video also out_median_<scene>.avi, out_cmedian_, out_std_, out_cstd_, out_id_.  Not with
--mesh.

Defaults for source_path, sh_degree, resolution and white_background come from <model_path>/cfg_args when it exists (the
Namespace(...) line train.py writes, read with `ast`: literals only, nothing is executed); the command line wins.
"""
from __future__ import annotations

import argparse
import ast
import os
import sys
import time

import torch


def read_cfg_args(model_path: str) -> dict:
    """The keyword literals of <model_path>/cfg_args ("Namespace(k=v, ...)"); {} when missing or not of that form."""
    path = os.path.join(model_path, "cfg_args")
    if not os.path.exists(path):
        return {}
    with open(path) as fp:
        text = fp.read()
    try:
        node = ast.parse(text.strip(), mode="eval").body
    except SyntaxError:
        return {}
    if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "Namespace"):
        return {}
    out = {}
    for kw in node.keywords:
        try:
            out[kw.arg] = ast.literal_eval(kw.value)
        except ValueError:
            pass
    return out


def max_iteration(model_path: str) -> int:
    """utils/system_utils.py searchForMaxIteration over <model_path>/point_cloud/iteration_<n>; a folder whose suffix is no
    number (iteration_<n>_pruned of prune.py) is no iteration of the training run and is passed over."""
    names = os.listdir(os.path.join(model_path, "point_cloud"))
    its = [int(n.split("_")[-1]) for n in names if n.startswith("iteration_") and n.split("_")[-1].isdigit()]
    if not its:
        raise FileNotFoundError(f"no point_cloud/iteration_* under {model_path}")
    return max(its)


def run(model_path: str, source_path: str = None, iteration: int = -1, resolution=None, white_background=None,
        sh_degree=None, n_frames: int = 180, video: bool = False, png: bool = True, fps: float = 25.0, quality: int = 90,
        mesh_path: str = None, shading: str = None, maps=None) -> str:
    from . import camera_path, frames
    from .gaussian_model import GaussianModel
    if mesh_path is not None and maps:
        raise ValueError("--maps are maps of the model: not with --mesh")
    if mesh_path is not None:
        return _run_mesh(model_path, source_path, resolution, white_background, n_frames, video, png, fps, quality, mesh_path, shading)
    cfg = read_cfg_args(model_path)
    source_path = source_path or cfg.get("source_path")
    if not source_path:
        raise ValueError("no source path: pass -s or keep cfg_args next to the model")
    resolution = resolution if resolution is not None else cfg.get("resolution", -1)
    white = white_background if white_background is not None else bool(cfg.get("white_background", False))
    sh = sh_degree if sh_degree is not None else int(cfg.get("sh_degree", 1))
    it = max_iteration(model_path) if iteration == -1 else iteration
    model = GaussianModel(sh)
    model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(it), "point_cloud.ply"))
    cams = camera_path.spiral_cameras_from_dir(source_path, n_frames=n_frames, resolution=resolution, device="cuda")
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    out_dir = os.path.join(model_path, "render", "ours_{}".format(it))
    scene = os.path.basename(os.path.normpath(source_path))
    t0 = time.perf_counter()
    if video:
        res = frames.render_path(model, cams, bg, out_dir, video=(model_path, scene), png=png, fps=fps, quality=quality)
        dt = time.perf_counter() - t0
        where = out_dir if png else "no PNG files"
        print(f"{len(cams)} frames ({cams[0].image_width}x{cams[0].image_height}) -> {where} in {dt:.2f} s")
        print(f"video (Motion-JPEG AVI, {fps:g} fps, quality {quality}):")
        for path in res["video"]:
            print(f"  {path}")
        if maps:
            _run_maps(model, cams, bg, out_dir, maps, (model_path, scene), png, fps, quality)
        return out_dir
    frames.render_path(model, cams, bg, out_dir)
    dt = time.perf_counter() - t0
    print(f"{len(cams)} frames ({cams[0].image_width}x{cams[0].image_height}) -> {out_dir} in {dt:.2f} s")
    if maps:
        _run_maps(model, cams, bg, out_dir, maps, None, True, fps, quality)
    print("video (not encoded here):")
    for pat, out in (("%05d.png", "out_{}.mp4"), ("depth_%05d.png", "out_depth_{}.mp4"), ("cdepth_%05d.png", "out_cdepth_{}.mp4")):
        print(f"  ffmpeg -i {os.path.join(out_dir, pat)} -q 2 {os.path.join(model_path, out.format(scene))} -y")
    return out_dir


def _run_maps(model, cams, bg, out_dir, maps, video, png, fps, quality):
    from . import pixel_maps
    t0 = time.perf_counter()
    res = pixel_maps.render_map_frames(model, cams, bg, out_dir, maps, video=video, png=png, fps=fps, quality=quality)
    print(f"maps ({', '.join(maps)}): {len(res['png'])} PNG files -> {out_dir if png else 'no PNG files'} in {time.perf_counter() - t0:.2f} s")
    for path in res["video"]:
        print(f"  {path}")


def _run_mesh(model_path, source_path, resolution, white_background, n_frames, video, png, fps, quality, mesh_path, shading) -> str:
    from . import camera_path, frames, mesh, mesh_render
    textured = mesh_path.lower().endswith(".obj")
    if shading is None:
        shading = "texture" if textured else "colour"
    if textured != (shading == "texture"):
        raise ValueError(f"--shading {shading} with {os.path.basename(mesh_path)}: texture goes with a textured .obj, colour, normal, smooth and lit with a .ply")
    cfg = read_cfg_args(model_path)
    source_path = source_path or cfg.get("source_path")
    if not source_path:
        raise ValueError("no source path: pass -s or keep cfg_args next to the model")
    resolution = resolution if resolution is not None else cfg.get("resolution", -1)
    white = white_background if white_background is not None else bool(cfg.get("white_background", False))
    if textured:
        from . import mesh_texture
        hv, hf, htex, cell = mesh_texture.read_textured_obj(mesh_path)
        v, f, tex = (torch.from_numpy(a).to("cuda") for a in (hv, hf, htex))
    else:
        hv, hc, hf, hn = mesh.read_mesh_ply(mesh_path, return_normals=True)
        v, c, f = (torch.from_numpy(a).to("cuda") for a in (hv, hc, hf))
        if shading in mesh_render.SHADED:
            from . import mesh_tools
            nrm = mesh_tools.vertex_normals(v, f) if hn is None else torch.from_numpy(hn).to("cuda")
    cams = camera_path.spiral_cameras_from_dir(source_path, n_frames=n_frames, resolution=resolution, device="cuda")
    bg = torch.tensor([1.0, 1.0, 1.0] if white else [0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    stem = "mesh_" + os.path.basename(os.path.normpath(source_path))
    out_dir = os.path.join(model_path, "render", stem)
    t0 = time.perf_counter()
    if textured:
        source = mesh_texture.batches_textured(v, f, tex, cell, cams, bg)
    elif shading in mesh_render.SHADED:
        source = mesh_render.batches_shaded(v, nrm, f, cams, bg, mode=shading)
    else:
        source = mesh_render.batches(v, c, f, cams, bg, shading=shading)
    res = frames.render_path(None, cams, bg, out_dir, video=(model_path, stem) if video else None, png=png, fps=fps, quality=quality,
                             source=source)
    dt = time.perf_counter() - t0
    print(f"{len(cams)} frames ({cams[0].image_width}x{cams[0].image_height}) of {f.shape[0]} triangles ({shading}) -> "
          f"{out_dir if png else 'no PNG files'} in {dt:.2f} s")
    if video:
        for path in res["video"]:
            print(f"  {path}")
    return out_dir


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="render the spiral path of a trained model (spiral.py)")
    p.add_argument("-m", "--model_path", required=True)
    p.add_argument("-s", "--source_path", default=None)
    p.add_argument("--iteration", type=int, default=-1)
    p.add_argument("-r", "--resolution", type=int, default=None)
    p.add_argument("-w", "--white_background", action="store_true", default=None)
    p.add_argument("--sh_degree", type=int, default=None)
    p.add_argument("--frames", type=int, default=180, help="frames of the spiral (the reference: 180)")
    p.add_argument("--video", action="store_true", help="also write out_<scene>.avi, out_depth_<scene>.avi, out_cdepth_<scene>.avi")
    p.add_argument("--no_png", action="store_true", help="with --video: write no PNG files")
    p.add_argument("--fps", type=float, default=25.0, help="frame rate of the videos (ffmpeg's default for an image sequence)")
    p.add_argument("--quality", type=int, default=90, help="JPEG quality of the video frames, 1..100")
    p.add_argument("--mesh", default=None, help="render this triangle mesh (PLY, or a textured OBJ) along the spiral in place of the model")
    p.add_argument("--shading", choices=("colour", "normal", "smooth", "lit", "texture"), default=None,
                   help="with --mesh: vertex colours (the default for a .ply), face normals, vertex normals as colours (smooth) or as a grey "
                        "headlight (lit), or the atlas (implied by a .obj)")
    p.add_argument("--maps", default=None, metavar="median,std,id",
                   help="also write pictures of the per-pixel geometry maps: median depth, depth spread, dominant Gaussian")
    a = p.parse_args(argv)
    if a.no_png and not a.video:
        p.error("--no_png needs --video")
    maps = None
    if a.maps is not None:
        maps = tuple(m for m in a.maps.split(",") if m)
        if not maps or any(m not in ("median", "std", "id") for m in maps):
            p.error("--maps is a comma-separated list out of median, std, id")
        if a.mesh is not None:
            p.error("--maps are maps of the model: not with --mesh")
    run(a.model_path, a.source_path, a.iteration, a.resolution, a.white_background, a.sh_degree, a.frames,
        video=a.video, png=not a.no_png, fps=a.fps, quality=a.quality, mesh_path=a.mesh, shading=a.shading, maps=maps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
