"""Per-pixel geometry maps of a model's renders: median depth, depth spread along the ray, and which Gaussian a pixel shows.

render_maps() renders the cameras as evaluate.py and importance.py do (up to 8 views of one W x H per b3gs_forward_raw_batch
launch on the evaluation-owned FusedRasterizer, no gradients) and, after every launch, walks the tile lists that forward left
on the device a second time (b3gs_blend_pixel_maps_batch, csrc/pixelmaps.hip).  Every blended (pixel, Gaussian) has the weight
w = alpha * T, T the transmittance in front of it, and the camera-space depth d of the Gaussian's centre; per pixel:

    median_depth  d of the last blended Gaussian whose T before the blend was > 0.5: the depth at which the transmittance
                  crosses one half (the depth 2DGS, RaDe-GS and GOF fuse).  A pixel that never reaches T = 0.5 (alpha < 0.5)
                  takes its last blended Gaussian; 0 where nothing was blended.  A copy of a float, never an average: always
                  a depth at which a Gaussian sits.
    depth_mean    sum(w d) / alpha -- rendered_depth / rendered_alpha, the depth the TSDF fusion uses by default; between the
                  surfaces where a semi-transparent Gaussian hangs in front of one.  0 where alpha is 0.
    depth_std     sqrt(max(sum(w d d) / alpha - depth_mean^2, 0)): the spread of the depth along the ray, an uncertainty map
                  (formed in float64 from the two float32 sums, returned as float32).  0 where alpha is 0.
    dominant      index of the Gaussian with the largest w (ties: the nearer one), -1 where nothing was blended   (int32)
    count         number of Gaussians blended into the pixel                                                     (int32)

Each pixel owns its numbers: nothing is summed across pixels, the maps are the same bits whatever the batch size.

The caveat of importance.py holds here too: the entry that saturates a pixel (T (1 - alpha) < 1e-4) stops the pixel WITHOUT
being blended, so it is in none of the maps; what it could have moved is bounded by the 1e-4 of transmittance that was left.
"""
from __future__ import annotations

from typing import Iterator, Optional, Sequence, Tuple

import torch

ALL = ("median_depth", "depth_mean", "depth_std", "dominant", "count")
_PLANES = ("median_depth", "depth_m1", "depth_m2", "dominant", "count")
_NEEDS = {"median_depth": ("median_depth",), "depth_mean": ("depth_m1",), "depth_std": ("depth_m1", "depth_m2"),
          "dominant": ("dominant",), "count": ("count",)}


def plane_batches(model, cameras: Sequence, bg: torch.Tensor, planes: Sequence[str] = _PLANES, *, batch: int = 8,
                  capacity: Optional[int] = None):
    """Yields (indices into `cameras`, the renderer's per-view output dicts, per view a dict of the wanted raw planes) per
    launch.  planes: names out of median_depth, depth_m1, depth_m2 (float32 [H,W]), dominant, count (int32 [H,W]): fresh
    tensors, the caller's to keep.  The output dicts are the renderer's slot buffers: valid until the next item is drawn."""
    from . import _C
    from .evaluate import _walk_batches
    unknown = [p for p in planes if p not in _PLANES]
    if unknown:
        raise ValueError(f"planes are out of {_PLANES}, not {unknown}")
    dev = model.get_xyz.device
    P = model.get_xyz.shape[0]
    for idx, outs, W, H, slots in _walk_batches(model, cameras, bg, batch, capacity):
        views, tables, raws = [], [], []
        for s in slots:
            views.append((s.geom, s.binning, s.img, P, W, H))
            raw = {}
            for name in _PLANES:
                if name in planes:
                    dtype = torch.float32 if name in _PLANES[:3] else torch.int32
                    # (the launch writes every pixel; without Gaussians there is no launch)
                    raw[name] = torch.empty((H, W), dtype=dtype, device=dev) if P else \
                        torch.full((H, W), -1 if name == "dominant" else 0, dtype=dtype, device=dev)
            tables.append(tuple(raw.get(name) for name in _PLANES))
            raws.append(raw)
        _C.blend_pixel_maps(views, tables)
        yield idx, outs, raws


def render_maps(model, cameras: Sequence, bg: torch.Tensor, *, maps: Sequence[str] = ALL, batch: int = 8,
                capacity: Optional[int] = None) -> Iterator[Tuple[int, dict]]:
    """Yields (camera index, dict) for every camera, launch by launch (cameras of one size together, otherwise in order).  The
    dict holds the maps named in `maps` (out of ALL; [H,W] device tensors, see the module's docstring) and the forward's own
    "rendered_depth" and "rendered_alpha" ([1,H,W], cloned out of the renderer's slot buffers).  All tensors are the caller's."""
    unknown = [m for m in maps if m not in ALL]
    if unknown:
        raise ValueError(f"maps are out of {ALL}, not {unknown}")
    planes = tuple(p for p in _PLANES if any(p in _NEEDS[m] for m in maps))
    for idx, outs, raws in plane_batches(model, cameras, bg, planes, batch=batch, capacity=capacity):
        for i, o, raw in zip(idx, outs, raws):
            depth, alpha = o["rendered_depth"].detach().clone(), o["rendered_alpha"].detach().clone()
            res = {"rendered_depth": depth, "rendered_alpha": alpha}
            for m in ("median_depth", "dominant", "count"):
                if m in maps:
                    res[m] = raw[m]
            if "depth_mean" in maps or "depth_std" in maps:
                a = alpha.reshape(raw["depth_m1"].shape).double()
                seen = a > 0
                safe = torch.where(seen, a, torch.ones_like(a))
                mean = torch.where(seen, raw["depth_m1"].double() / safe, torch.zeros_like(a))
                if "depth_mean" in maps:
                    res["depth_mean"] = mean.float()
                if "depth_std" in maps:
                    var = torch.where(seen, raw["depth_m2"].double() / safe - mean * mean, torch.zeros_like(a))
                    res["depth_std"] = var.clamp_(min=0.0).sqrt_().float()
            yield i, res


FRAME_MAPS = ("median", "std", "id")
# streams of a map -> (PNG name, video name); the gray and the turbo picture of a depth-like map, as depth_ / cdepth_ are
_STREAMS = {"median": (("median_{:05d}.png", "out_median_{}.avi"), ("cmedian_{:05d}.png", "out_cmedian_{}.avi")),
            "std": (("std_{:05d}.png", "out_std_{}.avi"), ("cstd_{:05d}.png", "out_cstd_{}.avi")),
            "id": (("id_{:05d}.png", "out_id_{}.avi"),)}


def render_map_frames(model, cameras: Sequence, bg: torch.Tensor, out_dir: str, maps: Sequence[str] = FRAME_MAPS, *, video=None,
                      png: bool = True, fps: float = 25.0, quality: int = 90, percentile: float = 99.) -> dict:
    """Pictures of the maps along a camera path, next to the frames of frames.render_path: per camera median_%05d.png and
    cmedian_%05d.png (the median depth), std_%05d.png and cstd_%05d.png (depth_std) -- both through frames.encode_frames, i.e.
    the gray map 1 - (1 - normalised) * alpha and the turbo colour map with percentile bounds that depth_ and cdepth_ are
    made with -- and id_%05d.png (id_colours of the dominant Gaussian).  maps: out of "median", "std", "id".
    video = (directory, stem): the streams also become out_median_<stem>.avi, out_cmedian_, out_std_, out_cstd_, out_id_
    (Motion-JPEG, as frames.render_path writes them); png=False then skips the PNG files.
    -> {"png": paths, "video": paths}."""
    import os
    from . import frames
    unknown = [m for m in maps if m not in FRAME_MAPS]
    if unknown or not maps:
        raise ValueError(f"maps are out of {FRAME_MAPS}, not {list(maps)}")
    want = tuple(dict.fromkeys({"median": "median_depth", "std": "depth_std", "id": "dominant"}[m] for m in maps))
    if video is not None:
        sizes = {(int(c.image_width), int(c.image_height)) for c in cameras}
        if len(sizes) != 1:
            raise ValueError(f"a video holds frames of one size; the cameras have {sorted(sizes)}")
    if png:
        os.makedirs(out_dir, exist_ok=True)
    jpegs = {names: [None] * len(cameras) for m in maps for names in _STREAMS[m]}
    paths = []

    def flush(group):
        if not group:
            return
        pictures = {}
        blank = [torch.zeros((3,) + g[1]["rendered_alpha"].shape[1:], device=g[1]["rendered_alpha"].device) for g in group]
        alphas = [g[1]["rendered_alpha"] for g in group]
        for m, key in (("median", "median_depth"), ("std", "depth_std")):
            if m in maps:
                enc = frames.encode_frames(blank, [g[1][key].unsqueeze(0) for g in group], alphas, percentile=percentile)
                pictures[_STREAMS[m][0]], pictures[_STREAMS[m][1]] = enc["depth"], enc["cdepth"]
        if "id" in maps:
            pictures[_STREAMS["id"][0]] = [id_colours(g[1]["dominant"]) for g in group]
        for names, imgs in pictures.items():
            if video is not None:
                for g, data in zip(group, frames.jpeg_encode(imgs, quality)):
                    jpegs[names][g[0]] = data
            if png:
                host = torch.stack(list(imgs)).cpu()
                for j, g in enumerate(group):
                    paths.append(frames.write_png(os.path.join(out_dir, names[0].format(g[0])), host[j]))

    group = []
    for i, res in render_maps(model, cameras, bg, maps=want):
        if group and (len(group) == 8 or res["rendered_alpha"].shape != group[0][1]["rendered_alpha"].shape):
            flush(group)
            group = []
        group.append((i, res))
    flush(group)
    vids = []
    if video is not None:
        vdir, stem = os.path.split(video) if isinstance(video, str) else (video[0], video[1])
        os.makedirs(vdir or ".", exist_ok=True)
        size = next(iter(sizes))
        vids = [frames.write_avi(os.path.join(vdir, names[1].format(stem)), data, size, fps) for names, data in jpegs.items()]
    return {"png": paths, "video": vids}


def gaussians_under(dominant: torch.Tensor, region_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The sorted, unique indices of the Gaussians that `dominant` (an id map of render_maps) shows inside `region_mask`
    ([H,W], nonzero / True = inside; None: the whole image) -- int64 [n] on the device.  The inverse of importance.prune()'s
    mask: what a picked region of the image is made of."""
    ids = dominant if region_mask is None else dominant[region_mask.reshape(dominant.shape).to(dominant.device) != 0]
    ids = ids.reshape(-1)
    return torch.unique(ids[ids >= 0].to(torch.int64), sorted=True)


def id_colours(dominant: torch.Tensor) -> torch.Tensor:
    """An id map as a picture: uint8 [H,W,3] on the device, every Gaussian index hashed to a colour (a multiplicative hash of
    the index, one byte of it per channel, brightened to 64 .. 255), black where nothing was blended."""
    ids = dominant.to(torch.int64)
    h = ((ids + 1) * 2654435761) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    rgb = torch.stack([(h >> 24) & 0xFF, (h >> 12) & 0xFF, h & 0xFF], dim=-1)
    rgb = 64 + (rgb * 191) // 255
    return torch.where((ids >= 0).unsqueeze(-1), rgb, torch.zeros_like(rgb)).to(torch.uint8)
