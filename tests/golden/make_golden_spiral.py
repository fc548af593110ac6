#!/usr/bin/env python
"""G13: tests/golden/spiral.npz -- the reference's spiral path (spiral.py, scene/dataset_readers.py CreateLLFFSpiral /
CreateDTUSpiral, utils/camera_utils.py loadRenderCam), by IMPORTING its Python under the CPU shim of make_golden.py:

  cameras  CreateLLFFSpiral / CreateDTUSpiral on seeded synthetic poses_bounds.npy files (forward-facing LLFF rig; a DTU
           arc whose optical axes converge on the object), then loadRenderCam at resolutions 1, 4, 8 (and -1, width 200):
           per frame R, T, FoVx, FoVy (identical across resolutions: checked), width and height per resolution
  frames   spiral.render_set with a stand-in render() returning seeded rgb / depth / alpha, a stand-in save_image that
           applies torchvision's quantiser uint8(clamp(x*255 + 0.5, 0, 255)) (make_grid: 1 channel -> 3) and records the
           bytes, os.system a no-op (no ffmpeg); spiral.weighted_percentile and the colormap are wrapped to record lo_auto /
           hi_auto and the fp64 value handed to the map.  Views: several sizes (one with 0.005 n < 1, some with an integer
           0.005 n), alpha = 0 regions, heavy ties, one empty view (constant depth)
  turbo    uint8(clamp(turbo._lut[:256, :3]*255 + 0.5, 0, 255)) in fp64, from matplotlib

Only data leaves this script.  Re-run with:  python tests/golden/make_golden_spiral.py"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, CudaToCpu, install_shim  # noqa: E402

RESOLUTIONS = (1, 4, 8, -1, 200)
# (H, W, kind): kind picks the depth / alpha pattern
VIEWS = ((24, 32, "background"), (10, 12, "random"), (40, 50, "random"), (48, 64, "ties"), (16, 20, "empty"),
         (36, 45, "smooth"), (30, 40, "ties"), (20, 40, "background"))


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (0, 2), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def llff_poses(rng):
    rows = []
    for k in range(9):
        R = _rot(0, rng.uniform(-0.08, 0.08)) @ _rot(1, rng.uniform(-0.08, 0.08)) @ _rot(2, rng.uniform(-0.03, 0.03))
        t = np.array([0.3 * (k % 3 - 1), 0.25 * (k // 3 - 1), 0.0]) + rng.normal(0, 0.03, 3)
        blk = np.concatenate([R, t[:, None], np.array([[378.0], [504.0], [407.56]])], 1)
        rows.append(np.concatenate([blk.ravel(), [rng.uniform(1.5, 2.5), rng.uniform(20.0, 40.0)]]))
    return np.array(rows)


def dtu_poses(rng):
    rows = []
    centre = np.array([0.1, -0.2, 0.05])
    for k in range(7):
        az, el = -0.6 + 0.2 * k + rng.normal(0, 0.02), 0.35 + rng.normal(0, 0.05)
        p = centre + 3.0 * np.array([np.cos(el) * np.sin(az), np.sin(el), np.cos(el) * np.cos(az)])
        z = (p - centre) / np.linalg.norm(p - centre)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        blk = np.concatenate([np.stack([x, y, z], 1), p[:, None], np.array([[300.0], [400.0], [350.3]])], 1)
        rows.append(np.concatenate([blk.ravel(), [2.0, 4.5]]))
    return np.array(rows)


def view_inputs(g, H, W, kind):
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    rgb = 1.3 * r(3, H, W) - 0.15
    if kind == "empty":
        return rgb, torch.zeros(1, H, W), torch.zeros(1, H, W)
    if kind == "ties":
        depth = torch.randint(0, 4, (1, H, W), generator=g).float() * 0.75 + 1.0
        alpha = torch.randint(0, 3, (1, H, W), generator=g).float() * 0.5
    elif kind == "smooth":
        yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        depth = (2.0 + torch.sin(3 * xx) * torch.cos(2 * yy))[None] * (0.9 + 0.2 * r(1, H, W))
        alpha = torch.clamp(1.2 * r(1, H, W) - 0.1, 0, 1)
    else:
        depth = 0.5 + 6.0 * r(1, H, W)
        alpha = r(1, H, W)
    if kind != "random":
        alpha[:, : H // 4, : W // 3] = 0.0      # background: v = 1 exactly (above the upper percentile)
    return rgb, depth, alpha


def main():
    install_shim({})
    torch.nn.Module.cuda = lambda self, *a, **k: self
    saved = []

    def save_image(tensor, fp, **kw):
        t = tensor.detach()
        if t.dim() == 3 and t.size(0) == 1:
            t = torch.cat((t, t, t), 0)
        nd = t.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)
        saved.append((os.path.basename(fp), nd.numpy().copy()))

    tv = types.ModuleType("torchvision")
    tv.utils = types.ModuleType("torchvision.utils")
    tv.utils.save_image = save_image
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.utils"] = tv.utils
    out = {"numpy_version": np.array(np.__version__)}
    rng = np.random.default_rng(131313)
    g = torch.Generator().manual_seed(1313)
    with CudaToCpu():
        import spiral
        from matplotlib import colormaps
        from scene.dataset_readers import CreateDTUSpiral, CreateLLFFSpiral
        from utils.camera_utils import loadRenderCam

        # ---- cameras ----
        with tempfile.TemporaryDirectory() as tmp:
            for name, maker, create in (("llff", llff_poses, CreateLLFFSpiral), ("dtu", dtu_poses, CreateDTUSpiral)):
                pb = maker(rng)
                np.save(os.path.join(tmp, "poses_bounds.npy"), pb)
                infos = create(tmp).test_cameras
                out[f"{name}_poses_bounds"] = pb
                first = None
                for res in RESOLUTIONS:
                    args = types.SimpleNamespace(resolution=res, data_device="cpu")
                    cams = [loadRenderCam(args, i, c, 1.0) for i, c in enumerate(infos)]
                    vals = (np.stack([c.R for c in cams]), np.stack([c.T for c in cams]),
                            np.array([c.FoVx for c in cams]), np.array([c.FoVy for c in cams]))
                    if first is None:
                        first = vals
                    assert all(np.array_equal(a, b) for a, b in zip(first, vals))
                    out[f"{name}_size_r{res}"] = np.array([[c.image_width, c.image_height] for c in cams], dtype=np.int64)
                for k, v in zip(("R", "T", "FovX", "FovY"), first):
                    out[f"{name}_{k}"] = v
                out[f"{name}_orig_wh"] = np.array([infos[0].width, infos[0].height], dtype=np.float64)
        out["resolutions"] = np.array(RESOLUTIONS)

        # ---- frames ----
        pkgs = []
        for H, W, kind in VIEWS:
            rgb, depth, alpha = view_inputs(g, H, W, kind)
            pkgs.append({"render": rgb, "rendered_depth": depth, "rendered_alpha": alpha})
        bounds, values = [], []
        real_wp = spiral.weighted_percentile

        def weighted_percentile(x, w, ps, assume_sorted=False):
            r = real_wp(x, w, ps, assume_sorted)
            bounds.append(np.array(r, dtype=np.float64))
            return r

        class Recorded:
            def __init__(self, cmap):
                self.cmap = cmap

            def __call__(self, x, *a, **k):
                values.append(np.array(x, dtype=np.float64, copy=True))
                return self.cmap(x, *a, **k)

        real_cmaps = spiral.colormaps
        spiral.weighted_percentile = weighted_percentile
        spiral.colormaps = types.SimpleNamespace(get_cmap=lambda n: Recorded(real_cmaps.get_cmap(n)))
        spiral.render = lambda view, gaussians, pipeline, background: pkgs[view.uid]
        spiral.os.system = lambda cmd: 0
        with tempfile.TemporaryDirectory() as tmp:
            args = types.SimpleNamespace(model_path=tmp, source_path=os.path.join(tmp, "scene"))
            views = [types.SimpleNamespace(uid=i) for i in range(len(VIEWS))]
            spiral.render_set(args, "render", 7, views, None, None, torch.zeros(3), 0)
        assert len(saved) == 3 * len(VIEWS) and len(bounds) == len(VIEWS) and len(values) == len(VIEWS)
        for i, (H, W, kind) in enumerate(VIEWS):
            names = [s[0] for s in saved[3 * i:3 * i + 3]]
            assert names == [f"{i:05d}.png", f"depth_{i:05d}.png", f"cdepth_{i:05d}.png"], names
            out[f"f{i}_kind"] = np.array(kind)
            for k in ("render", "rendered_depth", "rendered_alpha"):
                out[f"f{i}_{k}"] = pkgs[i][k].numpy()
            out[f"f{i}_rgb"], out[f"f{i}_gray"], out[f"f{i}_cdepth"] = (s[1] for s in saved[3 * i:3 * i + 3])
            out[f"f{i}_bounds"] = bounds[i]
            out[f"f{i}_value"] = values[i]
        out["n_frames_views"] = np.array(len(VIEWS))

        cm = colormaps.get_cmap("turbo")
        cm._init()
        out["turbo_u8"] = np.clip(cm._lut[:256, :3] * 255 + 0.5, 0, 255).astype(np.uint8)
    np.savez_compressed(os.path.join(OUT, "spiral.npz"), **out)
    print("wrote", os.path.join(OUT, "spiral.npz"), os.path.getsize(os.path.join(OUT, "spiral.npz")), "bytes")


if __name__ == "__main__":
    main()
