"""binocular3dgs_amd.pixel_maps on the device: render_maps() whatever the batch, its maps against the forward's own images,
gaussians_under(), and the opt-in median depth of mesh.fuse_model against a manual TsdfVolume.integrate -- with the default
still the mean depth, bit for bit."""
import numpy as np
import pytest
import torch

import helpers
import pixelmaps_ref

pytestmark = pytest.mark.gpu
W, H = 64, 48


@pytest.fixture(scope="module")
def scene():
    from binocular3dgs_amd import pixel_maps, synth
    model = synth.synth_model(600, seed=4, device="cuda", width=W, height=H, requires_grad=False, scale_mult=6.0)
    cams = synth.synth_cameras(W, H, yaws=(0.0, 7.0, -6.0), device="cuda")
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    maps = dict(pixel_maps.render_maps(model, cams, bg, batch=8))
    return model, cams, bg, maps


def _two_layer_model(front_opacity=0.3):
    """pixelmaps_ref.two_layer_scene as a GaussianModel and its camera."""
    from binocular3dgs_amd import synth
    from binocular3dgs_amd.camera import Camera, look_at_orbit
    from binocular3dgs_amd.gaussian_model import GaussianModel
    d = pixelmaps_ref.two_layer_scene(front_opacity)
    n = d["means3D"].shape[0]
    op = d["opacities"].double().reshape(-1, 1)
    model = GaussianModel.from_tensors(d["means3D"].float(), d["shs"][:, :1].float(), torch.zeros(n, 3, 3),
                                       torch.log(d["scales"].double()).float(), d["rotations"].float(), torch.log(op / (1 - op)).float(),
                                       sh_degree=1, active_sh_degree=1, device="cuda", requires_grad=False)
    cam = Camera(*look_at_orbit(0.0), helpers.BLEND_FOVX, synth.fovy_from(helpers.BLEND_FOVX, d["W"], d["H"]), d["W"], d["H"], device="cuda")
    return model, [cam], d["bg"].float().cuda()


def test_render_maps_is_the_same_bits_whatever_the_batch(scene):
    from binocular3dgs_amd import pixel_maps
    model, cams, bg, maps = scene
    assert sorted(maps) == [0, 1, 2]
    keys = set(pixel_maps.ALL) | {"rendered_depth", "rendered_alpha"}
    for i in range(3):
        m = maps[i]
        assert set(m) == keys
        assert all(m[k].shape == (H, W) for k in pixel_maps.ALL) and m["rendered_depth"].shape == (1, H, W)
        assert m["median_depth"].dtype == m["depth_mean"].dtype == m["depth_std"].dtype == torch.float32
        assert m["dominant"].dtype == m["count"].dtype == torch.int32
        assert int((m["count"] > 0).sum()) > H * W // 10 and int(m["count"].max()) > 1
    one = dict(pixel_maps.render_maps(model, cams, bg, batch=1))
    for i in range(3):
        for k in keys:
            assert torch.equal(one[i][k], maps[i][k]), (i, k)
    only = dict(pixel_maps.render_maps(model, cams[1:2], bg, maps=("median_depth",)))
    assert set(only[0]) == {"median_depth", "rendered_depth", "rendered_alpha"} and torch.equal(only[0]["median_depth"], maps[1]["median_depth"])
    with pytest.raises(ValueError):
        next(pixel_maps.render_maps(model, cams, bg, maps=("normal",)))


def test_maps_agree_with_the_forward_and_with_each_other(scene):
    model, cams, bg, maps = scene
    P = model.get_xyz.shape[0]
    for i in range(3):
        m = maps[i]
        depth, alpha = m["rendered_depth"][0].double(), m["rendered_alpha"][0].double()
        seen = m["count"] > 0
        assert torch.equal(seen, alpha > 0) and torch.equal(seen, m["dominant"] >= 0) and torch.equal(seen, m["median_depth"] != 0)
        assert int(m["dominant"].max()) < P and int(m["dominant"].min()) >= -1
        # depth_mean * alpha is the forward's depth image: within the float32 noise bound of the sum (10 x the reference's
        # noise, tests/test_pixelmaps_ref_cpu.py) plus the roundings of the division and the product back
        err = (m["depth_mean"].double() * alpha - depth).abs()
        assert bool((err <= (pixelmaps_ref.M1_BOUND + 3 * 2.0 ** -24) * depth.abs()).all()), float((err / depth.abs().clamp(min=1e-30)).max())
        assert not bool(m["depth_mean"][~seen].any()) and not bool(m["depth_std"][~seen].any())
        assert bool((m["depth_std"] >= 0).all()) and bool(torch.isfinite(m["depth_std"]).all()) and float(m["depth_std"].max()) > 0
        # the median and the mean are depths of the pixel's own Gaussians: between the nearest and the farthest centre
        z = (model.get_xyz @ cams[i].world_view_transform[:3, 2] + cams[i].world_view_transform[3, 2])
        lo, hi = float(z[z > 0.2].min()), float(z.max())
        for k in ("median_depth", "depth_mean"):
            assert bool((m[k][seen] >= lo * (1 - 1e-5)).all()) and bool((m[k][seen] <= hi * (1 + 1e-5)).all()), k
        # one blended Gaussian: all three depths are its depth
        single = m["count"] == 1
        if bool(single.any()):
            assert bool(((m["depth_mean"][single] - m["median_depth"][single]).abs() <= 4e-7 * m["median_depth"][single]).all())


def test_gaussians_under_a_region(scene):
    from binocular3dgs_amd import pixel_maps
    _model, _cams, _bg, maps = scene
    dom = maps[0]["dominant"]
    want = torch.unique(dom[dom >= 0]).to(torch.int64)
    got = pixel_maps.gaussians_under(dom)
    assert got.dtype == torch.int64 and torch.equal(got, want) and bool((got[1:] > got[:-1]).all()) and got.numel() > 10
    region = torch.zeros(H, W, dtype=torch.bool, device="cuda")
    region[10:20, 30:40] = True
    part = pixel_maps.gaussians_under(dom, region)
    sub = dom[10:20, 30:40]
    assert torch.equal(part, torch.unique(sub[sub >= 0]).to(torch.int64)) and 0 < part.numel() < got.numel()
    assert pixel_maps.gaussians_under(dom, torch.zeros(H, W, device="cuda")).numel() == 0
    col = pixel_maps.id_colours(dom)
    assert col.shape == (H, W, 3) and col.dtype == torch.uint8
    assert not bool(col[dom < 0].any()) and bool((col[dom >= 0] >= 64).all())


def _manual_volume(model, cams, bg, lo, hi, voxel, which):
    from binocular3dgs_amd import evaluate, mesh, pixel_maps
    maps = dict(pixel_maps.render_maps(model, cams, bg, maps=("median_depth",)))
    colours = evaluate.render_views(model, cams, bg)
    vol = mesh.TsdfVolume(lo, hi, voxel, 4.0 * voxel, device="cuda")
    alphas = [maps[i]["rendered_alpha"] for i in range(len(cams))]
    if which == "median":
        depths = [maps[i]["median_depth"] * maps[i]["rendered_alpha"][0] for i in range(len(cams))]
    else:
        depths = [maps[i]["rendered_depth"] for i in range(len(cams))]
    vol.integrate(cams, depths, alphas, colours)
    return vol


def _same(a, b):
    return torch.equal(a.tsdf, b.tsdf) and torch.equal(a.weight, b.weight) and torch.equal(a.rgb, b.rgb)


def test_fuse_model_median_is_a_manual_integrate_of_the_median_and_the_default_stays_the_mean(scene):
    from binocular3dgs_amd import mesh
    model, cams, bg, _maps = scene
    lo, hi = mesh.scene_bounds(model, 0.02)
    voxel = max(h - l for l, h in zip(lo, hi)) / 40
    kw = dict(voxel_size=voxel, bounds=(lo, hi), return_volume=True)
    *_, vol_default = mesh.fuse_model(model, cams, bg, **kw)
    *_, vol_mean = mesh.fuse_model(model, cams, bg, depth="mean", **kw)
    v, c, f, vol_median = mesh.fuse_model(model, cams, bg, depth="median", **kw)
    assert float(vol_default.weight.sum()) > 0 and f.shape[0] > 0
    assert _same(vol_default, _manual_volume(model, cams, bg, lo, hi, voxel, "mean")), "the default is the parent's mean-depth fusion"
    assert _same(vol_default, vol_mean)
    assert _same(vol_median, _manual_volume(model, cams, bg, lo, hi, voxel, "median"))
    with pytest.raises(ValueError):
        mesh.fuse_model(model, cams, bg, depth="mode", **kw)


def test_median_and_mean_fusion_differ_on_two_layers():
    from binocular3dgs_amd import mesh, pixel_maps
    model, cams, bg = _two_layer_model(0.3)
    d1, d2 = pixelmaps_ref.TWO_LAYER_D1, pixelmaps_ref.TWO_LAYER_D2
    (_, m), = pixel_maps.render_maps(model, cams, bg)
    covered = m["rendered_alpha"][0] > 0.95
    assert float(covered.float().mean()) > 0.9
    assert bool((m["median_depth"][covered] >= d2).all()) and bool((m["median_depth"][covered] <= d2 + 0.31).all())
    assert bool((m["depth_mean"][covered] > d1 + 0.5).all()) and bool((m["depth_mean"][covered] < m["median_depth"][covered] - 0.2).all())
    assert bool((m["depth_std"][covered] > 0.5).all())
    kw = dict(voxel_size=0.1, bounds=([-2.5, -2.5, 1.0], [2.5, 2.5, 5.5]), return_volume=True)
    vm, _, fm, vol_mean = mesh.fuse_model(model, cams, bg, **kw)
    vd, _, fd, vol_median = mesh.fuse_model(model, cams, bg, depth="median", **kw)
    assert not torch.equal(vol_mean.tsdf, vol_median.tsdf)
    assert fm.shape[0] > 0 and fd.shape[0] > 0
    # the mean-depth surface floats between the sheets; the median-depth surface lies on the back sheet
    zc = float(np.median(vm[:, 2].cpu().numpy())), float(np.median(vd[:, 2].cpu().numpy()))
    assert d1 + 0.5 < zc[0] < d2 - 0.3 and d2 - 0.15 < zc[1] < d2 + 0.45, zc
    # ... and agrees with the model's median depth, not with its mean depth (mesh_render.depth_agreement takes the same choice)
    from binocular3dgs_amd import mesh_render
    with_median = mesh_render.depth_agreement(model, vd, fd, cams, bg, depth="median")
    with_mean = mesh_render.depth_agreement(model, vd, fd, cams, bg)
    assert with_median["model_depth"] == "median" and "model_depth" not in with_mean and with_median["pixels"] == with_mean["pixels"] > 500
    assert with_median["median"] < 0.1 < 0.3 < with_mean["median"], (with_median, with_mean)
    with pytest.raises(ValueError):
        mesh_render.depth_agreement(model, vd, fd, cams, bg, depth="mode")


def test_spiral_maps_write_their_frames_and_videos(tmp_path, capsys):
    import os
    from binocular3dgs_amd import frames, pixel_maps, spiral, synth
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "scene_llff")
    model = synth.synth_model(5000, seed=1, device="cuda", width=64, height=48)
    ply = tmp_path / "m" / "point_cloud" / "iteration_7" / "point_cloud.ply"
    os.makedirs(ply.parent)
    model.save_ply(str(ply))
    assert spiral.main(["-m", str(tmp_path / "m"), "-s", src, "-r", "8", "--frames", "9", "--maps", "median,std,id"]) == 0
    assert "maps (median, std, id): 45 PNG files" in capsys.readouterr().out
    out = tmp_path / "m" / "render" / "ours_7"
    names = sorted(os.listdir(out))
    assert len(names) == 9 * (3 + 5)
    for stem in ("median", "cmedian", "std", "cstd", "id"):
        assert [n for n in names if n.startswith(stem + "_")] == [f"{stem}_{i:05d}.png" for i in range(9)]
    # the id picture is id_colours of the frame's dominant map; the median pictures are the depth encoder's of the median
    from binocular3dgs_amd import camera_path
    from binocular3dgs_amd.gaussian_model import GaussianModel
    loaded = GaussianModel(1)
    loaded.load_ply(str(ply))
    cams = camera_path.spiral_cameras_from_dir(src, n_frames=9, resolution=8, device="cuda")
    bg = torch.zeros(3, device="cuda")
    maps = dict(pixel_maps.render_maps(loaded, cams, bg))
    m = maps[8]
    assert open(out / "id_00008.png", "rb").read() == frames.png_bytes(pixel_maps.id_colours(m["dominant"]).cpu())
    enc = frames.encode_frames([torch.zeros(3, *m["median_depth"].shape, device="cuda")], [m["median_depth"][None]], [m["rendered_alpha"]])
    assert open(out / "median_00008.png", "rb").read() == frames.png_bytes(enc["depth"][0].cpu())
    assert open(out / "cmedian_00008.png", "rb").read() == frames.png_bytes(enc["cdepth"][0].cpu())
    assert len({open(out / f"id_{i:05d}.png", "rb").read() for i in range(9)}) > 1
    # videos follow --video; --maps does not go with --mesh
    assert spiral.main(["-m", str(tmp_path / "m"), "-s", src, "-r", "8", "--frames", "9", "--video", "--no_png", "--maps", "std,id"]) == 0
    avis = sorted(n for n in os.listdir(tmp_path / "m") if n.endswith(".avi"))
    assert avis == sorted(["out_scene_llff.avi", "out_depth_scene_llff.avi", "out_cdepth_scene_llff.avi", "out_std_scene_llff.avi",
                           "out_cstd_scene_llff.avi", "out_id_scene_llff.avi"])
    assert len(frames.avi_frames(str(tmp_path / "m" / "out_id_scene_llff.avi"))[3]) == 9
    with pytest.raises(SystemExit):
        spiral.main(["-m", str(tmp_path / "m"), "-s", src, "--maps", "median", "--mesh", "x.ply"])
    with pytest.raises(SystemExit):
        spiral.main(["-m", str(tmp_path / "m"), "-s", src, "--maps", "normal"])
