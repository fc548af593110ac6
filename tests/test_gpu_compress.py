"""GPU: binocular3dgs_amd.compress on a synthetic model of 4000 Gaussians at 160 x 120 with two cameras.

With as many codes as Gaussians every row is its own code: the decompressed colour tensors equal the original's bit for bit, and
the render equals the render of the original model as the file holds it -- the rotations canonicalised (compress.canonical_rotation)
and the opacity logit rounded to the float16 it is stored as -- bit for bit.  With 256 codes: the file round trip, a finite
render, the byte count, and what the contribution weights do to the codebook.  No PSNR threshold: what 256 codes cost on the
synthetic scene has not been measured."""
from dataclasses import fields

import numpy as np
import pytest
import torch

import kmeans_ref as ref
from binocular3dgs_amd import compress

pytestmark = pytest.mark.gpu
P, W, H = 4000, 160, 120


@pytest.fixture(scope="module")
def scene():
    from binocular3dgs_amd import importance, synth
    model = synth.synth_model(P, seed=3, device="cuda", width=W, height=H, requires_grad=False)
    cams = synth.synth_cameras(W, H, yaws=(0.0, 9.0), device="cuda")
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    return model, cams, bg, importance.contributions(model, cams, bg).weight


def renders(m, cams, bg):
    from binocular3dgs_amd import evaluate
    out = {}
    for idx, outs in evaluate._batches(m, cams, bg, 8, None, full=True):
        for i, o in zip(idx, outs):
            out[i] = tuple(o[k].clone() for k in ("render", "rendered_depth", "rendered_alpha"))
    return out


def test_one_code_per_gaussian_is_lossless(scene):
    from binocular3dgs_amd.gaussian_model import GaussianModel
    model, cams, bg, _w = scene
    cm = compress.compress(model, None, colour_codes=P, shape_codes=P, iters=2)
    assert cm.colour_codebook.shape == (P, 12) and cm.shape_codebook.shape == (P, 7)
    assert cm.colour_index.dtype == np.uint16 and cm.opacity.dtype == np.float16 and cm.xyz.dtype == np.float32
    assert np.array_equal(cm.colour_index, np.arange(P)) and np.array_equal(cm.shape_index, np.arange(P))
    assert np.array_equal(cm.colour_distortion, np.zeros(3)) and np.array_equal(cm.shape_distortion, np.zeros(3))
    back = compress.decompress(cm)
    assert back.max_sh_degree == model.max_sh_degree and back.active_sh_degree == model.active_sh_degree
    assert torch.equal(back._features_dc, model._features_dc) and torch.equal(back._features_rest, model._features_rest)
    assert torch.equal(back._xyz, model._xyz) and torch.equal(back._scaling, model._scaling)
    stored = GaussianModel.from_tensors(model._xyz, model._features_dc, model._features_rest, model._scaling,
                                        compress.canonical_rotation(model._rotation), model._opacity.half().float(),
                                        sh_degree=model.max_sh_degree, active_sh_degree=model.active_sh_degree, device="cuda",
                                        requires_grad=False)
    assert torch.equal(back._rotation, stored._rotation) and torch.equal(back._opacity, stored._opacity)
    a, b = renders(stored, cams, bg), renders(back, cams, bg)
    for i in range(len(cams)):
        assert a[i][2].max() > 0.05
        for x, y, k in zip(a[i], b[i], ("colour", "depth", "alpha")):
            assert torch.equal(x, y), (i, k)


def test_256_codes(scene, tmp_path):
    model, cams, bg, weight = scene
    assert int((weight > 0).sum()) > 256 and int((weight == 0).sum()) > 0
    cm = compress.compress(model, weight, colour_codes=256, shape_codes=256, iters=4)
    path = str(tmp_path / "model.npz")
    compress.save_compressed(path, cm)
    back = compress.load_compressed(path)
    for f in fields(cm):
        a, b = getattr(cm, f.name), getattr(back, f.name)
        assert (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()) if isinstance(a, np.ndarray) else a == b, f.name
    with np.load(path) as z:
        assert compress.compressed_bytes(cm) == sum(z[k].nbytes for k in compress._PAYLOAD)
    assert compress.compressed_bytes(cm) == P * (12 + 2 + 2 + 2) + 256 * (12 + 7) * 4
    assert compress.model_bytes(model) == 92 * P
    small = compress.decompress(back)
    assert small.get_xyz.shape[0] == P
    for i, outs in renders(small, cams, bg).items():
        assert all(bool(torch.isfinite(o).all()) for o in outs) and outs[2].max() > 0.05, i

    # the contribution weights move the codebook, and serve their own measure no worse than uniform weights do
    colour, _shape = compress.group_rows(model)
    cw, _codes, _counts, dw = compress.kmeans(colour, 256, weight, iters=4)
    cu, _codes, _counts, _du = compress.kmeans(colour, 256, None, iters=4)
    assert np.array_equal(cw.cpu().numpy(), cm.colour_codebook) and not torch.equal(cw, cu)
    du_under_w = float(compress.kmeans(colour, 256, weight, iters=0, init=cu)[3][0])
    bound = ref.step_bound(colour.cpu().numpy(), cw.cpu().numpy(), weight.cpu().numpy())
    print(f"weighted distortion: weighted codebook {float(dw[-1])}, uniform codebook {du_under_w}, bound {bound}")
    assert float(dw[-1]) <= du_under_w + bound
    assert all(float(dw[i + 1]) <= float(dw[i]) + bound for i in range(4))


def test_command_line_writes_a_compressed_iteration(tmp_path, capsys):
    import json
    import os
    import shutil
    from binocular3dgs_amd import spiral
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.init_points import load_ply
    from binocular3dgs_amd.scene import Scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = shutil.copytree(os.path.join(root, "tests", "golden", "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "model"
    np.random.seed(0)
    model = GaussianModel(1)
    scene = Scene.from_dataset(str(src), model, eval=True, n_views=3, dataset_name="LLFF", resolution=1, init_points="sparse",
                               model_path=str(out), shuffle=False)
    scene.save(7)
    n = model.get_xyz.shape[0]
    with open(out / "cfg_args", "w") as fp:
        fp.write(f"Namespace(source_path={str(src)!r}, images='images', eval=True, n_views=3, dataset_name='LLFF', resolution=1, "
                 "white_background=False, sh_degree=1, init_points='sparse')")
    assert compress.main(["-m", str(out), "--views", "all", "--colour_codes", "64", "--shape_codes", "32", "--iters", "3",
                          "--evaluate", "--decompress"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["P"] == n and res["bytes_before"] == 92 * n and res["bytes_after"] < res["bytes_before"]
    assert abs(res["ratio"] - res["bytes_before"] / res["bytes_after"]) < 1e-12
    assert len(res["colour_distortion"]) == 4 and len(res["shape_distortion"]) == 4
    for tag in ("before", "after"):
        assert set(res[tag]) == {"PSNR", "SSIM", "L1"} and all(np.isfinite(v) for v in res[tag].values())
    folder = out / "point_cloud" / "iteration_7_compressed"
    assert res["npz"] == str(folder / "model.npz") and compress.load_compressed(res["npz"]).xyz.shape == (n, 3)
    assert res["ply"] == str(folder / "point_cloud.ply") and load_ply(res["ply"], 1).get_xyz.shape[0] == n
    assert spiral.max_iteration(str(out)) == 7      # the compressed folder is not taken for a later iteration
    assert compress.main(["-m", str(out), "--uniform", "--colour_codes", "16", "--shape_codes", "16", "--iters", "1"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["weights"] == "uniform" and "ply" not in res and res["colour_codes"] == min(16, n)
