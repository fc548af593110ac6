"""GPU: LPIPS (VGG) on the device (binocular3dgs_amd/lpips.py, csrc/lpips.hip) against the float64 yardstick tests/lpips_ref.py.

Image sizes: 37x45 gives layers of 37x45, 18x22, 9x11, 4x5 and 2x2 -- an odd row or column is dropped at three pools, nothing is
a multiple of a tile, and the first layers span more than one workgroup; 16x16 is the smallest size the network accepts.

  1. features bit for bit with integer weights (every value an exactly representable integer): lane maps, k order, border
     padding, the pool's floor, the channel order;
  2. the zero padding comes after the z-score;
  3. the per-layer terms against float64, within 8 d32, d32 = the deviation of the SAME yardstick run in float32 (measured in the
     test): the device sums K in one ordered fmaf chain, the CPU blocks its sums, so two independent rounding patterns add;
  4. the same bits from call to call, alone or at any position of a batch, and with a workspace limit that forces single pairs;
  5. argument errors at the C ABI;
  6. evaluate_views(lpips_weights=...) and the command line."""
import ctypes as C
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

import lpips_ref
from binocular3dgs_amd import lpips

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 45), (16, 16)]
FACTOR = 8.0


def integer_weights(seed):
    """Every output channel: exactly 3 non-zero taps at random positions of its 9 Cin, +1 with probability 0.7, else -1; biases
    in {-1, 0, 1}; lin uniform; shift 0, scale 1."""
    gen = torch.Generator().manual_seed(seed)
    cw, cb = [], []
    for cin, cout in zip(lpips.CONV_CIN, lpips.CONV_COUT):
        w = torch.zeros(cout, 9 * cin)
        for o in range(cout):
            pos = torch.randperm(9 * cin, generator=gen)[:3]
            w[o, pos] = torch.where(torch.rand(3, generator=gen) < 0.7, 1.0, -1.0)
        cw.append(w.reshape(cout, cin, 3, 3))
        cb.append(torch.randint(-1, 2, (cout,), generator=gen).float())
    lin = [torch.rand(c, generator=gen) for c in lpips.TAP_C]
    return lpips.LpipsWeights(cw, cb, lin, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


@functools.lru_cache(maxsize=None)
def _integer_case(size):
    H, W = size
    w = integer_weights(5)
    x = torch.randint(0, 4, (3, 3, H, W), generator=torch.Generator().manual_seed(H)).float()
    return w, x, lpips_ref.features(x, w), lpips_ref.features(x, w, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _value_case(size, normalize):
    """8 pairs: x uniform, y = clamp(x + 0.1 noise); the float64 terms and the float32 ones, computed once."""
    H, W = size
    gen = torch.Generator().manual_seed(100 + H)
    x = torch.rand(8, 3, H, W, generator=gen)
    y = (x + 0.1 * torch.randn(8, 3, H, W, generator=gen)).clamp(0, 1)
    w = lpips.random_weights(0)
    return w, x, y, lpips_ref.lpips_layers(x, y, w, normalize), lpips_ref.lpips_layers(x, y, w, normalize, dtype=torch.float32).double()


def _rel(a, ref):
    return float(((a - ref).abs() / ref.abs()).max())


@pytest.mark.parametrize("size", SIZES)
def test_features_are_exact_with_integer_weights(size):
    w, x, ref, ref32 = _integer_case(size)
    H, W = size
    got = lpips.features(x.cuda(), w)
    assert [tuple(f.shape) for f in got] == [(3, c, H >> l, W >> l) for l, c in enumerate(lpips.TAP_C)]
    for l in range(5):
        r = ref[l]
        # the premise: integers far below 2^24, float32 torch equal to float64, a good part of every tap non-zero
        assert torch.equal(r, r.round()) and float(r.max()) < 2 ** 20 and torch.equal(ref32[l].double(), r)
        assert float((r != 0).double().mean()) > 0.2, l
        g = got[l].cpu()
        assert g.dtype == torch.float32
        bad = (g.double() != r)
        assert not bool(bad.any()), f"tap {l}: {int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[0].tolist()}"


def test_padding_is_zero_after_the_zscore():
    w = lpips.random_weights(0)
    H, W = 16, 16
    x = torch.full((1, 3, H, W), 0.5)
    ref = lpips_ref.features(x, w)[0]
    ref32 = lpips_ref.features(x, w, dtype=torch.float32)[0].double()
    got = lpips.features(x.cuda(), w)[0].cpu().double()
    # the constant image is constant two pixels inside the border only: x^(0.5) != 0 meets zero padding
    assert not torch.equal(got[0, :, 0, 0], got[0, :, 8, 8]) and not torch.equal(got[0, :, 8, 0], got[0, :, 8, 8])
    assert torch.equal(got[0, :, 5, 6], got[0, :, 8, 8])
    scale = float(ref.abs().max())
    d32 = float((ref32 - ref).abs().max()) / scale
    dev = float((got - ref).abs().max()) / scale
    print(f"relu1_2 of a constant image: d32 = {d32:.3e}, device = {dev:.3e}")
    assert 0 < d32 < 1e-5 and dev <= FACTOR * d32
    # had the padding been x^(0) (the z-score of a zero border) the corner would be off by far more than that
    assert float((ref[0, :, 0, 0] - ref[0, :, 8, 8]).abs().max()) / scale > 1e-2


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("npairs", [3, 8])
@pytest.mark.parametrize("size", SIZES)
def test_layer_terms_match_the_float64_yardstick(size, npairs, normalize):
    w, x, y, ref, ref32 = _value_case(size, normalize)
    x, y, ref, ref32 = x[:npairs], y[:npairs], ref[:npairs], ref32[:npairs]
    got = lpips.lpips_layers(x.cuda(), y.cuda(), w, normalize=normalize)
    assert got.dtype == torch.float64 and got.shape == (npairs, 5) and got.is_cuda
    total = lpips.lpips(x.cuda(), y.cuda(), w, normalize=normalize)
    assert torch.equal(total, got.sum(1)) and total.shape == (npairs,)
    got = got.cpu()
    assert bool((ref > 0).all())
    d32, dev = _rel(ref32, ref), _rel(got, ref)
    print(f"{size[0]}x{size[1]} n={npairs} normalize={normalize}: d32 = {d32:.3e}, device = {dev:.3e}, bound = {FACTOR * d32:.3e}")
    assert 0 < d32 < 1e-4
    assert dev <= FACTOR * d32


def test_determinism_and_batching():
    w, x, y, _, _ = _value_case((37, 45), False)
    x, y = x.cuda(), y.cuda()
    a = lpips.lpips_layers(x, y, w)
    b = lpips.lpips_layers(x, y, w)
    assert torch.equal(a, b)
    # every pair alone = its row of the batch
    for j in range(8):
        assert torch.equal(lpips.lpips_layers(x[j:j + 1], y[j:j + 1], w)[0], a[j]), j
    # pair 0 at every position of a batch of 8, among other pairs
    for j in range(1, 8):
        perm = list(range(8))
        perm[0], perm[j] = perm[j], perm[0]
        assert torch.equal(lpips.lpips_layers(x[perm], y[perm], w)[j], a[0]), j
    # a workspace limit that forces single pairs; 11 pairs cross the 8-pair cut
    assert torch.equal(lpips.lpips_layers(x, y, w, max_workspace_bytes=1), a)
    x11, y11 = torch.cat([x, x[:3]]), torch.cat([y, y[:3]])
    assert torch.equal(lpips.lpips_layers(x11, y11, w), torch.cat([a, a[:3]]))
    assert torch.equal(lpips.lpips(list(x[:2]), list(y[:2]), w), a[:2].sum(1))
    # identical images: exactly 0
    z = lpips.lpips(x, x.clone(), w)
    assert torch.equal(z, torch.zeros(8, dtype=torch.float64, device="cuda"))
    f8, f1 = lpips.features(x, w), lpips.features(x[5:6], w)
    assert all(torch.equal(p[5:6], q) for p, q in zip(f8, f1))


def test_argument_errors_at_the_c_abi():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    w = lpips.random_weights(0).to("cuda")
    cw, cb, lin = w.packed
    tab = _lib.B3gsLpipsWeights()
    for i in range(13):
        tab.conv_w[i], tab.conv_b[i] = cw[i].data_ptr(), cb[i].data_ptr()
    for l in range(5):
        tab.lin[l] = lin[l].data_ptr()
    for c in range(3):
        tab.shift[c], tab.scale[c] = w.shift[c], w.scale[c]
    x = torch.rand(9, 3, 16, 16, device="cuda")
    out = torch.full((9, 5), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.empty(L.b3gs_lpips_workspace_bytes(8, 16, 16), dtype=torch.uint8, device="cuda")
    args = lambda n, H, W: (n, x.data_ptr(), x.data_ptr(), H, W, C.byref(tab), 0, out.data_ptr(), ws.data_ptr(), None)  # noqa: E731
    assert L.b3gs_lpips_batch(*args(1, 15, 16)) == -1 and b"at least 16" in L.b3gs_last_error()
    assert L.b3gs_lpips_batch(*args(1, 16, 15)) == -1
    assert L.b3gs_lpips_batch(*args(9, 16, 16)) == -1 and b"b3gs_lpips_batch" in L.b3gs_last_error()
    feats = (C.c_void_p * 5)(*[out.data_ptr()] * 5)
    assert L.b3gs_lpips_features(9, x.data_ptr(), 16, 16, C.byref(tab), 0, feats, ws.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                      # nothing was launched
    assert L.b3gs_lpips_batch(*args(8, 16, 16)) == 0      # the same arguments within the limits run
    torch.cuda.synchronize()
    assert torch.equal(out[:8], lpips.lpips_layers(x[:8], x[:8], w)) and bool((out[8] == -7.0).all())
    with pytest.raises(ValueError):
        lpips.lpips(x[:1, :, :15], x[:1, :, :15], w)


def _small_scene():
    """The synthetic scene tests/test_gpu_evaluate.py builds its models from, at 64x48 and 48x32 (the yardstick runs VGG on the CPU)."""
    from binocular3dgs_amd import synth
    model = synth.synth_model(20000, seed=11, device="cuda", width=200, height=144)
    cams = synth.synth_cameras(64, 48, yaws=(-8.0, 4.0), device="cuda") + synth.synth_cameras(48, 32, yaws=(3.0,), device="cuda")
    cams = [cams[0], cams[2], cams[1]]                    # interleave the resolutions: the renderer groups them
    gen = torch.Generator(device="cuda").manual_seed(2)
    for c in cams:
        c.original_image = 1.2 * torch.rand(3, c.image_height, c.image_width, device="cuda", generator=gen) - 0.1
    masks = [None if i == 0 else (torch.rand(1, c.image_height, c.image_width, device="cuda", generator=gen) > 0.2).float()
             for i, c in enumerate(cams)]
    return model, cams, torch.tensor([0.1, 0.0, 0.2], device="cuda"), masks


def test_evaluate_views_with_lpips():
    from binocular3dgs_amd import evaluate
    model, cams, bg, masks = _small_scene()
    w = lpips.random_weights(0)
    base = evaluate.evaluate_views(model, cams, bg, mode="png", masks=masks)
    res = evaluate.evaluate_views(model, cams, bg, mode="png", masks=masks, lpips_weights=w)
    assert "LPIPS" not in base and all("LPIPS" not in v for v in base["per_view"])
    for key in ("SSIM", "PSNR", "L1"):                    # bit-equal to the call without weights
        assert res[key] == base[key] and [v[key] for v in res["per_view"]] == [v[key] for v in base["per_view"]]
    assert res["LPIPS"] == float(torch.tensor([v["LPIPS"] for v in res["per_view"]]).mean())
    renders = evaluate.render_views(model, cams, bg)
    for v, img, cam, m in zip(res["per_view"], renders, cams, masks):
        _, pi, pg = evaluate.image_metrics([img], [cam.original_image], None if m is None else [m], evaluate.QUANTIZE, prepared=True)
        ref = float(lpips_ref.lpips(pi.cpu(), pg.cpu(), w)[0])
        ref32 = float(lpips_ref.lpips(pi.cpu(), pg.cpu(), w, dtype=torch.float32)[0])
        d32, dev = abs(ref32 - ref) / ref, abs(v["LPIPS"] - ref) / ref
        print(f"view {cam.image_width}x{cam.image_height}: LPIPS {v['LPIPS']:.7f}, d32 = {d32:.3e}, device = {dev:.3e}")
        assert ref > 0 and dev <= FACTOR * max(d32, float(np.finfo(np.float32).eps))
    # mode "report" takes the clamped pair
    rep = evaluate.evaluate_views(model, cams[:1], bg, mode="report", lpips_weights=w)
    assert rep["per_view"][0]["LPIPS"] > 0 and rep["per_view"][0]["LPIPS"] != res["per_view"][0]["LPIPS"]


def test_command_line_writes_three_keys(tmp_path, capsys):
    from binocular3dgs_amd import evaluate
    from binocular3dgs_amd.gaussian_model import GaussianModel
    from binocular3dgs_amd.scene import Scene
    src = shutil.copytree(os.path.join(ROOT, "tests", "golden", "scene_llff"), tmp_path / "scene_llff")
    out = tmp_path / "model"
    np.random.seed(0)
    model = GaussianModel(1)
    scene = Scene.from_dataset(str(src), model, eval=True, n_views=3, dataset_name="LLFF", resolution=1, init_points="sparse",
                               model_path=str(out), shuffle=False)
    scene.save(7)
    ntest = len(scene.getTestCameras())
    assert ntest > 0
    with open(out / "cfg_args", "w") as fp:
        fp.write(f"Namespace(source_path={str(src)!r}, images='images', eval=True, n_views=3, dataset_name='LLFF', resolution=1, "
                 "white_background=False, sh_degree=1, init_points='sparse')")
    npz = str(tmp_path / "lpips_vgg.npz")
    lpips.save_weights(npz, lpips.random_weights(0))
    assert evaluate.main(["-m", str(out), "--lpips_npz", npz]) == 0
    text = capsys.readouterr().out
    assert "  SSIM : " in text and "  PSNR : " in text and "  LPIPS: " in text
    full = json.load(open(out / "results.json"))
    per = json.load(open(out / "per_view.json"))
    assert list(full) == list(per) == ["ours_7"]
    assert list(full["ours_7"]) == ["SSIM", "PSNR", "LPIPS"] == list(per["ours_7"])
    names = ["{0:05d}.png".format(i) for i in range(ntest)]
    for key in ("SSIM", "PSNR", "LPIPS"):
        assert list(per["ours_7"][key]) == names
        assert full["ours_7"][key] == torch.tensor(list(per["ours_7"][key].values())).mean().item()
        assert all(np.isfinite(v) for v in per["ours_7"][key].values())
    assert all(v > 0 for v in per["ours_7"]["LPIPS"].values())
    # without weights: the two keys of before
    assert evaluate.main(["-m", str(out), "-s", str(src), "--iteration", "7"]) == 0
    assert list(json.load(open(out / "results.json"))["ours_7"]) == ["SSIM", "PSNR"]
