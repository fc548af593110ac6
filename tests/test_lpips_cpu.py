"""CPU: the parts of LPIPS (binocular3dgs_amd/lpips.py, csrc/lpips.hip) that need no device -- the ABI surface, the weight
files (torchvision / LPIPS key names, the .npz round trip, errors that name the key), write_results with and without the
LPIPS key, and the yardstick tests/lpips_ref.py itself (identical images, a hand-computed tap)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lpips_ref
from binocular3dgs_amd import _lib, evaluate, lpips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("b3gs_lpips_workspace_bytes", "b3gs_lpips_batch", "b3gs_lpips_features")


def _same(a: lpips.LpipsWeights, b: lpips.LpipsWeights) -> bool:
    ts = zip(a.conv_w + a.conv_b + a.lin, b.conv_w + b.conv_b + b.lin)
    return all(x.dtype == y.dtype == torch.float32 and torch.equal(x, y) for x, y in ts) and a.shift == b.shift and a.scale == b.scale


def _state_dicts(w):
    vgg, lin = {}, {}
    for i, k in enumerate(lpips.VGG_LAYERS):
        vgg[f"features.{k}.weight"] = w.conv_w[i].clone()
        vgg[f"features.{k}.bias"] = w.conv_b[i].clone()
    for name, shape in (("classifier.0.weight", (8, 8)), ("classifier.0.bias", (8,))):      # keys the loader does not read
        vgg[name] = torch.zeros(shape)
    for l in range(5):
        lin[f"lin{l}.model.1.weight"] = w.lin[l].reshape(1, -1, 1, 1).clone()
    return vgg, lin


def test_abi_surface():
    with open(os.path.join(ROOT, "include", "b3gs_raster.h")) as fp:
        header = fp.read()
    for name in SYMBOLS:
        assert name + "(" in header and name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 18 and "#define B3GS_ABI_VERSION 18" in header
    L = _lib.lib()
    assert L.b3gs_abi_version() == 18
    for name in SYMBOLS:
        getattr(L, name)


def test_workspace_bytes_and_argument_checks_without_a_device():
    L = _lib.lib()
    sizes = [L.b3gs_lpips_workspace_bytes(n, 600, 800) for n in range(1, 9)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    # two activation buffers of 2 n * 64 * H * W floats
    assert sizes[0] >= 2 * 2 * 64 * 600 * 800 * 4
    assert L.b3gs_lpips_workspace_bytes(1, 16, 16) > 0
    assert L.b3gs_lpips_workspace_bytes(0, 600, 800) == 0 and L.b3gs_lpips_workspace_bytes(9, 600, 800) == 0
    assert L.b3gs_lpips_workspace_bytes(1, 15, 800) == 0 and L.b3gs_lpips_workspace_bytes(1, 600, 15) == 0
    w = _lib.B3gsLpipsWeights()
    p = C.c_void_p(256)                       # never dereferenced: the checks come first
    for i in range(13):
        w.conv_w[i] = w.conv_b[i] = 256
    for l in range(5):
        w.lin[l] = 256
    w.scale[0] = w.scale[1] = w.scale[2] = 1.0
    assert L.b3gs_lpips_batch(1, p, p, 15, 16, C.byref(w), 0, p, p, None) == -1
    assert b"b3gs_lpips_batch" in L.b3gs_last_error() and b"16" in L.b3gs_last_error()
    assert L.b3gs_lpips_batch(9, p, p, 16, 16, C.byref(w), 0, p, p, None) == -1
    assert b"b3gs_lpips_batch" in L.b3gs_last_error() and b"8" in L.b3gs_last_error()
    assert L.b3gs_lpips_batch(1, None, p, 16, 16, C.byref(w), 0, p, p, None) == -1
    assert L.b3gs_lpips_features(1, p, 16, 15, C.byref(w), 0, None, p, None) == -1
    assert b"b3gs_lpips_features" in L.b3gs_last_error()


def test_load_weights_from_the_two_state_dicts(tmp_path):
    w = lpips.random_weights(3)
    vgg, lin = _state_dicts(w)
    vp, lp = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg_lin.pth")
    torch.save(vgg, vp)
    torch.save(lin, lp)
    got = lpips.load_weights(vp, lp)
    assert _same(got, w)
    assert got.shift == tuple(float(np.float32(v)) for v in (-.030, -.088, -.188))
    assert got.scale == tuple(float(np.float32(v)) for v in (.458, .448, .450))
    # a missing key and a wrong shape name the key
    bad = dict(vgg)
    del bad["features.17.bias"]
    torch.save(bad, vp)
    with pytest.raises(ValueError, match=r"features\.17\.bias"):
        lpips.load_weights(vp, lp)
    bad = dict(vgg)
    bad["features.5.weight"] = torch.zeros(128, 64, 3, 2)
    torch.save(bad, vp)
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        lpips.load_weights(vp, lp)
    torch.save(vgg, vp)
    bad = dict(lin)
    del bad["lin3.model.1.weight"]
    torch.save(bad, lp)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        lpips.load_weights(vp, lp)
    bad = dict(lin)
    bad["lin0.model.1.weight"] = torch.zeros(1, 63, 1, 1)
    torch.save(bad, lp)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        lpips.load_weights(vp, lp)


def test_npz_round_trip_and_random_weights(tmp_path):
    w = lpips.random_weights(3)
    assert _same(w, lpips.random_weights(3)) and not _same(w, lpips.random_weights(4))
    path = str(tmp_path / "lpips_vgg.npz")
    lpips.save_weights(path, w)
    assert _same(lpips.load_weights(path), w)
    custom = lpips.LpipsWeights(w.conv_w, w.conv_b, w.lin, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    lpips.save_weights(path, custom)
    got = lpips.load_weights(path)
    assert got.shift == (0.0, 0.0, 0.0) and got.scale == (1.0, 1.0, 1.0)
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    del arrays["lin2"]
    np.savez(path, **arrays)
    with pytest.raises(ValueError, match="lin2"):
        lpips.load_weights(path)
    # .to() packs [K', Cout] with row 9 c + 3 ky + kx (one zero row behind the first convolution's 27)
    p = w.to("cpu")
    assert p is w.to("cpu") and p.to("cpu") is p
    pw = p.packed[0]
    assert pw[0].shape == (28, 64) and torch.equal(pw[0][27], torch.zeros(64)) and pw[5].shape == (9 * 256, 256)
    assert pw[0][9 * 2 + 3 * 1 + 2, 7] == w.conv_w[0][7, 2, 1, 2] and pw[5][9 * 100 + 3 * 2 + 0, 31] == w.conv_w[5][31, 100, 2, 0]


def test_write_results_with_and_without_lpips(tmp_path):
    names = ["00000.png", "00001.png", "00002.png"]
    base = [{"SSIM": 0.91, "PSNR": 20.5, "L1": 0.02}, {"SSIM": 0.87, "PSNR": 19.25, "L1": 0.03}, {"SSIM": 0.5, "PSNR": 11.0, "L1": 0.1}]
    lp = [0.123456789, 0.2, 0.31]
    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    evaluate.write_results(str(a), "ours_30000", base, names)
    with_lp = [dict(v, LPIPS=x) for v, x in zip(base, lp)]
    out = evaluate.write_results(str(b), "ours_30000", with_lp, names)
    full = json.load(open(b / "results.json"))
    per = json.load(open(b / "per_view.json"))
    assert full == out["results"] and per == out["per_view"]
    assert list(full["ours_30000"]) == ["SSIM", "PSNR", "LPIPS"] == list(per["ours_30000"])
    assert full["ours_30000"]["LPIPS"] == torch.tensor(lp).mean().item()
    assert per["ours_30000"]["LPIPS"] == dict(zip(names, torch.tensor(lp).tolist()))
    for k in ("SSIM", "PSNR"):
        assert full["ours_30000"][k] == torch.tensor([v[k] for v in base]).mean().item()
    # one entry without the key: the output is byte for byte the one without LPIPS
    partial = [with_lp[0], base[1], with_lp[2]]
    evaluate.write_results(str(c), "ours_30000", partial, names)
    for f in ("results.json", "per_view.json"):
        assert open(c / f, "rb").read() == open(a / f, "rb").read()
    assert b"LPIPS" not in open(a / "results.json", "rb").read()


def test_yardstick_identical_images_and_a_hand_computed_tap():
    w = lpips.random_weights(1)
    x = torch.rand(2, 3, 16, 16, generator=torch.Generator().manual_seed(0))
    assert torch.equal(lpips_ref.lpips_layers(x, x.clone(), w), torch.zeros(2, 5, dtype=torch.float64))
    assert [tuple(f.shape) for f in lpips_ref.features(x, w)] == [(2, 64, 16, 16), (2, 128, 8, 8), (2, 256, 4, 4), (2, 512, 2, 2),
                                                                 (2, 512, 1, 1)]
    # constant feature maps of 4 channels at 16x16: f = (3, 0, 4, 0) has norm 5, g = (0, 0, 0, 2) norm 2; the normalised
    # difference is (.6, 0, .8, -1), so the term is .36 w0 + .64 w2 + w3 at every pixel, and the mean is that value
    f = torch.tensor([3.0, 0.0, 4.0, 0.0], dtype=torch.float64)[None, :, None, None].expand(1, 4, 16, 16)
    g = torch.tensor([0.0, 0.0, 0.0, 2.0], dtype=torch.float64)[None, :, None, None].expand(1, 4, 16, 16)
    lin = torch.tensor([0.5, 7.0, 0.25, 2.0])
    got = float(lpips_ref.tap(f, g, lin)[0])
    assert abs(got - (0.36 * 0.5 + 0.64 * 0.25 + 2.0)) < 1e-9
    # an all-zero feature vector stays zero (the eps keeps the division finite)
    assert float(lpips_ref.tap(torch.zeros(1, 4, 16, 16, dtype=torch.float64), g, lin)[0]) == pytest.approx(2.0, abs=1e-9)
    # padding after the z-score: a constant image's relu1_1 input is constant inside, zero outside
    c = torch.full((1, 3, 16, 16), 0.5)
    f1 = lpips_ref.features(c, w)[0]
    assert not torch.equal(f1[0, :, 0, 0], f1[0, :, 8, 8]) and torch.equal(f1[0, :, 7, 7], f1[0, :, 8, 8])


def test_cpu_tensors_raise_the_device_only_message():
    w = lpips.random_weights(0)
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        lpips.lpips(x, x, w)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        lpips.lpips_layers([x[0]], [x[0]], w)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        lpips.features(x, w)
