"""GPU: the undistorter on the device (binocular3dgs_amd/undistort.py, csrc/undistort.hip) against tests/undistort_ref.py.

Shapes are chosen so that no tile of a kernel is full: source 37 x 29, output 41 x 31, plus a 1 x 1 output.

  1. remap equals the yardstick bit for bit (out and valid) for C in {1, 3, 4} and n in {1, 3, 8, 9} on a hand-built map: entries
     outside on each side, exactly at the validity bounds, ax / ay in {0, 255}, clamped taps at every corner, +-2^30;
     a batch of 8 and one image at a time give the same bytes;
  2. undistort_map equals it bit for bit for the four polynomial models; for the three fisheye models an entry may differ by
     one unit (device and libm atan may differ in the last place), and at most 1e-3 of the entries may;
  3. camera_points: both directions bit for bit for the polynomial models, within 1e-9 px for the fisheye ones; a point behind
     the fold-over comes back unconverged and finite;
  4. undistort_dataset on a tiny SIMPLE_RADIAL dataset: the existing reader accepts the output."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

import undistort_ref as ref
from binocular3dgs_amd import undistort as U

pytestmark = pytest.mark.gpu

WS, HS = ref.TEST_SIZE
WO, HO = ref.TEST_PINHOLE[:2]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def camera(model):
    return U.CameraModel(model, WS, HS, ref.TEST_CAMERAS[model])


@functools.lru_cache(maxsize=None)
def hand_map():
    """int32 [HO, WO, 2]: random entries reaching 1.5 pixels outside the source on every side, then the special ones"""
    rng = np.random.default_rng(7)
    m = np.stack([rng.integers(-400, 256 * WS + 400, (HO, WO)), rng.integers(-400, 256 * HS + 400, (HO, WO))], axis=2).astype(np.int32)
    xin, yin = 256 * 11 + 77, 256 * 13 + 200
    bx = (-128, -129, 256 * WS - 128, 256 * WS - 129)
    by = (-128, -129, 256 * HS - 128, 256 * HS - 129)
    special = [(x, yin) for x in bx] + [(xin, y) for y in by]
    special += [(x, y) for x in (-128, 256 * WS - 129) for y in (-128, 256 * HS - 129)]            # clamped taps at every corner
    special += [(x, y) for x in (0, 255, 256 * (WS - 1), 256 * (WS - 2) + 255) for y in (0, 255, 256 * (HS - 1), 256 * (HS - 2) + 255)]
    special += [(256 * 5 + a, 256 * 6 + b) for a in (0, 255) for b in (0, 255)]
    special += [(-(1 << 30), -(1 << 30)), (-(1 << 30), yin), (xin, 1 << 30), (1 << 30, 1 << 30), (-900, yin), (256 * WS + 900, yin),
                (xin, -900), (xin, 256 * HS + 900)]
    flat = m.reshape(-1, 2)
    where = rng.permutation(len(flat))[:len(special)]
    flat[where] = np.array(special, dtype=np.int32)
    flat[0], flat[-1] = (-128, -128), (256 * WS - 129, 256 * HS - 129)                             # the first and the last pixel
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def images(C):
    rng = np.random.default_rng(10 + C)
    a = rng.integers(0, 256, (9, HS, WS, C), dtype=np.uint8)
    a[0, 0, 0], a[0, -1, -1], a[1, 0, -1], a[1, -1, 0] = 255, 255, 255, 255
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def remap_ref(C, k):
    return ref.remap(images(C)[k], hand_map())


def test_the_hand_built_map_holds_its_cases():
    m = hand_map().reshape(-1, 2).astype(np.int64)
    X, Y = m[:, 0], m[:, 1]
    assert (X < -128).any() and (X >= 256 * WS - 128).any() and (Y < -128).any() and (Y >= 256 * HS - 128).any()
    for v in (-128, -129, 256 * WS - 128, 256 * WS - 129, -(1 << 30)):
        assert (X == v).any(), v
    for v in (-128, -129, 256 * HS - 128, 256 * HS - 129):
        assert (Y == v).any(), v
    inside = (X >= -128) & (X < 256 * WS - 128) & (Y >= -128) & (Y < 256 * HS - 128)
    assert 0.5 < inside.mean() < 0.99
    for a in (0, 255):
        for b in (0, 255):
            assert (inside & ((X & 255) == a) & ((Y & 255) == b)).any()


@pytest.mark.parametrize("n", [1, 3, 8, 9])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_remap_equals_the_yardstick_bit_for_bit(C, n):
    m = torch.from_numpy(hand_map().copy()).cuda()
    src = [images(C)[k] if C > 1 or k % 2 else images(C)[k][:, :, 0] for k in range(n)]        # [H,W] counts as one channel
    out, valid = U.remap([np.ascontiguousarray(s) for s in src], m)
    assert out.shape == (n, HO, WO, C) and valid.shape == (HO, WO) and out.dtype == valid.dtype == torch.uint8
    out, valid = host(out), host(valid)
    for k in range(n):
        want, wv = remap_ref(C, k)
        assert same_bits(valid, wv)
        assert same_bits(out[k], want), (C, n, k, int((out[k] != want).sum()))
    assert (out[:, valid == 0] == 0).all()
    if n == 8:                                          # the same images one at a time
        for k in range(n):
            one, v1 = U.remap([torch.from_numpy(images(C)[k].copy()).cuda()], m)
            assert same_bits(host(one)[0], out[k]) and same_bits(host(v1), valid)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_remap_of_a_one_pixel_output_and_a_one_pixel_source(C):
    for entry in ((256 * 36, 256 * 28), (256 * 3 + 100, 256 * 4 + 9), (-129, 0)):
        m = np.array(entry, dtype=np.int32).reshape(1, 1, 2)
        out, valid = U.remap([images(C)[2]], torch.from_numpy(m).cuda())
        want, wv = ref.remap(images(C)[2], m)
        assert same_bits(host(out)[0], want) and same_bits(host(valid), wv)
    tiny = images(C)[3][:1, :1]
    m = hand_map()[:5, :7]
    out, valid = U.remap([np.ascontiguousarray(tiny)], torch.from_numpy(m.copy()).cuda())
    want, wv = ref.remap(tiny, m)
    assert same_bits(host(out)[0], want) and same_bits(host(valid), wv)


@pytest.mark.parametrize("model", ref.POLYNOMIAL)
def test_undistort_map_equals_the_yardstick_bit_for_bit(model):
    for pin in (ref.TEST_PINHOLE, (1, 1, 28.0, 33.0), (70, 3, 9.0, 40.0)):
        got = host(U.undistort_map(camera(model), pin))
        want = ref.undistort_map(model, ref.TEST_CAMERAS[model], pin)
        assert same_bits(got, want), (model, pin, int((got != want).sum()))


@pytest.mark.parametrize("model", ref.FISHEYE)
def test_fisheye_maps_differ_by_at_most_one_unit_in_very_few_entries(model):
    differing = total = 0
    for pin in (ref.TEST_PINHOLE, (1, 1, 28.0, 33.0), (70, 3, 9.0, 40.0)):
        got = host(U.undistort_map(camera(model), pin)).astype(np.int64)
        want = ref.undistort_map(model, ref.TEST_CAMERAS[model], pin).astype(np.int64)
        assert got.shape == want.shape
        d = np.abs(got - want)
        print(model, pin, "entries that differ:", int((d != 0).sum()), "of", d.size, "largest:", int(d.max()))
        assert d.max() <= 1, (model, pin, int(d.max()))
        differing += int((d != 0).sum())
        total += d.size
    assert differing <= 1e-3 * total, (model, differing, total)


def test_a_map_entry_that_is_not_finite_or_too_large_is_pinned():
    # a pinhole so wide that FULL_OPENCV's denominator crosses zero and the radial polynomials overflow 2^30
    cam = U.CameraModel("FULL_OPENCV", WS, HS, (31.0, 27.5, 17.3, 15.6, 0.3, 0.2, 0.0, 0.0, 0.1, -0.5, 0.0, 0.0))
    pin = (33, 5, 1e-3, 1e-3)
    got = host(U.undistort_map(cam, pin))
    want = ref.undistort_map("FULL_OPENCV", cam.params, pin)
    assert same_bits(got, want) and np.abs(got.astype(np.int64)).max() == 1 << 30
    # and a coefficient so large that u * (k r^2) is infinite away from the axes: -2^30
    cam = U.CameraModel("SIMPLE_RADIAL", WS, HS, (31.0, 17.3, 15.6, 1e300))
    got = host(U.undistort_map(cam, pin))
    want = ref.undistort_map("SIMPLE_RADIAL", cam.params, pin)
    assert same_bits(got, want) and (got[0, 0] == -(1 << 30)).all() and tuple(got[2, 16]) == (4301, 3866)


def points(seed=3, n=700):
    rng = np.random.default_rng(seed)
    return rng.uniform((-2.0, -2.0), (WS + 2.0, HS + 2.0), (n, 2))


@pytest.mark.parametrize("model", sorted(ref.MODEL_PARAMS))
def test_camera_points_both_directions(model):
    cam, p = camera(model), ref.TEST_CAMERAS[model]
    xy = points()
    d = host(U.distort_points(cam, xy))
    wd, _ = ref.camera_points(model, p, xy, False)
    u, conv = U.undistort_points(cam, d)                       # the distorted points are images of points: all invertible
    u, conv = host(u), host(conv)
    wu, wconv = ref.camera_points(model, p, d, True)
    if model in ref.POLYNOMIAL:
        assert same_bits(d, wd), model
        assert same_bits(conv, wconv) and same_bits(u, wu), (model, int((conv != wconv).sum()))
    else:
        print(model, "distort:", np.abs(d - wd).max(), "undistort:", np.abs(u - wu).max())
        assert np.abs(d - wd).max() <= 1e-9 and same_bits(conv, wconv) and np.abs(u - wu).max() <= 1e-9, model
    assert conv.all() and np.abs(u - xy).max() <= 1e-9, (model, np.abs(u - xy).max())


def test_a_point_behind_the_fold_over_comes_back_unconverged_and_finite():
    # SIMPLE_RADIAL with k < 0: the distorted radius r (1 + k r^2) has its maximum (2/3) sqrt(-1 / (3 k)) = 0.84 at the fold-over
    # radius 1.26; distorted radii beyond that maximum are the image of no point in front of the fold-over
    model, p = "SIMPLE_RADIAL", ref.TEST_CAMERAS["SIMPLE_RADIAL"]
    f, cx, cy, k = p
    rmax = 2 / 3 * np.sqrt(-1 / (3 * k))
    ang = np.linspace(0.1, 6.2, 9)
    bad = np.concatenate([np.stack([cx + f * r * np.cos(ang), cy + f * r * np.sin(ang)], axis=1) for r in (1.02 * rmax, 1.5, 4.0)])
    good = np.stack([cx + f * 0.95 * rmax * np.cos(ang), cy + f * 0.95 * rmax * np.sin(ang)], axis=1)
    xy = np.concatenate([bad, good])
    u, conv = U.undistort_points(camera(model), xy)
    u, conv = host(u), host(conv)
    wu, wconv = ref.camera_points(model, p, xy, True)
    assert same_bits(u, wu) and same_bits(conv, wconv)
    assert (conv[:len(bad)] == 0).all() and (conv[len(bad):] == 1).all()
    assert np.isfinite(u).all() and same_bits(u[:len(bad)], xy[:len(bad)])
    # a fisheye point beyond the lens' 180 degrees: no preimage either
    fcam = U.CameraModel("OPENCV_FISHEYE", WS, HS, (31.0, 27.5, 17.3, 15.6, 0.0, 0.0, 0.0, 0.0))
    u, conv = U.undistort_points(fcam, np.array([[17.3 + 31.0 * 1.7, 15.6], [17.3 + 31.0 * 0.5, 15.6]]))
    assert host(conv).tolist() == [0, 1] and np.isfinite(host(u)).all()


def test_pinhole_rule_on_the_device_equals_the_yardstick():
    for model in ("SIMPLE_RADIAL", "OPENCV", "OPENCV_FISHEYE"):
        for blank in (0.0, 0.5, 1.0):
            got = U.pinhole_for(camera(model), blank=blank)
            want = ref.pinhole_for(model, WS, HS, ref.TEST_CAMERAS[model], blank=blank)
            assert got == want, (model, blank, got, want)


def test_undistort_dataset_writes_what_the_reader_accepts(tmp_path):
    from binocular3dgs_amd import dataset_readers as dr
    from binocular3dgs_amd.frames import read_png, write_png
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    os.makedirs(os.path.join(src, "images"))
    os.makedirs(os.path.join(src, "sparse/0"))
    W, H = 32, 24
    params = (30.0, 16.7, 11.4, -0.12)
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
    U.write_cameras_bin(os.path.join(src, "sparse/0/cameras.bin"), {1: ("SIMPLE_RADIAL", W, H, params)})
    recs = {}
    for k in range(4):
        write_png(os.path.join(src, "images", f"im{k}.png"), imgs[k])
        q = np.array([1.0, 0.01 * k, 0.0, 0.0])
        xys = rng.uniform((1, 1), (W - 1, H - 1), (5, 2))
        recs[10 + k] = (q / np.linalg.norm(q), np.array([0.1 * k, 0.0, 0.0]), 1, f"im{k}.png", xys, np.arange(5) + 1)
    U.write_images_bin(os.path.join(src, "sparse/0/images.bin"), recs)
    shutil.copyfile(os.path.join(ROOT, "tests/golden/scene_llff/sparse/0/points3D.bin"), os.path.join(src, "sparse/0/points3D.bin"))
    np.save(os.path.join(src, "poses_bounds.npy"), np.arange(6.0))

    pins = U.undistort_dataset(src, dst)
    Wo, Ho, fx, fy = pins[1]
    assert pins[1] == ref.pinhole_for("SIMPLE_RADIAL", W, H, params) and (fx, fy) == (30.0, 30.0)
    scene = dr.read_scene(dst, eval=False, init_points="sparse")
    assert len(scene.train_cameras) == 4 and len(scene.points) > 0
    cams = dr.read_cameras_bin(os.path.join(dst, "sparse/0/cameras.bin"))
    assert cams[1][:3] == ("PINHOLE", Wo, Ho) and cams[1][3].tolist() == [30.0, 30.0, Wo / 2, Ho / 2]
    m = ref.undistort_map("SIMPLE_RADIAL", params, pins[1])
    full = U.read_images_bin_full(os.path.join(dst, "sparse/0/images.bin"))
    assert list(full) == list(recs)
    for k in range(4):
        want, valid = ref.remap(imgs[k], m)
        assert (valid == 255).all()
        assert same_bits(read_png(os.path.join(dst, "images", f"im{k}.png")), want)
        rec = full[10 + k]
        assert rec[3] == f"im{k}.png" and rec[2] == 1 and np.array_equal(rec[0], recs[10 + k][0]) and np.array_equal(rec[1], recs[10 + k][1])
        wu, ok = ref.camera_points("SIMPLE_RADIAL", params, recs[10 + k][4], True)
        assert ok.all() and np.array_equal(rec[5], recs[10 + k][5])
        wxy = np.stack([(wu[:, 0] - 16.7) / 30.0 * fx + Wo / 2, (wu[:, 1] - 11.4) / 30.0 * fy + Ho / 2], axis=1)
        assert same_bits(rec[4], wxy)
    for name in ("sparse/0/points3D.bin", "poses_bounds.npy"):
        assert open(os.path.join(dst, name), "rb").read() == open(os.path.join(src, name), "rb").read()
    for c in scene.train_cameras:
        assert (c.width, c.height) == (Wo, Ho) and os.path.exists(c.image_path)
