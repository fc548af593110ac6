"""CPU: the numpy yardstick of the undistorter (tests/undistort_ref.py) against the properties the device code is then held to,
the COLMAP writers against the existing readers, and the argument errors that never reach a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_ref as ref  # noqa: E402


def test_zero_coefficients_give_the_identity_map():
    W, H = 38, 30
    for model, n in ref.MODEL_PARAMS.items():
        if model in ref.FISHEYE:
            continue                                  # (a fisheye lens with zero coefficients is still a fisheye)
        p = np.zeros(n)
        if n in (4, 5):
            p[:3] = 29.0, W / 2, H / 2
            pin = (W, H, 29.0, 29.0)
        else:
            p[:4] = 29.0, 33.0, W / 2, H / 2
            pin = (W, H, 29.0, 33.0)
        m = ref.undistort_map(model, p, pin)
        assert np.array_equal(m[..., 0], np.broadcast_to(256 * np.arange(W)[None, :], (H, W))), model
        assert np.array_equal(m[..., 1], np.broadcast_to(256 * np.arange(H)[:, None], (H, W))), model


def test_identity_map_resamples_to_the_same_image():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (30, 38, 3), dtype=np.uint8)
    m = ref.undistort_map("SIMPLE_RADIAL", (29.0, 19.0, 15.0, 0.0), (38, 30, 29.0, 29.0))
    out, valid = ref.remap(img, m)
    assert np.array_equal(out, img) and (valid == 255).all()


@pytest.mark.parametrize("model", sorted(ref.MODEL_PARAMS))
def test_distort_of_undistort_is_the_point(model):
    W, H = ref.TEST_SIZE
    # moderate coefficients: a third of the strong ones of the GPU tests
    p = np.array(ref.TEST_CAMERAS[model], dtype=np.float64)
    nk = 3 if len(p) in (4, 5) else 4
    p[nk:] /= 3.0
    rng = np.random.default_rng(1)
    xy = rng.uniform((0, 0), (W, H), (500, 2))
    und, ok = ref.camera_points(model, p, xy, True)
    assert ok.all(), model
    back, _ = ref.camera_points(model, p, und, False)
    assert np.abs(back - xy).max() <= 1e-9, (model, np.abs(back - xy).max())


@pytest.mark.parametrize("k", [-0.18, 0.22], ids=["barrel", "pincushion"])
def test_blank_zero_leaves_no_blank_pixel(k):
    W, H = 64, 48
    p = (50.0, 30.5, 25.25, k)                        # off-centre principal point
    pin = ref.pinhole_for("SIMPLE_RADIAL", W, H, p, blank=0.0)
    assert 1 <= pin[0] <= 2 * W and 1 <= pin[1] <= 2 * H and pin[2:] == (50.0, 50.0)
    m = ref.undistort_map("SIMPLE_RADIAL", p, pin)
    _, valid = ref.remap(np.zeros((H, W), dtype=np.uint8), m)
    assert (valid == 255).all(), (k, pin, int((valid == 0).sum()))
    # and blank = 1 keeps every border pixel: the output is larger and does show blank pixels
    pin1 = ref.pinhole_for("SIMPLE_RADIAL", W, H, p, blank=1.0, max_scale=4.0)
    assert pin1[0] >= pin[0] and pin1[1] >= pin[1] and pin1[0] * pin1[1] > pin[0] * pin[1]


def test_pinhole_rule_of_the_module_is_the_yardsticks_with_a_given_size():
    from binocular3dgs_amd import undistort as U
    cam = U.CameraModel("OPENCV", 37, 29, ref.TEST_CAMERAS["OPENCV"])
    assert U.pinhole_for(cam, size=(41, 31)) == ref.pinhole_for("OPENCV", 37, 29, ref.TEST_CAMERAS["OPENCV"], size=(41, 31)) \
        == (41, 31, 31.0, 27.5)
    s = U.scaled_to(cam, 74, 87)
    assert s.params[:4] == (62.0, 82.5, 34.6, 15.6 * 3) and s.params[4:] == cam.params[4:] and (s.width, s.height) == (74, 87)
    one = U.scaled_to(U.CameraModel("RADIAL", 37, 29, ref.TEST_CAMERAS["RADIAL"]), 74, 58)
    assert one.params == (62.0, 34.6, 31.2, -0.25, 0.06)


def test_writers_round_trip_through_the_readers(tmp_path):
    from binocular3dgs_amd import dataset_readers as dr
    from binocular3dgs_amd import undistort as U
    cams = {3: ("PINHOLE", 41, 31, np.array([28.0, 33.0, 20.5, 15.5])), 1: ("SIMPLE_RADIAL", 37, 29, np.array([31.0, 17.3, 15.6, -0.21])),
            7: ("FULL_OPENCV", 9, 8, np.arange(12.0))}
    U.write_cameras_bin(str(tmp_path / "cameras.bin"), cams)
    back = dr.read_cameras_bin(str(tmp_path / "cameras.bin"))
    assert list(back) == list(cams)
    for cid, (name, w, h, p) in cams.items():
        assert back[cid][:3] == (name, w, h) and np.array_equal(back[cid][3], p)
    rng = np.random.default_rng(2)
    images = {5: (rng.normal(size=4), rng.normal(size=3), 3, "a/b.png", rng.uniform(0, 30, (6, 2)), np.array([4, -1, 9, 2 ** 40, 0, 1])),
              2: (rng.normal(size=4), rng.normal(size=3), 1, "c.png"),
              9: (rng.normal(size=4), rng.normal(size=3), 1, "d.JPG", np.zeros((0, 2)), np.zeros(0, dtype=np.int64))}
    U.write_images_bin(str(tmp_path / "images.bin"), images)
    back = dr.read_images_bin(str(tmp_path / "images.bin"))
    assert list(back) == list(images)
    for iid, rec in images.items():
        assert np.array_equal(back[iid][0], rec[0]) and np.array_equal(back[iid][1], rec[1]) and back[iid][2:] == rec[2:4]
    full = U.read_images_bin_full(str(tmp_path / "images.bin"))
    assert np.array_equal(full[5][4], images[5][4]) and np.array_equal(full[5][5], images[5][5]) and len(full[2][4]) == 0
    with pytest.raises(ValueError, match="NOT_A_MODEL"):
        U.write_cameras_bin(str(tmp_path / "x.bin"), {1: ("NOT_A_MODEL", 4, 4, (1.0,))})


def test_argument_errors_never_reach_a_device():
    import torch
    from binocular3dgs_amd import _C, _lib
    from binocular3dgs_amd import undistort as U
    for name in ("FOV", "THIN_PRISM_FISHEYE", "PINHOLE"):
        with pytest.raises(ValueError, match=name):
            U.CameraModel(name, 37, 29, (1.0,) * 5)
    with pytest.raises(ValueError, match="SIMPLE_RADIAL has 4 parameters"):
        U.CameraModel("SIMPLE_RADIAL", 37, 29, (30.0, 18.0, 14.0))
    assert set(U.SUPPORTED_MODELS) == set(ref.MODEL_PARAMS)
    m = torch.zeros(31, 41, 2, dtype=torch.int32)
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8)   # noqa: E731
    with pytest.raises(ValueError, match="channels"):
        U.remap([z(29, 37, 2)], m)
    with pytest.raises(ValueError, match="one size"):
        U.remap([z(29, 37, 3), z(29, 36, 3)], m)
    with pytest.raises(ValueError, match="int32"):
        U.remap([z(29, 37, 3)], m.float())
    with pytest.raises(ValueError, match="1..8"):
        _C.remap([z(29, 37, 3)] * 9, m)
    with pytest.raises(ValueError, match="channels"):
        _C.remap([z(29, 37, 2)], m)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.remap([z(29, 37, 3)], m)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.camera_points(2, 37, 29, [30.0, 18.0, 14.0, 0.1], torch.zeros(4, 2, dtype=torch.float64), False)

    # the C ABI itself: B3GS_ERR_ARG before the first HIP call
    L = _lib.lib()
    ERR_ARG = -1

    def cam(model, n):
        c = _lib.B3gsCameraModel()
        c.model, c.width, c.height, c.n_params = model, 37, 29, n
        for i in range(n):
            c.params[i] = 30.0 if i < 2 else 0.01
        return c
    for model, n in ((7, 5), (10, 12), (1, 4), (0, 3), (99, 4)):          # FOV, THIN_PRISM_FISHEYE, PINHOLE, SIMPLE_PINHOLE
        assert L.b3gs_camera_points(C.byref(cam(model, n)), 0, 4, 256, 256, None, None) == ERR_ARG
        assert b"unsupported camera model" in L.b3gs_last_error()
        assert L.b3gs_undistort_map(C.byref(cam(model, n)), 41, 31, 28.0, 33.0, 256, None) == ERR_ARG
    for model, n in ((2, 5), (3, 4), (4, 12), (6, 8), (5, 4), (8, 5), (9, 8)):
        assert L.b3gs_camera_points(C.byref(cam(model, n)), 0, 4, 256, 256, None, None) == ERR_ARG
        assert b"parameter count" in L.b3gs_last_error()
    good = cam(2, 4)
    assert L.b3gs_camera_points(C.byref(good), 0, 0, None, None, None, None) == 0                  # no points: nothing to do
    assert L.b3gs_camera_points(C.byref(good), 0, -1, 256, 256, None, None) == ERR_ARG
    assert L.b3gs_camera_points(C.byref(good), 1, 4, 256, 256, None, None) == ERR_ARG              # no converged bytes
    assert L.b3gs_undistort_map(C.byref(good), 0, 31, 28.0, 33.0, 256, None) == ERR_ARG
    assert L.b3gs_undistort_map(C.byref(good), 41, 31, 0.0, 33.0, 256, None) == ERR_ARG
    assert L.b3gs_undistort_map(C.byref(good), 41, 31, 28.0, 33.0, 260, None) == ERR_ARG           # map not 8-byte aligned
    ptrs = (C.c_void_p * 9)(*([256] * 9))
    for nviews, Hs, Ws, ch, H, W in ((9, 29, 37, 3, 31, 41), (0, 29, 37, 3, 31, 41), (1, 29, 37, 2, 31, 41), (1, 29, 37, 5, 31, 41),
                                     (1, 0, 37, 3, 31, 41), (1, 29, 37, 3, 0, 41), (1, 29, 1 << 21, 1, 31, 41)):
        assert L.b3gs_remap_batch(nviews, ptrs, Hs, Ws, ch, 256, H, W, ptrs, 256, None) == ERR_ARG, (nviews, Hs, Ws, ch, H, W)
    assert L.b3gs_remap_batch(1, ptrs, 29, 37, 3, None, 31, 41, ptrs, 256, None) == ERR_ARG
    assert L.b3gs_remap_batch(1, ptrs, 29, 37, 3, 256, 31, 41, ptrs, None, None) == ERR_ARG


def test_reader_still_refuses_a_distorted_model_and_names_the_command(tmp_path):
    import struct
    from binocular3dgs_amd import dataset_readers as dr
    from binocular3dgs_amd import undistort as U
    os.makedirs(tmp_path / "sparse/0")
    U.write_cameras_bin(str(tmp_path / "sparse/0/cameras.bin"), {1: ("OPENCV", 32, 24, ref.TEST_CAMERAS["OPENCV"])})
    U.write_images_bin(str(tmp_path / "sparse/0/images.bin"), {1: ((1.0, 0, 0, 0), (0.0, 0, 0), 1, "a.png")})
    with pytest.raises(ValueError, match=r"OPENCV.*binocular3dgs_amd\.undistort"):
        dr.read_scene(str(tmp_path), eval=False, init_points="sparse")
    assert struct.calcsize("<i7di") == 64
