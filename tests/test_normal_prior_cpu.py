"""CPU: the normal-prior yardstick (tests/normal_prior_ref.py) against torch.autograd on the definition, a closed form (a plane
seen through the pinhole), the shared inputs' properties, the two mutants, the argument errors of the four entry points (no
device), the loader's layouts, frames and errors, and the rules between the training flags."""
import argparse
import ctypes as C
import math

import numpy as np
import pytest
import torch

import normal_prior_ref as ref

W_COS, W_L1 = 0.7, 0.3


def _exact(case):
    """the shared float32 planes as float64 (the same values): what autograd and the yardstick's float64 gradients both see"""
    d, a, t, m = case
    return d.astype(np.float64), a.astype(np.float64), t.astype(np.float64), m


def _yardstick(case, mutant=None):
    d, a, t, m = _exact(case)
    return ref.loss(d, a, t, m, *ref.TANFOV, w_cos=W_COS, w_l1=W_L1, alpha_min=ref.ALPHA_MIN, mutant=mutant, exact_inputs=True)


def _autograd(case, valid):
    d, a, t, _ = _exact(case)
    td, ta = torch.tensor(d, requires_grad=True), torch.tensor(a, requires_grad=True)
    L, dot = ref.torch_loss(td, ta, torch.tensor(t), torch.tensor(valid), *ref.TANFOV, w_cos=W_COS, w_l1=W_L1)
    if L.requires_grad:
        L.backward()
    zero = torch.zeros_like(td)
    return float(L.detach()), float(dot.detach()), (zero if td.grad is None else td.grad)[0].numpy(), (zero if ta.grad is None else ta.grad)[0].numpy()


@pytest.mark.parametrize("name", list(ref.CASES))
def test_yardstick_gradients_against_autograd(name):
    """The analytic gather against torch.autograd in float64 on an independently written formula over the yardstick's valid
    set: max |g_ref - g_autograd| <= 1e-9 max |g| for depth and for alpha.  Observed: 3x3 5.6e-17 (depth) / 4.4e-16 (alpha) of
    max |g| 4.9e-1 / 1.2; 37x29 8.7e-18 / 1.7e-17 of 2.8e-2 / 6.4e-2; 300x260 1.7e-18 / 3.5e-18 of 4.2e-3 / 8.7e-3: the worst
    ratio is 3.7e-16."""
    W, H = ref.CASES[name]
    case = ref.make_case(W, H)
    got = _yardstick(case)
    L, dot, gd, ga = _autograd(case, got["valid"] != 0)
    if name == "2x5":
        assert got["parts"][3] == 0 and not got["parts"].any() and not got["g_depth64"].any() and not got["g_alpha64"].any()
        assert np.isfinite(got["g_depth"]).all() and np.isfinite(got["g_alpha"]).all()
        return
    for what, mine, theirs in (("depth", got["g_depth64"], gd), ("alpha", got["g_alpha64"], ga)):
        err, top = np.abs(mine - theirs).max(), np.abs(theirs).max()
        print(f"{name} {what}: max |dg| {err:.3e}, max |g| {top:.3e}")
        assert top > 0 and err <= 1e-9 * top
    assert abs(got["parts"][0] - L) <= 1e-12 * max(1.0, abs(L)) and abs(got["parts"][4] - dot) <= 1e-12


@pytest.mark.parametrize("name", list(ref.CASES))
def test_shared_inputs_have_the_properties_the_device_test_relies_on(name):
    W, H = ref.CASES[name]
    case = ref.make_case(W, H)
    N, interior, thin = ref.conditions(W, H, case)
    assert thin == 0                                   # no pixel with 0 < c.c < 1e-6 |tx|^2 |ty|^2
    if name == "2x5":
        assert interior == 0 and N == 0
    else:
        assert N >= interior / 2 and N >= 1
    if name in ("37x29", "300x260"):
        assert N < interior                            # holes and masked pixels are there
        alpha, mask = case[1][0], case[3][0]
        assert (alpha[0] < ref.ALPHA_MIN).any() and (alpha[:, -1] < ref.ALPHA_MIN).any() and (mask == 0).any()
    got = ref.loss(*case, *ref.TANFOV, w_cos=W_COS, w_l1=W_L1, alpha_min=ref.ALPHA_MIN)
    for k in ("normals", "g_depth", "g_alpha"):
        assert np.isfinite(got[k]).all() and got[k].dtype == np.float32
    assert not got["normals"][:, got["valid"] == 0].any()


def test_a_plane_through_the_pinhole_has_its_own_normal():
    """depth of the plane m.X = d with alpha 1 (float64 planes: no float32 rounding of the inputs): central differences of
    points on a plane lie in the plane, so every interior normal is m, facing the camera, and the loss against it vanishes."""
    W, H = 31, 23
    m = np.array([0.3, -0.2, -0.9])
    m /= np.sqrt((m * m).sum())
    d = -2.0
    rx, ry = ref.rays(W, H, *ref.TANFOV)
    z = d / (m[0] * rx[None, :] + m[1] * ry[:, None] + m[2])
    assert (z > 0).all()
    alpha = np.ones((1, H, W))
    target = np.broadcast_to(m[:, None, None], (3, H, W)).copy()
    got = ref.loss(z[None], alpha, target, None, *ref.TANFOV, w_cos=1.0, w_l1=1.0, alpha_min=0.5, exact_inputs=True)
    inner = got["n64"][:, 1:-1, 1:-1]
    assert got["parts"][3] == (W - 2) * (H - 2) and (inner[2] < 0).all()
    assert np.abs(inner - m[:, None, None]).max() <= 1e-12 and 0 <= got["parts"][0] <= 1e-12
    # the fronto-parallel plane: the normal points at the camera
    flat = ref.loss(np.full((1, H, W), 3.0), alpha, target, None, *ref.TANFOV, alpha_min=0.5, exact_inputs=True)["n64"][:, 1:-1, 1:-1]
    assert np.abs(flat - np.array([0.0, 0.0, -1.0])[:, None, None]).max() <= 1e-12


@pytest.mark.parametrize("mutant", ["cross_order", "gather_sign"])
def test_mutants_are_caught(mutant):
    caught = []
    for name in ("3x3", "37x29"):
        W, H = ref.CASES[name]
        case = ref.make_case(W, H)
        good, bad = _yardstick(case), _yardstick(case, mutant)
        _, _, gd, _ = _autograd(case, good["valid"] != 0)
        bound = 1e-9 * np.abs(gd).max()
        assert np.abs(good["g_depth64"] - gd).max() <= bound
        caught.append(np.abs(bad["g_depth64"] - gd).max() > bound)
    assert any(caught)
    if mutant == "cross_order":      # ... and the forward sees it: the normals turn away from the camera
        assert (bad["n64"][2][bad["valid"] != 0] > 0).all() and bad["parts"][4] < 0 < good["parts"][4]


# ---- the four entry points: argument errors need no device ------------------------------------------------------------------
def test_argument_errors_of_the_entry_points_need_no_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    raw = (C.c_uint8 * 1024)()                     # host bytes: never read, the calls must fail before any HIP call
    p = (C.addressof(raw) + 255) & ~255
    nan = float("nan")
    assert L.b3gs_normal_prior_workspace_bytes(0, 4) == 0 and L.b3gs_normal_prior_workspace_bytes(4, -1) == 0
    assert L.b3gs_normal_prior_workspace_bytes(4097, 4096) == 0 and L.b3gs_normal_prior_workspace_bytes(4096, 4096) > 48 * 4096 * 4096
    assert L.b3gs_normal_prior_workspace_bytes(3, 3) % 256 == 0

    def loss_io(**over):
        io = _lib.B3gsNormalPriorIO(W=8, H=6, depth=p, alpha=p, target=p, mask=None, alpha_min=0.5, tanfovx=0.6, tanfovy=0.5, w_cos=1.0,
                                    w_l1=0.0, dL_ddepth=p, dL_dalpha=p, normals=None, valid=None, parts=p, workspace=p)
        for k, v in over.items():
            setattr(io, k, v)
        return (_lib.B3gsNormalPriorIO * 9)(*([io] * 9))

    def normals_io(**over):
        io = _lib.B3gsDepthNormalsIO(W=8, H=6, depth=p, alpha=p, mask=None, alpha_min=0.5, tanfovx=0.6, tanfovy=0.5, normals=p, valid=p)
        for k, v in over.items():
            setattr(io, k, v)
        return (_lib.B3gsDepthNormalsIO * 9)(*([io] * 9))

    def resize_io(**over):
        io = _lib.B3gsNormalResizeIO(Wsrc=5, Hsrc=4, W=8, H=6, src=p, src_mask=None, normals=p, mask=p)
        for k, v in over.items():
            setattr(io, k, v)
        return (_lib.B3gsNormalResizeIO * 9)(*([io] * 9))

    shared = [dict(W=0), dict(H=0), dict(W=4097, H=4096), dict(depth=None), dict(alpha=None), dict(alpha_min=0.0), dict(alpha_min=-1.0),
              dict(alpha_min=nan), dict(tanfovx=0.0), dict(tanfovy=-0.5), dict(tanfovx=nan)]
    table = ((L.b3gs_normal_prior_loss_batch, loss_io, b"b3gs_normal_prior_loss_batch",
              shared + [dict(target=None), dict(dL_ddepth=None), dict(dL_dalpha=None), dict(parts=None), dict(workspace=None),
                        dict(workspace=p + 8), dict(w_cos=nan), dict(w_l1=nan)]),
             (L.b3gs_depth_normals_batch, normals_io, b"b3gs_depth_normals_batch", shared + [dict(normals=None), dict(valid=None)]),
             (L.b3gs_resize_normals_batch, resize_io, b"b3gs_resize_normals_batch",
              [dict(W=0), dict(Hsrc=0), dict(Wsrc=4097, Hsrc=4096), dict(src=None), dict(normals=None), dict(mask=None)]))
    for fn, make, name, bad in table:
        for n in (0, 9, -1):
            assert fn(n, make(), None) == -1 and b"n_views" in L.b3gs_last_error()
        assert fn(1, None, None) == -1 and b"NULL" in L.b3gs_last_error()
        for over in bad:
            assert fn(1, make(**over), None) == -1, (name, over)
            assert name in L.b3gs_last_error(), (name, over, L.b3gs_last_error())


# ---- the loader -------------------------------------------------------------------------------------------------------------
def _cam(name, R=None, W=8, H=6):
    return argparse.Namespace(image_name=name, image_width=W, image_height=H, R=np.eye(3) if R is None else R)


def test_loader_layouts_png_decoding_frames_and_errors(tmp_path):
    from binocular3dgs_amd import normal_prior as npr
    from binocular3dgs_amd.frames import write_png
    rng = np.random.default_rng(0)
    n = rng.standard_normal((6, 8, 3))
    n /= np.sqrt((n * n).sum(-1, keepdims=True))
    np.save(tmp_path / "hwc.npy", n.astype(np.float64))
    np.save(tmp_path / "chw.npy", n.transpose(2, 0, 1).astype(np.float32))
    a, _ = npr._read_normal_prior(str(tmp_path), "hwc")
    b, mask = npr._read_normal_prior(str(tmp_path), "chw")
    assert a.shape == b.shape == (3, 6, 8) and a.dtype == b.dtype == np.float32 and np.array_equal(a, b) and mask is None
    assert np.array_equal(a, n.transpose(2, 0, 1).astype(np.float32))
    # PNG: n = 2 c / 255 - 1, and the mask next to it
    c = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)
    c[0, 0], c[0, 1] = (255, 0, 128), (0, 255, 255)
    write_png(str(tmp_path / "pic.png"), c)
    m = (rng.random((6, 8)) > 0.3).astype(np.uint8) * 255
    write_png(str(tmp_path / "pic_mask.png"), np.repeat(m[..., None], 3, axis=-1))
    g, gm = npr._read_normal_prior(str(tmp_path), "pic")
    assert np.array_equal(g, (2.0 * c.astype(np.float32) / 255.0 - 1.0).transpose(2, 0, 1)) and np.array_equal(gm, (m != 0).astype(np.uint8))
    assert tuple(g[:2, 0, 0]) == (1.0, -1.0) and abs(g[2, 0, 0] - (2.0 * 128 / 255 - 1)) <= 1e-6 and tuple(g[:, 0, 1]) == (-1.0, 1.0, 1.0)
    # frames on a hand-made camera: 90 degrees about the world y axis, camera-to-world R maps the camera's z to the world's x
    R = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
    cam = _cam("v", R)
    one = np.zeros((3, 1, 1), np.float32)
    one[:, 0, 0] = (0.25, 0.5, -0.75)
    assert np.array_equal(npr.to_camera_frame(one, "opencv", cam), one)
    assert tuple(npr.to_camera_frame(one, "opengl", cam)[:, 0, 0]) == (0.25, -0.5, 0.75)
    world_x = np.zeros((3, 1, 1), np.float32)
    world_x[0] = 1.0                                 # a normal along the world's x axis is the camera's z axis: away from it
    assert np.allclose(npr.to_camera_frame(world_x, "world", cam)[:, 0, 0], (0.0, 0.0, 1.0))
    assert np.allclose(npr.to_camera_frame(one, "world", cam)[:, 0, 0], R.T @ one[:, 0, 0])
    with pytest.raises(ValueError, match="normal_prior_frame"):
        npr.to_camera_frame(one, "blender", cam)
    # errors that name the file
    with pytest.raises(FileNotFoundError, match="view_b.npy"):
        npr.load_normal_priors(str(tmp_path), [_cam("view_b")], device="cpu")
    np.save(tmp_path / "view_b.npy", np.ones((6, 8), np.float32))
    with pytest.raises(ValueError, match="view_b.npy"):
        npr.load_normal_priors(str(tmp_path), [_cam("view_b")], device="cpu")
    write_png(str(tmp_path / "chw_mask.png"), np.zeros((5, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="chw_mask.png"):
        npr._read_normal_prior(str(tmp_path), "chw")


def test_term_window_and_mixed_sets():
    from binocular3dgs_amd._lib import B3gsError
    from binocular3dgs_amd.normal_prior import NormalTerm, check_prior_set
    t = NormalTerm(cos=0.1, from_iter=5, until_iter=9)
    assert t.enabled and not t.active(4) and t.active(5) and t.active(9) and not t.active(10)
    assert not NormalTerm().enabled and NormalTerm(l1=0.2).active(0)
    with pytest.raises(ValueError, match="alpha_min"):
        NormalTerm(cos=1.0, alpha_min=0.0)
    base = object()
    assert t.add(base, 7, argparse.Namespace(normal_prior=None), None) is base          # no prior on the view: no call
    assert t.add(base, 1, argparse.Namespace(normal_prior=torch.zeros(1)), None) is base  # outside the window: no call
    with_p, without = argparse.Namespace(normal_prior=torch.zeros(1), image_name="a"), argparse.Namespace(normal_prior=None, image_name="b")
    assert check_prior_set([with_p, with_p]) and not check_prior_set([without])
    with pytest.raises(B3gsError, match="all or none"):
        check_prior_set([with_p, without])


def test_shifted_cameras_carry_no_normal_prior():
    from binocular3dgs_amd.camera import Camera
    cam = Camera(np.eye(3), np.zeros(3), 0.9, 0.7, 8, 6, image=torch.zeros(3, 6, 8), normal_prior=torch.zeros(3, 6, 8),
                 normal_prior_mask=torch.ones(1, 6, 8, dtype=torch.uint8))
    assert cam.normal_prior is not None and cam.normal_prior_mask is not None
    s = cam.shifted(0.1)
    assert s.normal_prior is None and s.normal_prior_mask is None and cam.normal_prior is not None


# ---- the command line -------------------------------------------------------------------------------------------------------
def _args(*argv, **kw):
    from binocular3dgs_amd.train import parser
    args = parser().parse_args(["-s", "src", "-m", "out", *argv])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_check_args_rules_and_cfg_args():
    from binocular3dgs_amd.train import cfg_args_text, check_args, parser
    a = _args()
    check_args(a)
    assert (a.normal_priors, a.normal_prior_frame, a.normal_prior_cos, a.normal_prior_l1, a.normal_prior_from, a.normal_prior_until,
            a.normal_prior_alpha_min) == (None, "opencv", 0.0, 0.0, 0, None, 0.5)
    check_args(_args("--normal_priors", "normals", "--normal_prior_cos", "0.05"))
    check_args(_args("--normal_priors", "normals", "--normal_prior_l1", "0.05", "--step", "graph", "--depth_priors", "d",
                     "--depth_prior_weight", "0.1", "--exposure"))
    check_args(_args("--normal_priors", "normals", "--normal_prior_cos", "0.05", "--densify", "mcmc", "--cap_max", "1000"))
    with pytest.raises(ValueError, match="--normal_priors"):
        check_args(_args("--normal_prior_cos", "0.05"))
    with pytest.raises(ValueError, match="--normal_priors"):
        check_args(_args("--normal_prior_l1", "0.05"))
    for bad in (0.0, -0.5, math.nan):
        with pytest.raises(ValueError, match="normal_prior_alpha_min"):
            check_args(_args("--normal_priors", "normals", normal_prior_alpha_min=bad))
    with pytest.raises(SystemExit):
        parser().parse_args(["-s", "src", "--normal_prior_frame", "blender"])
    text = cfg_args_text(_args("--normal_priors", "normals", "--normal_prior_frame", "opengl", "--normal_prior_cos", "0.05",
                               "--normal_prior_until", "900"))
    for piece in ("normal_priors='normals'", "normal_prior_frame='opengl'", "normal_prior_cos=0.05", "normal_prior_l1=0.0",
                  "normal_prior_from=0", "normal_prior_until=900", "normal_prior_alpha_min=0.5"):
        assert piece in text, piece
