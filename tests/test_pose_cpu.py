"""CPU: the camera pose gradient (binocular3dgs_amd/pose.py, csrc/pose.hip) without a device.

  1. the SH generators: antisymmetric, expm(theta G) = edit.sh_rotation_matrices(R_k(theta)), the commutators close;
  2. the identity: the yardstick's six numbers (tests/pose_ref.py) from autograd's per-Gaussian gradients of
     oracle/dense_torch.py equal autograd's gradient with respect to the 6-vector that builds the camera matrices, to 1e-9
     relative L2 (float64; degrees 0..3; a scene with Gaussians at the 1.3 tan clamp and at the near plane); both mutants of
     the yardstick miss that bound by at least 1e-3;
  3. se3_exp / se3_log / moved_camera;
  4. the argument errors of b3gs_pose_gradient."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pose_ref

BOUND = 1e-9          # the issue's bound: a CPU check measured 1e-11, two orders are left for other seeds
MUTANT_MISS = 1e-3


def _rot(k, th):
    c, s = math.cos(th), math.sin(th)
    return [np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])][k]


# ---- 1. generators ---------------------------------------------------------------------------------------------------------------
def test_generators_are_antisymmetric_and_integrate_to_the_band_rotations():
    from scipy.linalg import expm
    from binocular3dgs_amd import edit, pose
    Gs = pose.sh_generators()
    for G, ref, n in zip(Gs, pose_ref.generators(), (3, 5, 7)):
        assert G.shape == (3, n, n) and G.dtype == np.float64
        assert np.array_equal(G, ref), "pose.py and the yardstick hold the same constants"
        for k in range(3):
            assert np.array_equal(G[k].T, -G[k])
    for k in range(3):
        for th in (0.3, 1.1, -2.0):
            D = edit.sh_rotation_matrices(_rot(k, th))
            for G, d in zip(Gs, D):
                err = np.abs(expm(th * G[k]) - d).max()
                assert err <= 1e-12, (k, th, G.shape, err)


def test_generator_commutators_close():
    """D is a homomorphism: Y(d)^T D(R1 R2) = Y(R2^T R1^T d)^T = Y(R1^T d)^T D(R2) = Y(d)^T D(R1) D(R2).  So the generators
    close with so(3)'s own sign: [G^x, G^y] = +G^z and cyclic, in every band."""
    from binocular3dgs_amd import pose
    for G in pose.sh_generators():
        for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            comm = G[a] @ G[b] - G[b] @ G[a]
            assert np.abs(comm - G[c]).max() <= 1e-14, (G.shape, a, b)


# ---- 2. the identity -------------------------------------------------------------------------------------------------------------
W, H = 32, 24


def _camera():
    from binocular3dgs_amd import synth
    return synth.synth_cameras(W, H, yaws=(5.0,))[0]


def _scene(P, K, seed, edge=False):
    """raw float64 parameters of P Gaussians in front of the camera; edge: a few means placed by hand past the 1.3 tan limit
    of the EWA Jacobian, next to the near plane, and behind it"""
    from binocular3dgs_amd import synth
    p = synth.synth_gaussians(P, seed, W, H, K=16)
    g = torch.Generator().manual_seed(seed + 5)
    raw = dict(xyz=p["xyz"].double(), f_dc=p["features_dc"].double(), f_rest=0.3 * torch.randn(P, 15, 3, generator=g, dtype=torch.float64),
               scaling=math.log(0.25) + 0.4 * torch.randn(P, 3, generator=g, dtype=torch.float64),
               rotation=p["rotation"].double() * (0.5 + 1.5 * torch.rand(P, 1, generator=g, dtype=torch.float64)),
               opacity=p["opacity"].double())
    raw["f_rest"] = raw["f_rest"][:, :K - 1].contiguous()
    if edge:
        cam = _camera()
        V = cam.world_view_transform.double()
        tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
        view = torch.tensor([[1.45 * tx * 3.0, 0.2 * ty * 3.0, 3.0], [-1.5 * tx * 2.5, 0.0, 2.5], [0.3 * tx * 4.0, 1.4 * ty * 4.0, 4.0],
                             [-1.38 * tx * 3.5, -1.42 * ty * 3.5, 3.5],                       # past the clamp: x, x, y, both
                             [0.02, 0.01, 0.23], [-0.03, 0.02, 0.26], [0.0, -0.02, 0.21],     # next to the near plane (0.2), visible
                             [0.01, 0.0, 0.15], [0.0, 0.01, -1.0]], dtype=torch.float64)     # culled
        raw["xyz"][:len(view)] = (view - V[3, :3]) @ torch.linalg.inv(V[:3, :3])
        raw["scaling"][:4] = math.log(0.8)             # wide enough to reach the image from outside it
        raw["scaling"][4:9] = math.log(0.01)
    return raw


def _weights(seed):
    g = torch.Generator().manual_seed(900 + seed)
    return tuple(torch.randn(c, H, W, generator=g, dtype=torch.float64) for c in (3, 1, 1))


def _render(leaf, cam_mats, deg):
    from oracle import dense_torch
    cam = _camera()
    viewmatrix, projmatrix, campos = cam_mats
    return dense_torch.render_dense(
        means3D=leaf["xyz"], opacities=torch.sigmoid(leaf["opacity"]), scales=torch.exp(leaf["scaling"]),
        rotations=torch.nn.functional.normalize(leaf["rotation"]), shs=torch.cat([leaf["f_dc"], leaf["f_rest"]], 1),
        viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos, bg=torch.tensor([0.1, 0.2, 0.3]), W=W, H=H,
        tanfovx=math.tan(cam.FoVx / 2), tanfovy=math.tan(cam.FoVy / 2), sh_degree=deg)


def _camera_from_twist(xi, pivot, cam=None):
    """(viewmatrix, projmatrix, campos) in float64 of the camera (default: the test camera) moved by the world twist xi about
    pivot: autograd's path from the 6-vector to the three things the renderer reads"""
    cam = _camera() if cam is None else cam
    V0 = cam.world_view_transform.detach().cpu().double()          # row-vector form: the transpose of W2C
    w, t = xi[:3], xi[3:]
    A = torch.stack([torch.stack([0 * w[0], -w[2], w[1], t[0]]), torch.stack([w[2], 0 * w[0], -w[0], t[1]]),
                     torch.stack([-w[1], w[0], 0 * w[0], t[2]]), torch.zeros(4, dtype=torch.float64)])
    c = torch.as_tensor(pivot, dtype=torch.float64)
    Tc, Tm = torch.eye(4, dtype=torch.float64), torch.eye(4, dtype=torch.float64)
    Tc[:3, 3], Tm[:3, 3] = c, -c
    M = Tc @ torch.linalg.matrix_exp(A) @ Tm        # the camera-to-world pose is multiplied by M on the left
    w2c = V0.t() @ torch.linalg.inv(M)
    viewmatrix = w2c.t()
    projmatrix = viewmatrix @ cam.projection_matrix.detach().cpu().double()
    centre = torch.linalg.inv(V0.t())[:3, 3]
    campos = (M @ torch.cat([centre, torch.ones(1, dtype=torch.float64)]))[:3]
    return viewmatrix, projmatrix, campos


def _both_sides(raw, deg, seed, pivot):
    """-> (autograd's gradient with respect to the camera twist [6], the per-Gaussian gradients, the render)"""
    wc, wd, wa = _weights(seed)
    leaf = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    out = _render(leaf, _camera_from_twist(xi, pivot), deg)
    loss = (out["color"] * wc).sum() + (out["depth"] * wd).sum() + (out["alpha"] * wa).sum()
    g = torch.autograd.grad(loss, [xi, leaf["xyz"], leaf["rotation"], leaf["f_rest"]], allow_unused=True)
    gf = torch.zeros_like(raw["f_rest"]) if g[3] is None else g[3]
    return g[0].numpy(), (g[1].numpy(), g[2].numpy(), gf.numpy()), out


def _yardstick(raw, grads, pivot, K, mut=None):
    deg = int(round(math.sqrt(K))) - 1
    s = pose_ref.pose_sums(raw["xyz"].numpy(), raw["rotation"].numpy(), raw["f_rest"].numpy(), [grads], None, pivot, deg, mut)[0]
    return -s                                       # camera = - scene


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("deg,K", [(3, 16), (0, 16), (1, 16), (2, 16), (2, 9), (1, 4)])
def test_identity_against_autograd_through_the_camera(deg, K):
    pivot = np.array([0.3, -0.2, 5.0])
    raw = _scene(40, K, seed=deg)
    want, grads, out = _both_sides(raw, deg, deg, pivot)
    assert int((out["radii"] > 0).sum()) >= 20 and np.linalg.norm(want) > 0
    got = _yardstick(raw, grads, pivot, K)
    err = _rel(got, want)
    parts = pose_ref.row_parts(raw["xyz"].numpy(), raw["rotation"].numpy(), raw["f_rest"].numpy(), *grads, pivot, int(round(math.sqrt(K))) - 1)
    size = [float(np.abs(p).sum()) for p in parts]
    print(f"degree {deg} K {K}: rel L2 {err:.2e}; sum |cross| {size[0]:.2e} |h/2| {0.5 * size[1]:.2e} |s| {size[2]:.2e}")
    assert err <= BOUND
    miss = {m: _rel(_yardstick(raw, grads, pivot, K, m), want) for m in ("no_sh", "quat_right")}
    print(f"  mutants: {miss}")
    assert miss["quat_right"] >= BOUND + MUTANT_MISS
    if deg > 0:
        assert miss["no_sh"] >= BOUND + MUTANT_MISS


def test_identity_with_clamped_and_near_plane_gaussians():
    from binocular3dgs_amd import pose
    cam = _camera()
    pivot = pose.camera_centre(cam)                 # the default pivot of camera_gradient
    raw = _scene(40, 16, seed=11, edge=True)
    want, grads, out = _both_sides(raw, 3, 11, pivot)
    V = cam.world_view_transform.double()
    pv = torch.cat([raw["xyz"], torch.ones(40, 1, dtype=torch.float64)], 1) @ V
    tx, ty = math.tan(cam.FoVx / 2), math.tan(cam.FoVy / 2)
    clamped = ((pv[:, 0] / pv[:, 2]).abs() > 1.3 * tx) | ((pv[:, 1] / pv[:, 2]).abs() > 1.3 * ty)
    touched = torch.from_numpy(np.abs(grads[0]).sum(1) > 0)
    near = (pv[:, 2] > 0.2) & (pv[:, 2] < 0.3)
    culled = pv[:, 2] <= 0.2
    assert int((clamped & touched & (pv[:, 2] > 0.2)).sum()) >= 3, "Gaussians past the 1.3 tan limit take part in the gradient"
    assert int((near & touched).sum()) >= 2, "Gaussians next to the near plane take part"
    assert int(culled.sum()) >= 2 and not bool(touched[culled].any()) and bool((out["radii"][culled] == 0).all())
    err = _rel(_yardstick(raw, grads, pivot, 16), want)
    print(f"edge scene: rel L2 {err:.2e}")
    assert err <= BOUND
    for m in ("no_sh", "quat_right"):
        assert _rel(_yardstick(raw, grads, pivot, 16, m), want) >= BOUND + MUTANT_MISS, m


def test_yardstick_chunking_follows_the_stated_rule():
    assert [pose_ref.nblocks(P) for P in (1, 1024, 1025, 2048, 2049, 1023 * 1024, 1023 * 1024 + 1, 5_000_000)] == [1, 1, 2, 2, 3, 1023, 1024, 1024]
    g = np.random.default_rng(0)
    t = g.standard_normal((2500, 6))
    assert np.allclose(pose_ref.fold(t), t.sum(0), rtol=1e-12, atol=1e-12)
    skip = g.uniform(size=2500) < 0.5
    assert np.allclose(pose_ref.fold(t, skip), t[~skip].sum(0), rtol=1e-12, atol=1e-12)
    assert np.array_equal(pose_ref.fold(np.zeros((0, 6))), np.zeros(6))


# ---- 3. Lie-group helpers --------------------------------------------------------------------------------------------------------
def test_se3_round_trip_and_series():
    from scipy.linalg import expm
    from binocular3dgs_amd import pose
    g = np.random.default_rng(3)
    for scale in (0.0, 1e-9, 1e-5, 9e-5, 1.1e-4, 1e-2, 1.0, 3.0):
        xi = np.concatenate([g.standard_normal(3) * scale / math.sqrt(3), g.standard_normal(3)])
        T = pose.se3_exp(xi)
        A = np.zeros((4, 4))
        A[:3, :3], A[:3, 3] = pose._hat(xi[:3]), xi[3:]
        assert np.abs(T - expm(A)).max() <= 1e-13, scale
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-14
        assert np.abs(pose.se3_log(T) - xi).max() <= 1e-11 * max(1.0, np.abs(xi).max()), scale
    assert np.array_equal(pose.se3_exp(np.zeros(6)), np.eye(4))
    axis = np.array([0.6, 0.0, 0.8])
    xi = np.concatenate([axis * (math.pi - 1e-9), [0.1, 0.2, 0.3]])        # next to pi
    assert np.abs(pose.se3_log(pose.se3_exp(xi)) - xi).max() <= 1e-6


def test_moved_camera_identity_and_inverse():
    from binocular3dgs_amd import pose, synth
    for cam in synth.synth_cameras(W, H, yaws=(0.0, 7.0, -13.0)):
        cam.original_image = torch.rand(3, H, W)
        same = pose.moved_camera(cam, np.zeros(6), [0.3, 0.1, 6.0])
        for k in ("world_view_transform", "projection_matrix", "full_proj_transform", "camera_center"):
            assert torch.equal(getattr(same, k), getattr(cam, k)), k
        assert same.original_image is cam.original_image and same is not cam
        xi = np.array([0.02, -0.03, 0.01, 0.05, -0.02, 0.04])
        pivot = np.array([0.3, 0.1, 6.0])
        there = pose.moved_camera(cam, xi, pivot)
        back = pose.moved_camera(there, -xi, pivot)
        assert np.abs(back.R - cam.R).max() <= 1e-12 and np.abs(back.T - cam.T).max() <= 1e-12
        # the pose is multiplied on the LEFT by the twist about the pivot
        M = pose.twist_matrix(xi, pivot)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = cam.R, pose.camera_centre(cam)
        want = M @ c2w
        assert np.abs(there.R - want[:3, :3]).max() <= 1e-14 and np.abs(pose.camera_centre(there) - want[:3, 3]).max() <= 1e-13
        assert float((there.camera_center.double() - torch.from_numpy(want[:3, 3])).abs().max()) <= 1e-5


# ---- 4. argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors_without_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    ERR_ARG = -1
    one = (C.c_void_p * 8)(*([8] * 8))              # never dereferenced: every call below fails its checks first
    piv = (C.c_double * 3)(0.0, 0.0, 0.0)
    ok = dict(P=10, deg=3, V=1, xyz=8, rot=8, rest=8, gx=one, gr=one, gf=one, skip=None, pivot=piv, out=8, ws=8)

    def call(**over):
        a = dict(ok, **over)
        return L.b3gs_pose_gradient(a["P"], a["deg"], a["V"], a["xyz"], a["rot"], a["rest"], a["gx"], a["gr"], a["gf"], a["skip"],
                                    a["pivot"], a["out"], a["ws"], None)
    for bad in (dict(V=0), dict(V=9), dict(V=-1), dict(deg=-1), dict(deg=4), dict(P=-1), dict(xyz=None), dict(rot=None), dict(rest=None),
                dict(gx=None), dict(gr=None), dict(gf=None), dict(pivot=None), dict(out=None), dict(ws=None),
                dict(pivot=(C.c_double * 3)(0.0, math.nan, 0.0)), dict(pivot=(C.c_double * 3)(math.inf, 0.0, 0.0))):
        assert call(**bad) == ERR_ARG, bad
        assert b"b3gs_pose_gradient" in L.b3gs_last_error()
    nul = (C.c_void_p * 8)(8, None, 8, 8, 8, 8, 8, 8)
    assert call(V=2, gx=nul) == ERR_ARG and call(V=2, gr=nul) == ERR_ARG and call(V=2, gf=nul) == ERR_ARG
    assert L.b3gs_pose_gradient_workspace_bytes(0, 1) == 0 and L.b3gs_pose_gradient_workspace_bytes(10, 9) == 0
    assert L.b3gs_pose_gradient_workspace_bytes(1, 1) == 256
    assert L.b3gs_pose_gradient_workspace_bytes(2_000_000, 8) == 8 * 1024 * 6 * 8
