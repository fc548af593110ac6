"""TSDF fusion and marching tetrahedra on the device (csrc/mesh.hip, binocular3dgs_amd/mesh.py) against the numpy restatement of
tests/mesh_ref.py.  The integration uses +, -, x, /, min and round-to-nearest only, one correctly rounded float32 operation per
statement on both sides, and so do the vertex positions and colours: everything is compared bit for bit."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
DIMS, ORIGIN, VOXEL, TRUNC = (20, 17, 13), (-1.25, -1.0625, 2.0), 0.125, 0.5      # three sizes, none a multiple of anything
W, H, NCAM = 40, 30, 9
CENTRE = np.array([0.0, 0.0, 2.8])


def _cameras():
    """9 cameras in front of the box, turned about y; the last two stand far to the side and see only a part of it."""
    rows, poses = np.zeros((NCAM, 14), F), []
    for k in range(NCAM):
        yaw = 0.06 * (k - 4)
        centre = np.array([0.25 * (k - 4), 0.1 * (k % 3 - 1), 0.0])
        if k >= 7:
            centre[0] = 1.6 if k == 7 else -1.7
        R = np.array([[math.cos(yaw), 0.0, -math.sin(yaw)], [0.0, 1.0, 0.0], [math.sin(yaw), 0.0, math.cos(yaw)]])   # world -> camera
        t = -R @ centre
        rows[k, :9], rows[k, 9:12], rows[k, 12], rows[k, 13] = R.reshape(9), t, 20.0 + k, 21.0 - 0.5 * k
        poses.append((R, centre))
    return rows, poses


def _images(scene, rows, poses, seed):
    """Analytic z-depth of a tilted plane or a sphere per camera (float64, then float32), alpha 1 / 0.8 / 0.3 in bands (0.3 is
    below alpha_min), the renderer's convention depth = z * alpha, seeded colours."""
    rng = np.random.default_rng(seed)
    depths, alphas, colours = [], [], []
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    for k, (R, centre) in enumerate(poses):
        fx, fy = float(rows[k, 12]), float(rows[k, 13])
        dc = np.stack([(u - (0.5 * W - 0.5)) / fx, (v - (0.5 * H - 0.5)) / fy, np.ones_like(u)], axis=-1)
        dw = dc @ R                                             # R^T d per pixel
        if scene == "plane":
            n = np.array([0.2, 0.1, 1.0])
            z = (n @ CENTRE - n @ centre) / (dw @ n)
            hit = z > 0
        else:
            oc = centre - CENTRE
            a, b, c = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - 0.6 ** 2
            disc = b * b - 4 * a * c
            hit = disc > 0
            z = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
        alpha = np.where(hit, 1.0, 0.0)
        alpha[:, 5 + k:9 + k] *= 0.3
        alpha[20:24, :] *= 0.8
        alpha = alpha.astype(F)
        depths.append((np.where(hit, z, 0.0).astype(F) * alpha).astype(F))
        alphas.append(alpha)
        colours.append(rng.uniform(size=(3, H, W)).astype(F))
    return depths, alphas, colours


@pytest.fixture(scope="module")
def scenes():
    """Per scene: the camera table, the images (host and device) and the yardstick's volume after 1, 3, 8 and 9 views."""
    rows, poses = _cameras()
    out = {}
    for seed, scene in enumerate(("plane", "sphere")):
        depths, alphas, colours = _images(scene, rows, poses, seed)
        refs = {}
        for n in (1, 3, 8, 9):
            vol = mr.new_volume(DIMS, ORIGIN, VOXEL)
            refs[n] = mr.integrate(vol, rows[:n], depths[:n], alphas[:n], colours[:n], TRUNC)
        w9 = refs[9]["weight"]
        assert w9.max() >= 7 and (w9 == 0).any() and (refs[9]["tsdf"][w9 > 0] == 1.0).any() and (refs[9]["tsdf"] < 0).any()
        assert (refs[9]["weight"] != refs[8]["weight"]).any()
        dev = [[torch.from_numpy(a).to(DEV) for a in arrs] for arrs in (depths, alphas, colours)]
        out[scene] = {"cams": rows, "dev": dev, "refs": refs}
    return out


def _device_volume(ref=None, dims=DIMS, origin=ORIGIN, voxel=VOXEL, truncation=TRUNC):
    from binocular3dgs_amd.mesh import TsdfVolume
    if ref is not None:
        nz, ny, nx = ref["tsdf"].shape
        dims, origin, voxel = (nx, ny, nz), ref["origin"], ref["voxel"]
    vol = TsdfVolume(origin, [o + d * voxel for o, d in zip(origin, dims)], voxel, truncation, device=DEV)
    assert vol.dims == tuple(dims)
    if ref is not None:
        vol.tsdf.copy_(torch.from_numpy(ref["tsdf"]))
        vol.weight.copy_(torch.from_numpy(ref["weight"]))
        vol.rgb.copy_(torch.from_numpy(ref["rgb"]))
    return vol


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_volume(vol, ref):
    for name in ("tsdf", "weight", "rgb"):
        got, want = _bits(getattr(vol, name)), _bits(ref[name])
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} of {got.size} words differ"


def _assert_mesh(got, want):
    (v, c, f), (rv, rc, rf) = got, want
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32
    assert tuple(v.shape) == rv.shape and tuple(f.shape) == rf.shape and tuple(c.shape) == rc.shape
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(_bits(v), _bits(rv))
    assert np.array_equal(c.cpu().numpy(), rc)


# ---- integration -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 8, 9])
@pytest.mark.parametrize("scene", ["plane", "sphere"])
def test_integration_matches_the_yardstick(scenes, scene, n):
    s = scenes[scene]
    vol = _device_volume()
    vol.integrate(s["cams"][:n], *[imgs[:n] for imgs in s["dev"]])        # 9: one launch of 8 and one of 1
    _assert_volume(vol, s["refs"][n])


def test_two_batches_equal_one_pass(scenes):
    s = scenes["sphere"]
    vol = _device_volume()
    vol.integrate(s["cams"][:3], *[imgs[:3] for imgs in s["dev"]])
    _assert_volume(vol, s["refs"][3])
    vol.integrate(s["cams"][3:], *[imgs[3:] for imgs in s["dev"]])
    _assert_volume(vol, s["refs"][9])
    vol.reset()
    assert float(vol.weight.max()) == 0.0 and float(vol.tsdf.min()) == 1.0 and float(vol.rgb.abs().max()) == 0.0


# ---- extraction --------------------------------------------------------------------------------------------------------
def _open_sphere():
    vol = mr.sphere_volume()
    vol["weight"][:, :, vol["weight"].shape[2] // 2:] = 0.0          # the right half was never observed: an open boundary
    return vol


VOLUMES = {"sphere": mr.sphere_volume, "random": mr.random_volume, "open": _open_sphere,
           # 70 x 66 x 116 voxels = 2094 blocks of 256: three chunks of the 1024-wide scan
           "three_scan_chunks": lambda: mr.sphere_volume((70, 66, 116), 25.0)}


@pytest.mark.parametrize("name", list(VOLUMES))
def test_extraction_matches_the_yardstick(name):
    ref = VOLUMES[name]()
    want = mr.extract(ref)
    assert len(want[2]) > 0
    got = _device_volume(ref).extract()
    _assert_mesh(got, want)
    v, f = got[0].cpu().numpy(), got[2].cpu().numpy()
    _, uses = mr.edge_uses(f)
    if name == "sphere":
        assert (uses == 2).all() and mr.euler_characteristic(len(v), f) == 2
        volume, exact = mr.signed_volume(v, f), 4.0 / 3.0 * math.pi * 6.0 ** 3
        assert volume > 0 and abs(volume - exact) / exact <= 2 * 0.013904          # (the bound of tests/test_mesh_cpu.py)
    if name == "open":
        assert (uses == 1).any() and uses.max() == 2
    if name == "three_scan_chunks":
        assert ref["tsdf"].size > 2 * 1024 * 256


def test_all_positive_volume_gives_an_empty_mesh():
    vol = _device_volume()
    assert vol.count().tolist() == [0, 0]
    v, c, f = vol.extract()
    assert tuple(v.shape) == (0, 3) and tuple(c.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    assert v.dtype == torch.float32 and c.dtype == torch.uint8 and f.dtype == torch.int32 and v.is_cuda


def test_min_weight_selects_the_cells(scenes):
    s = scenes["sphere"]
    vol = _device_volume()
    vol.integrate(s["cams"], *s["dev"])
    want1, want4 = mr.extract(s["refs"][9], 1.0), mr.extract(s["refs"][9], 4.0)
    assert 0 < len(want4[2]) < len(want1[2])
    _assert_mesh(vol.extract(1.0), want1)
    _assert_mesh(vol.extract(4.0), want4)


def test_integrate_and_count_replay_from_a_graph(scenes):
    s = scenes["plane"]
    vol = _device_volume()
    args = (s["cams"][:3], *[imgs[:3] for imgs in s["dev"]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up: the workspace exists before the capture
        vol.integrate(*args)
        vol.count()
    torch.cuda.current_stream().wait_stream(side)
    vol.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        vol.integrate(*args)
        totals = vol.count()
    want = mr.extract(s["refs"][3])
    for _ in range(2):
        vol.reset()
        totals.zero_()
        graph.replay()
        _assert_volume(vol, s["refs"][3])
        assert totals.tolist() == [len(want[0]), len(want[2])]


# ---- end to end --------------------------------------------------------------------------------------------------------
def _shell_model(tmp_path, P=400):
    """Gaussians on a sphere shell of radius 1 around (0, 0, 6), saved as a trained model folder with 6 cameras around it
    (cameras.json); -> (model path, model, cameras), both read back from the folder."""
    from binocular3dgs_amd.camera import look_at_orbit
    from binocular3dgs_amd.extract_mesh import cameras_from_json
    from binocular3dgs_amd.gaussian_model import GaussianModel, inverse_sigmoid
    g = torch.Generator().manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1)
    xyz = d + torch.tensor([0.0, 0.0, 6.0])
    model = GaussianModel.from_tensors(xyz, torch.rand(P, 1, 3, generator=g), torch.zeros(P, 3, 3), torch.full((P, 3), math.log(0.12)),
                                       torch.randn(P, 4, generator=g), inverse_sigmoid(torch.full((P, 1), 0.95)), sh_degree=1,
                                       device=DEV, requires_grad=False)
    path = str(tmp_path / "model")
    model.save_ply(os.path.join(path, "point_cloud", "iteration_7", "point_cloud.ply"))
    entries = []
    for k in range(6):
        R, T = look_at_orbit(60.0 * k)
        entries.append({"id": k, "img_name": f"v{k}", "width": 64, "height": 48, "position": (-R @ T).tolist(),
                        "rotation": [row.tolist() for row in R], "fx": 110.0, "fy": 110.0})
    with open(os.path.join(path, "cameras.json"), "w") as fp:
        json.dump(entries, fp)
    with open(os.path.join(path, "cfg_args"), "w") as fp:
        fp.write("Namespace(sh_degree=1, white_background=False, source_path='')")
    loaded = GaussianModel(1)
    loaded.load_ply(os.path.join(path, "point_cloud", "iteration_7", "point_cloud.ply"))
    return path, loaded, cameras_from_json(os.path.join(path, "cameras.json"))


def test_fuse_model_and_the_command_line(tmp_path, capsys):
    from binocular3dgs_amd import extract_mesh, mesh
    from binocular3dgs_amd.evaluate import _batches
    path, model, cams = _shell_model(tmp_path)
    bg = torch.zeros(3, device=DEV)
    v, c, f, vol = mesh.fuse_model(model, cams, bg, resolution=24, return_volume=True)
    assert f.shape[0] > 200 and max(vol.dims) <= 24 + 9 and float(vol.weight.max()) >= 2
    # the yardstick, fed the same rendered tensors
    table = mesh.camera_table(cams)
    ref = mr.new_volume(vol.dims, vol.origin, vol.voxel_size)
    for idx, outs in _batches(model, cams, bg, 8, full=True):
        host = [[o[key].cpu().numpy() for o in outs] for key in ("rendered_depth", "rendered_alpha", "render")]
        mr.integrate(ref, table[idx], host[0], host[1], host[2], vol.truncation)
    _assert_volume(vol, ref)
    _assert_mesh((v, c, f), mr.extract(ref))
    # the command line on the saved model
    assert extract_mesh.main(["-m", path, "--views", "all", "--resolution", "24"]) == 0
    out = os.path.join(path, "mesh", "iteration_7", "mesh.ply")
    assert f"{v.shape[0]} vertices, {f.shape[0]} triangles" in capsys.readouterr().out
    pv, pc, pf = mesh.read_mesh_ply(out)
    assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(pc, c.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy())
