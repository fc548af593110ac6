"""CPU: the host half of binocular3dgs_amd/edit.py and the yardstick tests/edit_ref.py.  The SH rotation matrices have their
defining property at fp64 round-off; the float64 dense oracle renders the yardstick-transformed model from the transformed
cameras as it renders the original (d_ref), and sees both mutants of the yardstick; orient_from_cameras, merge, Similarity and
the yardstick's ICP loop do what they say."""
import math

import numpy as np
import pytest
import torch

import edit_ref
from binocular3dgs_amd import edit


def _rotations():
    Rs = [edit_ref.random_similarity(100 + k)[0] for k in range(20)] + [np.eye(3)]
    for ax in range(3):
        a = np.zeros(3)
        a[ax] = 1.0
        Rs.append(edit._rotation_about(a, 90.0))
    return Rs


def test_sh_rotation_matrices_have_their_defining_property():
    g = np.random.default_rng(5)
    d = g.standard_normal((1000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Rs = _rotations()
    e_prop = e_orth = e_hom = 0.0
    for i, R in enumerate(Rs):
        D = edit.sh_rotation_matrices(R)
        Y, Yr = edit_ref.sh_basis(d), edit_ref.sh_basis(d @ R)          # (d @ R: R^T d, row by row)
        R2 = Rs[(i + 7) % len(Rs)]
        D2, D12 = edit.sh_rotation_matrices(R2), edit.sh_rotation_matrices(R @ R2)
        for l in range(3):
            e_prop = max(e_prop, np.abs(Y[l] @ D[l] - Yr[l]).max())
            e_orth = max(e_orth, np.abs(D[l].T @ D[l] - np.eye(2 * l + 3)).max())
            e_hom = max(e_hom, np.abs(D12[l] - D[l] @ D2[l]).max())
    print(f"sh_rotation_matrices: |Y D - Y(R^T d)| {e_prop:.3e}  |D^T D - I| {e_orth:.3e}  |D(R1 R2) - D(R1) D(R2)| {e_hom:.3e}")
    assert e_prop <= 1e-12 and e_orth <= 1e-12 and e_hom <= 1e-12
    I1, I2, I3 = edit.sh_rotation_matrices(np.eye(3))
    assert np.abs(I1 - np.eye(3)).max() <= 1e-14 and np.abs(I2 - np.eye(5)).max() <= 1e-14 and np.abs(I3 - np.eye(7)).max() <= 1e-14


def test_oracle_renders_the_transformed_model_alike_and_sees_the_mutants():
    d_ref = edit_ref.d_of(None)
    d_sh, d_q = edit_ref.d_of("sh_identity"), edit_ref.d_of("quat_right")
    print(f"d_ref {d_ref:.3e}  sh_identity {d_sh:.3e}  quat_right {d_q:.3e}")
    assert d_ref < 1e-4
    assert d_sh > 10.0 * d_ref and d_q > 10.0 * d_ref


def test_device_words_belong_together():
    R, t, s = edit_ref.random_similarity(3)
    T = edit.Similarity(R, t, s)
    w = edit_ref.unpack(T.device_words())
    qw, qx, qy, qz = w["q"]
    Rq = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                   [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                   [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])
    assert np.abs(Rq - R).max() <= 1e-14 and abs(w["ln_s"] - math.log(s)) == 0.0 and w["s"] == s
    assert np.array_equal(edit_ref.quaternion_of(R), T.quaternion())
    for Rax in _rotations():                                  # every pivot of the quaternion extraction
        q = edit.Similarity(Rax).quaternion()
        assert abs((q * q).sum() - 1.0) <= 1e-15 and q[0] >= 0.0


def test_similarity_algebra_and_refusals():
    A, B = edit.Similarity(*edit_ref.random_similarity(1)), edit.Similarity(*edit_ref.random_similarity(2))
    x = np.random.default_rng(0).standard_normal((10, 3))
    assert np.abs(A.compose(B).apply(x) - A.apply(B.apply(x))).max() <= 1e-12
    assert np.abs(A.inverse().apply(A.apply(x)) - x).max() <= 1e-12
    C = edit.Similarity.from_matrix(A.matrix())
    assert np.abs(C.R - A.R).max() <= 1e-12 and np.abs(C.t - A.t).max() == 0.0 and abs(C.s - A.s) <= 1e-12
    with pytest.raises(ValueError, match="reflection"):
        edit.Similarity(np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="reflection"):
        edit.Similarity.from_matrix(np.diag([1.0, -1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="non-uniform"):
        edit.Similarity.from_matrix(np.diag([1.0, 2.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="orthogonal"):
        edit.Similarity(np.diag([1.0, 2.0, 0.5]))
    with pytest.raises(ValueError, match="non-finite"):
        edit.Similarity(t=[0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="positive"):
        edit.Similarity(s=0.0)


def test_orient_from_cameras_recovers_a_tilted_ring():
    from binocular3dgs_amd.camera import Camera
    tilt = edit._rotation_about([0.3, -0.5, 0.2], 37.0)      # the ring's frame in the world
    focus = np.array([0.7, -1.1, 2.3])
    cams = []
    for k in range(8):
        a = 2.0 * math.pi * k / 8
        c_local = np.array([3.0 * math.cos(a), 3.0 * math.sin(a), 1.0])       # on a ring 1 above the focus plane, looking at the focus
        fwd = -c_local / np.linalg.norm(c_local)
        right = np.cross(fwd, [0.0, 0.0, 1.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        Rc = tilt @ np.stack([right, down, fwd], axis=1)                       # camera-to-world: columns = x (right), y (down), z
        C = focus + tilt @ c_local
        cams.append(Camera(Rc, -Rc.T @ C, 1.0, 0.8, 32, 24))
    T = edit.orient_from_cameras(cams)
    assert np.abs(T.R @ tilt[:, 2] - np.array([0.0, 0.0, 1.0])).max() <= 1e-12      # up -> +z
    assert np.abs(T.apply(focus[None])).max() <= 1e-12                              # the focus -> origin
    assert abs(T.s - 1.0) == 0.0
    r0 = T.R @ cams[0].R[:, 0]
    assert abs(r0[1]) <= 1e-12 and abs(r0[2]) <= 1e-12 and r0[0] > 0.0              # x: the first camera's right vector
    Tu = edit.orient_from_cameras(cams, unit_radius=True)
    assert abs(np.mean([np.linalg.norm(Tu.apply((-c.R @ c.T)[None])) for c in cams]) - 1.0) <= 1e-12
    par = [Camera(np.eye(3), -np.array([float(k), 0.0, 0.0]), 1.0, 0.8, 32, 24) for k in range(3)]
    with pytest.raises(ValueError, match="parallel"):
        edit.orient_from_cameras(par)


def test_transform_cameras_scales_view_coordinates():
    case = edit_ref.render_case()
    T = case["T"]
    x = case["model"]._xyz.numpy().astype(np.float64)[:50]
    for c0, c1 in zip(case["cameras"], case["moved_cameras"]):
        v0 = np.c_[x, np.ones(len(x))] @ c0.world_view_transform.numpy().astype(np.float64)
        v1 = np.c_[T.apply(x), np.ones(len(x))] @ c1.world_view_transform.numpy().astype(np.float64)
        assert np.abs(v1[:, :3] - T.s * v0[:, :3]).max() <= 2e-5 * T.s
        assert c1.znear == c0.znear * T.s and c1.zfar == c0.zfar * T.s


def test_merge_pads_degrees():
    from binocular3dgs_amd import synth
    a = synth.synth_model(5, seed=1, K=4, requires_grad=False)       # degree 1
    b = synth.synth_model(7, seed=2, K=16, requires_grad=False)      # degree 3
    m = edit.merge([a, b])
    assert m._xyz.shape == (12, 3) and m._features_rest.shape == (12, 15, 3) and m.max_sh_degree == 3
    assert torch.equal(m._features_rest[:5, :3], a._features_rest) and torch.count_nonzero(m._features_rest[:5, 3:]) == 0
    assert torch.equal(m._features_rest[5:], b._features_rest) and torch.equal(m._xyz[5:], b._xyz) and torch.equal(m._opacity[:5], a._opacity)


def test_yardstick_transform_identity_and_selection_edges():
    g = np.random.default_rng(2)
    xyz, rot, sc, rest = (g.standard_normal(s).astype(np.float32) for s in ((9, 3), (9, 4), (9, 3), (9, 15, 3)))
    out = edit_ref.transform(xyz, rot, sc, rest, edit.Similarity().device_words(), 3)
    for a, b in zip(out, (xyz, rot, sc, rest)):
        assert np.array_equal(a, b)
    M = np.c_[np.eye(3), np.zeros(3)]
    pts = np.array([[1.0, 0, 0], [np.nextafter(np.float32(1), np.float32(2)), 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    keep, _ = edit_ref.select(pts, None, None, box=(M, np.ones(3)))
    assert keep.tolist() == [True, False, False, True]
    keep, _ = edit_ref.select(pts, None, None, sphere=(np.zeros(3), 1.0))
    assert keep.tolist() == [True, False, False, True]


def test_yardstick_icp_recovers_a_small_similarity():
    src = edit_ref.surface_points(400, seed=3)
    R = edit._rotation_about([0.2, 1.0, -0.4], 5.0)
    t, s = np.array([0.03, -0.02, 0.025]), 1.02
    dst = (s * (src.astype(np.float64) @ R.T) + t).astype(np.float32)
    (Re, te, se), hist = edit_ref.register(src, dst, max_dist=0.5, iterations=60, with_scale=True)
    print(f"icp: {len(hist)} iterations, pairs {hist[-1][0]}, rms {hist[-1][1]:.3e}, |R - R*| {np.abs(Re - R).max():.3e}")
    assert hist[-1][0] == 400
    assert np.abs(Re - R).max() <= 1e-6 and abs(se - s) <= 1e-6 and np.abs(te - t).max() <= 1e-6
    # the host math of edit.py is the yardstick's, bit for bit
    idx = np.arange(400, dtype=np.int32)
    dist = np.zeros(400, np.float32)
    oa, ob = np.zeros(3), np.ones(3) * 0.1
    sums = edit_ref.similarity_sums(src, dst, idx, dist, 1.0, None, oa, ob)
    assert sums.shape == (18,)
    Tm, rms = edit.umeyama(sums, oa, ob, True)
    Ry, ty, sy, rmsy = edit_ref.umeyama(sums, oa, ob, True)
    assert np.array_equal(Tm.R, Ry) and np.array_equal(Tm.t, ty) and Tm.s == sy and rms == rmsy
    assert np.abs(Ry - R).max() <= 1e-6


def _colmap_folder(root, with_bin_points=True):
    """a tiny COLMAP dataset folder: 3 PINHOLE images with 2-D points, points3D.txt, an image file, poses_bounds.npy"""
    import os
    from binocular3dgs_amd import undistort as U
    sp = os.path.join(root, "sparse/0")
    os.makedirs(sp)
    os.makedirs(os.path.join(root, "images"))
    g = np.random.default_rng(4)
    images = {}
    for k in range(3):
        R, t, _ = edit_ref.random_similarity(50 + k)
        images[k + 1] = (edit_ref.quaternion_of(R), t, 1, f"im{k}.png", g.uniform(0, 30, (4, 2)), np.arange(4, dtype=np.int64))
        open(os.path.join(root, "images", f"im{k}.png"), "wb").write(b"x")
    U.write_cameras_bin(os.path.join(sp, "cameras.bin"), {1: ("PINHOLE", 32, 24, (20.0, 21.0, 16.0, 12.0))})
    U.write_images_bin(os.path.join(sp, "images.bin"), images)
    pts = g.standard_normal((6, 3))
    with open(os.path.join(sp, "points3D.txt"), "w") as fp:
        fp.write("# comment\n")
        for i, p in enumerate(pts):
            fp.write(f"{i + 1} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {10 * i} {20 * i} {255 - i} 0.5 1 0\n")
    from binocular3dgs_amd.dataset_readers import quaternion_to_rotation
    pb = []
    for k in range(3):                                      # the same poses as camera-to-world blocks in LLFF's axis order
        R, t = quaternion_to_rotation(images[k + 1][0]), images[k + 1][1]
        c2w = np.concatenate([R.T, (-R.T @ t)[:, None]], 1)
        blk = np.concatenate([np.stack([c2w[:, 1], c2w[:, 0], -c2w[:, 2], c2w[:, 3]], 1), np.array([[24.0], [32.0], [20.0]])], 1)
        pb.append(np.concatenate([blk.ravel(), [1.5 + k, 6.0 + k]]))
    np.save(os.path.join(root, "poses_bounds.npy"), np.array(pb))
    open(os.path.join(root, "notes.txt"), "w").write("kept")
    open(os.path.join(sp, "project.ini"), "w").write("kept")
    return images, pts


def test_transform_dataset_moves_poses_and_points_together(tmp_path):
    import os
    from binocular3dgs_amd import dataset_readers as dr, undistort as U
    from binocular3dgs_amd.init_points import fetch_point_cloud
    src, dst = str(tmp_path / "src"), str(tmp_path / "dst")
    images, pts = _colmap_folder(src)
    T = edit.Similarity(*edit_ref.random_similarity(9))
    info = edit.transform_dataset(src, dst, T)
    assert info["images"] == 3 and info["points"] == 6 and info["poses_bounds"] == 3
    back = U.read_images_bin_full(os.path.join(dst, "sparse/0/images.bin"))
    X = np.random.default_rng(1).standard_normal((20, 3))
    for iid, rec in images.items():
        q, t, cid, name, xys, pid = back[iid]
        assert (cid, name) == (rec[2], rec[3]) and np.array_equal(xys, rec[4]) and np.array_equal(pid, rec[5]) and q[0] >= 0.0
        old = X @ dr.quaternion_to_rotation(rec[0]).T + rec[1]
        new = T.apply(X) @ dr.quaternion_to_rotation(q).T + t
        assert np.abs(new - T.s * old).max() <= 1e-12 * max(1.0, T.s)              # x_cam' = s x_cam: the same pixels
    assert dr.read_cameras_bin(os.path.join(dst, "sparse/0/cameras.bin"))[1][0] == "PINHOLE"
    got, rgb = fetch_point_cloud(os.path.join(dst, "sparse/0/points3D.ply"))
    assert np.array_equal(got, T.apply(pts).astype(np.float32))
    assert np.array_equal(np.rint(rgb * 255.0)[:, 0], 10.0 * np.arange(6))
    names = sorted(os.listdir(os.path.join(dst, "sparse/0")))
    assert names == ["cameras.bin", "images.bin", "points3D.ply", "project.ini"]       # no unmoved points, no stale text files
    assert sorted(os.listdir(dst)) == ["images", "notes.txt", "poses_bounds.npy", "sparse"] and sorted(os.listdir(os.path.join(dst, "images"))) == ["im0.png", "im1.png", "im2.png"]
    # the reader sees the moved cameras: centres C' = s R C + t
    cams0, cams1 = dr._colmap_cameras(src, "images"), dr._colmap_cameras(dst, "images")
    for a, b in zip(cams0, cams1):
        assert np.abs((-b.R @ b.T) - T.apply((-a.R @ a.T)[None])[0]).max() <= 1e-12 * max(1.0, T.s) * 10
    # poses_bounds.npy holds the same moved cameras as images.bin: axes and centre of every block, both bounds times s, hwf kept
    pb0, pb1 = np.load(os.path.join(src, "poses_bounds.npy")), np.load(os.path.join(dst, "poses_bounds.npy"))
    assert pb1.shape == (3, 17) and np.abs(pb1[:, 15:] - T.s * pb0[:, 15:]).max() <= 1e-15 * 10 * T.s
    for k in range(3):
        blk = pb1[k, :15].reshape(3, 5)
        q, t = back[k + 1][:2]
        Rw = dr.quaternion_to_rotation(q)
        c2w = np.stack([blk[:, 1], blk[:, 0], -blk[:, 2]], 1)
        assert np.abs(c2w - Rw.T).max() <= 1e-12 and np.abs(blk[:, 3] - (-Rw.T @ t)).max() <= 1e-12 * max(1.0, T.s) * 10
        assert np.array_equal(blk[:, 4], [24.0, 32.0, 20.0])
    # moving back gives the folder's poses again
    back2 = str(tmp_path / "back")
    edit.transform_dataset(dst, back2, T.inverse())
    again = U.read_images_bin_full(os.path.join(back2, "sparse/0/images.bin"))
    for iid, rec in images.items():
        assert np.abs(again[iid][0] - rec[0]).max() <= 1e-12 and np.abs(again[iid][1] - rec[1]).max() <= 1e-11


def test_transform_dataset_refuses_by_name(tmp_path):
    import os
    blender, llff = str(tmp_path / "blender"), str(tmp_path / "llff")
    os.makedirs(blender)
    os.makedirs(llff)
    open(os.path.join(blender, "transforms_train.json"), "w").write("{}")
    np.save(os.path.join(llff, "poses_bounds.npy"), np.zeros((3, 17)))
    with pytest.raises(ValueError, match="Blender"):
        edit.transform_dataset(blender, str(tmp_path / "o1"), edit.Similarity())
    with pytest.raises(ValueError, match="poses_bounds.npy"):
        edit.transform_dataset(llff, str(tmp_path / "o2"), edit.Similarity())
    assert not os.path.exists(tmp_path / "o1") and not os.path.exists(tmp_path / "o2")      # nothing written
    with pytest.raises(ValueError, match="source folder"):
        edit.transform_dataset(llff, llff, edit.Similarity())
    # a COLMAP folder whose poses_bounds.npy cannot be moved is refused by that name, and so is an output inside the source
    bad = str(tmp_path / "bad")
    _colmap_folder(bad)
    np.save(os.path.join(bad, "poses_bounds.npy"), np.arange(6.0))
    with pytest.raises(ValueError, match=r"poses_bounds\.npy.*\[N, 17\]"):
        edit.transform_dataset(bad, str(tmp_path / "o3"), edit.Similarity())
    assert not os.path.exists(tmp_path / "o3")
    good = str(tmp_path / "good")
    _colmap_folder(good)
    with pytest.raises(ValueError, match="inside the source"):
        edit.transform_dataset(good, os.path.join(good, "moved"), edit.Similarity())
    assert not os.path.exists(os.path.join(good, "moved"))


@pytest.mark.parametrize("name", ["fern", "scan5"])
def test_spiral_of_the_moved_folder_is_the_moved_spiral(tmp_path, name):
    """The spiral path of the rewritten folder (camera_path reads poses_bounds.npy; DTU's rule when the path holds 'scan') is the
    spiral path of the source folder moved by transform_cameras.  In exact arithmetic the path construction commutes with a
    similarity (mean pose, percentiles of recentred positions, look-at frames, the focus depth from the bounds); in float64 the
    two sides differ by round-off through a few hundred operations and two inverses of rigid 4x4 matrices whose entries are of
    order 1..10, far below 1e-9, while a wrong axis order, a missed s on a bound or a stale file moves the cameras by O(0.1)."""
    import os
    import shutil
    from binocular3dgs_amd import camera_path
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene_llff")
    src, dst = str(tmp_path / name), str(tmp_path / (name + "_moved"))
    shutil.copytree(golden, src)
    R, t, s = edit_ref.random_similarity(31)
    T = edit.Similarity(R, t, s)
    info = edit.transform_dataset(src, dst, T)
    assert info["poses_bounds"] == 10 and camera_path.is_dtu(dst) == (name == "scan5")
    want = edit.transform_cameras(camera_path.spiral_cameras_from_dir(src, n_frames=24, device="cpu"), T)
    got = camera_path.spiral_cameras_from_dir(dst, n_frames=24, device="cpu")
    assert len(got) == len(want) == 24
    worst = 0.0
    for a, b in zip(got, want):
        assert (a.image_width, a.image_height, a.FoVx, a.FoVy) == (b.image_width, b.image_height, b.FoVx, b.FoVy)
        (Ra, Ca), (Rb, Cb) = edit._camera_pose(a), edit._camera_pose(b)
        worst = max(worst, np.abs(Ra - Rb).max(), np.abs(Ca - Cb).max() / max(1.0, s))
    print(f"spiral of the moved folder ({name}): worst pose difference {worst:.3e}")
    assert worst <= 1e-9
    # and it is another path than the source's: the check can see a folder that was not moved
    old = camera_path.spiral_cameras_from_dir(src, n_frames=24, device="cpu")
    assert max(np.abs(edit._camera_pose(a)[1] - edit._camera_pose(b)[1]).max() for a, b in zip(got, old)) > 0.1
