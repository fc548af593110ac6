"""CPU: the yardstick of the mesh extraction (tests/mesh_ref.py) holds the properties a marching-tetrahedra mesh must have,
and the host side of ABI 17 (argument checks before any device call, the PLY writer, the command line) works without a GPU.
The kernels themselves are held against the yardstick in tests/test_gpu_mesh.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref as mr  # noqa: E402

F = np.float32


sphere_volume, random_volume, plane_scene = mr.sphere_volume, mr.random_volume, mr.plane_scene


def test_sphere_mesh_is_closed_and_oriented():
    vol = sphere_volume()
    vertices, colours, faces = mr.extract(vol)
    assert len(vertices) > 1000 and len(faces) > 2000
    _, uses = mr.edge_uses(faces)
    assert (uses == 2).all()
    assert mr.euler_characteristic(len(vertices), faces) == 2
    volume = mr.signed_volume(vertices, faces)
    assert volume > 0
    exact = 4.0 / 3.0 * math.pi * 6.0 ** 3
    # measured from the yardstick: 0.013904 (the chords of a radius-6 sphere at unit voxels cut 1.4 % off); bound: twice that
    assert abs(volume - exact) / exact <= 2 * 0.013904


def test_random_field_covers_every_case():
    vol = random_volume()
    assert mr.cases_seen(vol).all()                      # all 16 cases of all 6 tetrahedra
    vertices, colours, faces = mr.extract(vol)
    assert len(faces) > 0
    assert faces.min() >= 0 and faces.max() < len(vertices)
    assert (np.bincount(faces.reshape(-1), minlength=len(vertices)) > 0).all()       # no unreferenced vertex
    assert vertices.dtype == np.float32 and colours.dtype == np.uint8 and faces.dtype == np.int32


def test_case_table_follows_the_orientation_rule():
    table = mr.tables()
    for t in range(6):
        assert table[t][0] == [] and table[t][15] == []
        for case in range(1, 15):
            assert len(table[t][case]) == (2 if bin(case).count("1") == 2 else 1)
            # the complementary case cuts the same edges, wound the other way
            a = [tuple(tri) for tri in table[t][case]]
            b = [tuple(tri) for tri in table[t][15 - case]]
            assert sorted(sorted(tri) for tri in a) == sorted(sorted(tri) for tri in b)


def test_fused_plane_lies_on_the_plane():
    z0 = 2.8
    cams, depths, alphas, colours = plane_scene(z0=z0)
    vol = mr.new_volume((20, 17, 13), origin=(-1.25, -1.0625, 2.0), voxel=0.125)
    mr.integrate(vol, cams, depths, alphas, colours, truncation=0.5)
    assert vol["weight"].max() == 3.0 and (vol["weight"] == 0).any()
    vertices, _, faces = mr.extract(vol)
    assert len(faces) > 100
    # Linear interpolation of a linear function is exact, so a vertex leaves the plane only by the roundings on its way:
    # 3 in the camera z of a voxel, 2 in sdf / truncation, 2 per step of the running average (3 views), 3 in t and 2 in
    # p0 + t (p1 - p0): fewer than 16, each at most 2^-24 of the largest magnitude in play (the far side of the box, 3.625).
    assert np.abs(vertices[:, 2].astype(np.float64) - z0).max() <= 16 * 2.0 ** -24 * 3.625


def test_ply_round_trip(tmp_path):
    from binocular3dgs_amd import mesh
    vertices, colours, faces = mr.extract(random_volume())
    path = str(tmp_path / "m.ply")
    mesh.write_mesh_ply(path, vertices, colours, faces)
    v, c, f = mesh.read_mesh_ply(path)
    assert v.dtype == np.float32 and c.dtype == np.uint8 and f.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), vertices.view(np.uint32)) and np.array_equal(c, colours) and np.array_equal(f, faces)
    with open(path, "rb") as fp:
        data = fp.read()
    assert data.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(vertices))
    body = data.index(b"end_header\n") + 11
    assert len(data) == body + 15 * len(vertices) + 13 * len(faces)          # 3 floats + 3 bytes; a count byte + 3 ints
    empty = str(tmp_path / "e.ply")
    mesh.write_mesh_ply(empty, np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    v, c, f = mesh.read_mesh_ply(empty)
    assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)


def test_argument_errors_without_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    ERR_ARG = -1
    vol = _lib.B3gsTsdfVolume()
    vol.nx, vol.ny, vol.nz, vol.voxel = 20, 17, 13, 0.125
    vol.tsdf, vol.weight, vol.rgb = 256, 256, 256            # non-NULL: never dereferenced, every call below is refused
    views = (_lib.B3gsTsdfView * 9)()
    for v in views:
        v.depth, v.alpha, v.colour = 256, 256, 256
    call = L.b3gs_tsdf_integrate_batch
    assert call(C.byref(vol), 0, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG and b"views" in L.b3gs_last_error()
    assert call(C.byref(vol), 9, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG and b"views" in L.b3gs_last_error()
    assert call(C.byref(vol), 1, views, 40, 30, 0.0, 0.2, 0.5, None) == ERR_ARG and b"truncation" in L.b3gs_last_error()
    assert call(C.byref(vol), 1, views, 40, 30, -1.0, 0.2, 0.5, None) == ERR_ARG
    assert call(C.byref(vol), 1, views, 40, 30, 0.5, 0.2, 0.0, None) == ERR_ARG and b"alpha_min" in L.b3gs_last_error()
    assert call(C.byref(vol), 1, views, 0, 30, 0.5, 0.2, 0.5, None) == ERR_ARG
    assert call(None, 1, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG and b"NULL" in L.b3gs_last_error()
    assert call(C.byref(vol), 1, None, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG
    big = _lib.B3gsTsdfVolume()
    C.memmove(C.byref(big), C.byref(vol), C.sizeof(vol))
    big.ny = 1025
    assert call(C.byref(big), 1, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG and b"1024" in L.b3gs_last_error()
    null = _lib.B3gsTsdfVolume()
    C.memmove(C.byref(null), C.byref(vol), C.sizeof(vol))
    null.weight = None
    assert call(C.byref(null), 1, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG and b"NULL" in L.b3gs_last_error()
    views[0].alpha = None
    assert call(C.byref(vol), 1, views, 40, 30, 0.5, 0.2, 0.5, None) == ERR_ARG
    # count / emit
    assert L.b3gs_mesh_count(None, 1.0, 256, None) == ERR_ARG
    assert L.b3gs_mesh_count(C.byref(big), 1.0, 256, None) == ERR_ARG
    assert L.b3gs_mesh_count(C.byref(vol), 1.0, None, None) == ERR_ARG
    assert L.b3gs_mesh_count(C.byref(vol), 1.0, 257, None) == ERR_ARG and b"aligned" in L.b3gs_last_error()
    assert L.b3gs_mesh_emit(C.byref(vol), 256, 1 << 31, 1, 256, 256, 256, None) == ERR_ARG and b"2^31" in L.b3gs_last_error()
    assert L.b3gs_mesh_emit(C.byref(vol), 256, 1, 1 << 31, 256, 256, 256, None) == ERR_ARG
    assert L.b3gs_mesh_emit(C.byref(vol), 256, -1, 0, 256, 256, 256, None) == ERR_ARG
    assert L.b3gs_mesh_emit(C.byref(vol), 256, 5, 5, None, 256, 256, None) == ERR_ARG
    assert L.b3gs_mesh_emit(C.byref(vol), 256, 0, 0, None, None, None, None) == 0          # an empty mesh: nothing to launch
    # the workspace: totals + 6 bytes per voxel + two words per block of 256 voxels, 256-byte aligned; 0 for bad sizes
    n = 20 * 17 * 13
    size = L.b3gs_mesh_workspace_bytes(20, 17, 13)
    assert size % 256 == 0 and 6 * n < size < 6 * n + 8 * 256
    assert L.b3gs_mesh_workspace_bytes(1025, 4, 4) == 0 and L.b3gs_mesh_workspace_bytes(4, 0, 4) == 0
    assert L.b3gs_mesh_workspace_bytes(1024, 1024, 1024) > 6 * 2 ** 30
    assert C.sizeof(_lib.B3gsTsdfView) == 3 * 8 + 14 * 4 and C.sizeof(_lib.B3gsTsdfVolume) == 7 * 4 + 4 + 3 * 8


def test_compiled_module_refuses_host_tensors():
    import torch
    from binocular3dgs_amd import _C, _lib
    z = torch.zeros
    cams = torch.zeros(1, 14)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.tsdf_integrate(z(4, 4, 4), z(4, 4, 4), z(4, 4, 4, 3), [0.0, 0.0, 0.0], 1.0, [z(8, 8)], [z(8, 8)], [z(3, 8, 8)], cams, 4.0)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.mesh_count(z(4, 4, 4), z(4, 4, 4), z(4, 4, 4, 3), [0.0, 0.0, 0.0], 1.0)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        _C.mesh_emit(z(4, 4, 4), z(4, 4, 4), z(4, 4, 4, 3), [0.0, 0.0, 0.0], 1.0, torch.zeros(8, dtype=torch.uint8), 0, 0)
    assert _C.mesh_workspace_bytes(20, 17, 13) == _lib.lib().b3gs_mesh_workspace_bytes(20, 17, 13)


def test_volume_and_command_line_defaults():
    from binocular3dgs_amd import extract_mesh, mesh
    a = extract_mesh.parser().parse_args(["-m", "out"])
    assert (a.model_path, a.source_path, a.iteration, a.views) == ("out", None, -1, "train")
    assert a.resolution is None and a.voxel_size is None and a.bounds is None
    assert (a.truncation_voxels, a.alpha_min, a.min_weight) == (4.0, 0.5, 1.0)
    a = extract_mesh.parser().parse_args(["-m", "out", "--views", "all", "--voxel_size", "0.01", "--bounds", "0", "0", "0", "1", "2", "3"])
    assert a.views == "all" and a.voxel_size == 0.01 and a.bounds == [0.0, 0.0, 0.0, 1.0, 2.0, 3.0]
    with pytest.raises(SystemExit):
        extract_mesh.parser().parse_args(["-m", "out", "--resolution", "64", "--voxel_size", "0.01"])
    vol = mesh.TsdfVolume((0.0, 0.0, 0.0), (2.5, 2.125, 1.625), 0.125, device="cpu")
    assert vol.dims == (20, 17, 13) and vol.truncation == 0.5 and vol.tsdf.shape == (13, 17, 20) and vol.rgb.shape == (13, 17, 20, 3)
    with pytest.raises(ValueError, match="1024"):
        mesh.TsdfVolume((0.0, 0.0, 0.0), (1025.0, 1.0, 1.0), 1.0, device="cpu")
