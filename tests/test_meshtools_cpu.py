"""CPU: the yardstick of the mesh tools (tests/meshtools_ref.py) against truths written out by hand, and the checks of the
ABI 18 entry points that need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meshtools_ref as tr  # noqa: E402
from binocular3dgs_amd import mesh_tools  # noqa: E402,F401  (the yardstick belongs to this module: without it nothing here runs)

F = np.float32
TETRA = [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]


def test_abi_version_is_18():
    from binocular3dgs_amd import _lib
    assert _lib.ABI_VERSION == 18 and _lib.lib().b3gs_abi_version() == 18


def test_components_of_three_tetrahedra_and_a_loose_vertex():
    """Tetrahedron A on vertices 0-3, B on 3-6 (they share vertex 3), C apart on 8-11; vertex 7 is named by no triangle."""
    faces = [[f + 0 for f in t] for t in TETRA] + [[f + 3 for f in t] for t in TETRA] + [[f + 8 for f in t] for t in TETRA]
    labels, count = tr.components(12, np.array(faces, np.int32))
    assert labels.tolist() == [0, 0, 0, 0, 0, 0, 0, 7, 8, 8, 8, 8]
    assert count.tolist() == [8, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0, 0]
    assert tr.threshold(count, 0, 0) == 1 and tr.threshold(count, 1, 0) == 8 and tr.threshold(count, 2, 0) == 4
    assert tr.threshold(count, 5, 0) == 1 and tr.threshold(count, 2, 6) == 6
    v = np.arange(36, dtype=F).reshape(12, 3)
    c = np.arange(36, dtype=np.uint8).reshape(12, 3)
    cv, cc, cf = tr.clean(v, c, np.array(faces, np.int32), keep_largest=1)
    assert np.array_equal(cv, v[:7]) and np.array_equal(cc, c[:7]) and cf.tolist() == faces[:8]
    cv, cc, cf = tr.clean(v, c, np.array(faces, np.int32))
    assert np.array_equal(cv, np.delete(v, 7, axis=0))
    assert cf.tolist() == faces[:8] + [[f + 7 for f in t] for t in TETRA]        # 8 -> 7 once vertex 7 is gone
    # a repeated index connects what it names
    labels, count = tr.components(4, np.array([[3, 3, 1]], np.int32))
    assert labels.tolist() == [0, 1, 2, 1] and count.tolist() == [0, 1, 0, 0]


def test_lattice_of_a_right_triangle_by_hand():
    """Legs 3.5 and 2.2 spacings: n1 = 3, n2 = 2, so i / 4 along e1 and j / 3 along e2; kept where 3 i + 4 j < 12, without (0, 0):
    i = 0: j = 1, 2;  i = 1: j = 0, 1, 2;  i = 2: j = 0, 1;  i = 3: j = 0  -- eight points."""
    s = 0.25
    pts = tr.lattice([0, 0, 0], [3.5 * s, 0, 0], [0, 2.2 * s, 0], s)
    ij = [(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (3, 0)]
    want = np.array([[F(i) / F(4) * F(3.5 * s), F(j) / F(3) * F(2.2 * s), 0.0] for i, j in ij], dtype=F)
    assert pts.shape == (8, 3) and np.array_equal(pts.view(np.uint32), want.view(np.uint32))
    # shorter than the spacing on both legs: the vertices only
    assert len(tr.lattice([0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], s)) == 0
    cloud = tr.sample_surface(np.array([[0, 0, 0], [3.5 * s, 0, 0], [0, 2.2 * s, 0]], F), np.array([[0, 1, 2]], np.int32), s)
    assert cloud.shape == (11, 3) and np.array_equal(cloud[3:], pts)


def test_lattice_count_closed_form():
    """csrc/meshtools.hip counts a lattice as ((A-1)(B-1) + g - 1) / 2 + A + B - g - 1, g = gcd(A, B): the enumeration."""
    from math import gcd
    for A in range(1, 14):
        for B in range(1, 14):
            n = sum(1 for i in range(A) for j in range(B) if (i or j) and i * B + j * A < A * B)
            g = gcd(A, B)
            assert n == ((A - 1) * (B - 1) + g - 1) // 2 + A + B - g - 1, (A, B)


def test_brute_force_on_three_points():
    b = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], F)
    a = np.array([[0.25, 0, 0], [1, 0, 0.5], [0, 2, 0], [10, 10, 10]], F)
    d = tr.nearest_distances(a, b, 3.0)
    assert d.dtype == F and d.tolist() == [0.25, 0.5, 0.0, 3.0]
    s = tr.score(d, tr.nearest_distances(b, a, 3.0), 0.3, mask_recon=np.array([True, True, True, False]))
    assert s["n_recon"] == 3 and s["accuracy"] == 0.25 and s["precision"] == 2 / 3
    assert s["n_gt"] == 3 and s["completeness"] == 0.25 and s["recall"] == 2 / 3 and s["fscore"] == pytest.approx(2 / 3, rel=1e-15)


def test_workspace_sizes_and_argument_checks_without_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    big = 1 << 31
    assert L.b3gs_mesh_clean_workspace_bytes(-1, 5) == 0 and L.b3gs_mesh_clean_workspace_bytes(5, big) == 0
    assert L.b3gs_mesh_clean_workspace_bytes(1000, 2000) % 256 == 0 and L.b3gs_mesh_clean_workspace_bytes(1000, 2000) >= 4 * 1000
    assert L.b3gs_mesh_clean_workspace_bytes(0, 0) > 0
    assert L.b3gs_mesh_sample_workspace_bytes(-1) == 0 and L.b3gs_mesh_sample_workspace_bytes(big) == 0
    assert L.b3gs_mesh_sample_workspace_bytes(300) >= 4 * 300
    assert L.b3gs_nearest_workspace_bytes(0) == 0 and L.b3gs_nearest_workspace_bytes(big) == 0
    assert L.b3gs_nearest_workspace_bytes(7001) >= 7001 * 36 + 8 * 8 * 7001
    assert L.b3gs_cloud_score_workspace_bytes(0) == 0 and L.b3gs_cloud_score_workspace_bytes(big) == 0
    assert L.b3gs_cloud_score_workspace_bytes(5003) % 256 == 0 and L.b3gs_cloud_score_workspace_bytes(5003) > 0
    ERR_ARG = -1
    assert L.b3gs_mesh_components(-1, 0, None, None, None, None) == ERR_ARG
    assert L.b3gs_mesh_components(4, 2, None, None, None, None) == ERR_ARG
    assert L.b3gs_mesh_components(0, 0, None, None, None, None) == 0
    assert L.b3gs_mesh_clean_count(4, 2, None, None, None, None, None, None) == ERR_ARG
    assert L.b3gs_mesh_clean_emit(4, 2, None, None, None, None, None, None, None, 0, 0, None, None, None, None) == ERR_ARG
    ws = C.c_void_p(256)                                      # aligned and never dereferenced: the checks come first
    assert L.b3gs_mesh_sample_count(3, 1, None, None, 0.0, ws, None) == ERR_ARG and b"spacing" in L.b3gs_last_error()
    assert L.b3gs_mesh_sample_count(3, 1, None, None, -1.0, ws, None) == ERR_ARG
    assert L.b3gs_mesh_sample_emit(3, 1, None, None, 1.0, ws, (1 << 31), None, None) == ERR_ARG
    assert L.b3gs_nearest_grid(0, None, 1.0, ws, None) == ERR_ARG and b"1 .." in L.b3gs_last_error()
    assert L.b3gs_nearest_grid(5, None, 0.0, ws, None) == ERR_ARG and b"max_dist" in L.b3gs_last_error()
    assert L.b3gs_nearest_query(5, None, 0, 1.0, ws, None, None) == ERR_ARG
    assert L.b3gs_cloud_score(0, None, None, 0.1, None, None, None) == ERR_ARG


def test_host_tensors_and_bad_arguments_are_refused():
    import torch
    from binocular3dgs_amd import _lib, mesh_tools
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mesh_tools.components(v, f)
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        mesh_tools.nearest_distances(v, v, 1.0)
    with pytest.raises(ValueError, match="spacing"):
        mesh_tools.sample_surface(v, f, 0.0)
    with pytest.raises(ValueError, match="empty"):
        mesh_tools.nearest_distances(v, torch.zeros(0, 3), 1.0)
    with pytest.raises(ValueError, match="int32"):
        mesh_tools.components(v, f.long())
    with pytest.raises(ValueError, match="negative"):
        mesh_tools.component_threshold(torch.zeros(3, dtype=torch.int32), -1, 0)
