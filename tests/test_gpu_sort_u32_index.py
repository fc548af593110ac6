"""GPU: b3gs_launch_sort_u32_index -- the 8-bit radix family of csrc/binning.hip with values and no device-side count --
against numpy's stable argsort, exactly, at the seams of its 4096-key radix tiles.

The function is internal to the library and its callers (knn, kmeans, meshtools, simplify, meshsmooth) derive the keys
themselves, but two of them sort inside a workspace that the CALLER owns, where the keys, the sorted keys and the permutation
stay behind:
  * the k-nearest-neighbour init sorts the Morton codes of its points (layout: knn.hip::carve_ws).  Any n can be had; points
    on an 8 x 8 x 8 lattice give at most 512 distinct codes, so every size but 1 is full of ties, whose order only a stable
    sort keeps.  Morton codes have 30 bits: no key above 0x3FFFFFFF.
  * the mesh adjacency build sorts the 6 F directed edges of a mesh by their first vertex (layout: meshsmooth.hip::adj_carve;
    gkey is the input of that last sort).  The edges of a face with an out-of-range index, and edges with equal ends, carry
    the key 0xFFFFFFFF; 40 vertices give ties everywhere.  n = 6 F crosses the tile seams at 4092 | 4098 and 8190 | 8196."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _a256(nbytes):
    return (nbytes + 255) & ~255


def _words(ws, offset, n):
    return ws[offset: offset + 4 * n].cpu().numpy().view(np.uint32)


def _assert_stable_sort(keys, skey, sval):
    perm = np.argsort(keys, kind="stable")
    assert np.array_equal(sval, perm.astype(np.uint32))
    assert np.array_equal(skey, keys[perm])


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8193])
def test_sort_u32_index_is_the_stable_argsort(n):
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    pts = rng.integers(0, 8, size=(n, 3)).astype(np.float32)
    pts[0] = 7.0                                      # the bounding box is the whole lattice at every n
    dev = torch.from_numpy(pts).cuda()
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    ws = torch.full((L.b3gs_knn_workspace_bytes(n),), 255, dtype=torch.uint8, device="cuda")   # (no result is the fill value)
    _lib.check(L.b3gs_knn_mean_dist2(n, dev.data_ptr(), out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "b3gs_knn_mean_dist2")
    torch.cuda.synchronize()
    first, step = _a256(6 * 256 * 4), _a256(4 * n)    # part | codes | skey[0] | skey[1] | sval[0] | sval[1] | ...
    codes, skey, sval = (_words(ws, first + k * step, n) for k in (0, 1, 3))
    assert int(codes.max()) == 0x3FFFFFFF and (n == 1 or len(np.unique(codes)) < n)   # bits in every pass, and ties
    _assert_stable_sort(codes, skey, sval)


@pytest.mark.parametrize("F", [682, 683, 1365, 1366])
def test_sort_u32_index_with_all_ones_keys(F):
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    V, n = 40, 6 * F
    rng = np.random.default_rng(F)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    bad = rng.random(F) < 0.25
    faces[bad, rng.integers(0, 3, size=int(bad.sum()))] = rng.choice(np.array([-1, V, 2**31 - 1], dtype=np.int32), size=int(bad.sum()))
    ends = np.stack([faces, np.roll(faces, -1, axis=1)], axis=2)                       # [F, 3, 2]: edge e = (corner e, corner e + 1)
    no_key = 6 * int(bad.sum()) + 2 * int((ends[~bad, :, 0] == ends[~bad, :, 1]).sum())
    ws = torch.zeros(L.b3gs_mesh_adjacency_workspace_bytes(V, F), dtype=torch.uint8, device="cuda")
    verts = torch.zeros(V, 3, device="cuda")
    _lib.check(L.b3gs_mesh_adjacency_build(V, F, verts.data_ptr(), torch.from_numpy(faces).cuda().data_ptr(), ws.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "b3gs_mesh_adjacency_build")
    torch.cuda.synchronize()
    offs = (C.c_size_t * 5)()
    _lib.check(L.b3gs_mesh_adjacency_layout(V, F, offs), "b3gs_mesh_adjacency_layout")
    # behind `pinned` [V bytes]: pos[2] (float4 [V]) | skey[2] | sval[2] | hist (b3gs_sort_scratch_words(n)) | pa | pb | ord | gkey
    step = _a256(4 * n)
    skey0 = offs[4] + _a256(V) + 2 * _a256(16 * V)
    gkey0 = skey0 + 4 * step + _a256(4 * (1280 + 8192 + 4 * 256 * ((n + 4095) // 4096 + 1))) + 3 * step
    keys, skey, sval = _words(ws, gkey0, n), _words(ws, skey0, n), _words(ws, skey0 + 2 * step, n)
    assert no_key > 64 and int((keys == 0xFFFFFFFF).sum()) == no_key                   # (the array read IS the sort's input)
    assert set(np.unique(keys)) <= set(range(V)) | {0xFFFFFFFF} and len(np.unique(keys)) > 2
    _assert_stable_sort(keys, skey, sval)
