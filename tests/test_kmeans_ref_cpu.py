"""No GPU: the k-means yardstick (tests/kmeans_ref.py) against a brute-force fp64 Lloyd step, the compressed-model file, the
argument checks of the three k-means entry points, and the undecided share of the seeded cases tests/test_gpu_kmeans.py runs."""
import ctypes as C
import os

import numpy as np
import pytest

import kmeans_ref as ref


def test_yardstick_equals_a_brute_force_lloyd_step():
    g = np.random.default_rng(7)
    N, K, D = 700, 5, 9                                  # ~140 members per code and one code past a chunk of 256
    x = g.standard_normal((N, D)).astype(np.float32)
    x[:400] += 4.0
    c = x[g.choice(N, K, replace=False)].copy()
    c[4] = 50.0                                          # no member: keeps its centroid
    w = g.random(N).astype(np.float32)
    w[::7] = 0.0
    best, decided, S, E = ref.assign(x, c)
    x64, c64, w64 = x.astype(np.float64), c.astype(np.float64), w.astype(np.float64)
    d2 = ((x64[:, None, :] - c64[None, :, :]) ** 2).sum(-1)
    brute = np.argmin(d2, axis=1)
    assert decided.mean() > 0.99 and np.array_equal(best[decided], brute[decided])
    assert np.all(ref.admissible(brute, best, S, E)) and np.all(E > 0)
    assert np.bincount(best, minlength=K).max() > ref.CHUNK and not np.any(best == 4)
    new = ref.update(x, w, best, c)
    for k in range(K):
        m = best == k
        if m.any():
            mean = (x64[m] * w64[m, None]).sum(0) / w64[m].sum()
            assert np.allclose(new[k], mean, rtol=1e-6, atol=0) and new[k].dtype == np.float32
    assert np.array_equal(new[4], c[4])
    assert np.array_equal(ref.update(x, np.zeros(N, np.float32), best, c), c)          # sum w == 0 keeps every centroid
    uni = ref.update(x, None, best, c)
    assert np.allclose(uni[0], x64[best == 0].mean(0), rtol=1e-6)
    dist = ref.distortion(x, w, c, best)
    want = float((w64 * d2[np.arange(N), best]).sum())
    assert abs(dist - want) <= 1e-12 * want
    assert abs(ref.distortion(x, None, c, best) - d2[np.arange(N), best].sum()) <= 1e-12 * d2.sum()
    # a Lloyd step never raises the distortion by more than the float32 decisions allow
    b2 = ref.assign(x, new)[0]
    assert ref.distortion(x, w, new, b2) <= dist + ref.step_bound(x, new, w)
    # h is the float32 of the fp64 half norm
    assert np.array_equal(ref.half_norms(c), (0.5 * (c64 * c64).sum(1)).astype(np.float32))


def test_integer_cases_are_exact_and_tie_to_the_lower_code():
    x, c = ref.integer_case(200, 40, 12, 3, duplicates=True)
    best, _decided, S, _E = ref.assign(x, c)
    assert np.array_equal(c[20:40], c[:20]) and best.max() < 20           # a duplicate never wins over its original
    assert np.array_equal(S, np.round(S * 2) / 2) and np.abs(S).max() < 2 ** 23


@pytest.mark.parametrize("N,K,D,seed", ref.FLOAT_CASES)
def test_undecided_share_of_the_seeded_float_cases(N, K, D, seed):
    x, c = ref.float_case(N, K, D, seed)
    _best, decided, _S, _E = ref.assign(x, c)
    assert (~decided).sum() <= 0.01 * N, f"{(~decided).sum()} of {N} rows undecided: pick another seed"


def _hand_built():
    from binocular3dgs_amd.compress import CompressedModel
    g = np.random.default_rng(1)
    P = 9
    return CompressedModel(xyz=g.standard_normal((P, 3)).astype(np.float32), opacity=g.standard_normal((P, 1)).astype(np.float16),
                           colour_codebook=g.standard_normal((4, 12)).astype(np.float32),
                           colour_index=g.integers(0, 4, P).astype(np.uint16),
                           shape_codebook=g.standard_normal((3, 7)).astype(np.float32),
                           shape_index=g.integers(0, 3, P).astype(np.uint16), colour_distortion=np.array([3.0, 2.0, 1.5]),
                           shape_distortion=np.array([1.0, 0.5, 0.25]), sh_degree=1, active_sh_degree=0)


def test_compressed_model_file_round_trip(tmp_path):
    from dataclasses import fields
    from binocular3dgs_amd import compress
    cm = _hand_built()
    path = str(tmp_path / "model.npz")
    compress.save_compressed(path, cm)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = compress.load_compressed(path)
    for f in fields(cm):
        a, b = getattr(cm, f.name), getattr(back, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f.name
        else:
            assert a == b and type(b) is int, f.name
    with np.load(path) as z:
        assert int(z["format_version"]) == compress.FORMAT_VERSION and int(z["sh_degree"]) == 1
    assert compress.compressed_bytes(cm) == 9 * (12 + 2 + 2 + 2) + 4 * 12 * 4 + 3 * 7 * 4
    bad = _hand_built()
    bad.colour_index = bad.colour_index.astype(np.int32)
    with pytest.raises(ValueError, match="colour_index"):
        compress.save_compressed(path, bad)
    bad = _hand_built()
    bad.shape_index[0] = 3
    with pytest.raises(ValueError, match="past"):
        compress.save_compressed(path, bad)
    np.savez(str(tmp_path / "other.npz"), xyz=cm.xyz)
    with pytest.raises(ValueError, match="format version"):
        compress.load_compressed(str(tmp_path / "other.npz"))


def test_kmeans_argument_errors_are_reported_without_touching_a_device():
    from binocular3dgs_amd import _lib
    L = _lib.lib()
    ERR_ARG = -1
    p = C.c_void_p(256)                                  # never dereferenced: every check comes before the first HIP call
    assert L.b3gs_kmeans_workspace_bytes(1000, 12, 256) > 0 and L.b3gs_kmeans_workspace_bytes(1000, 12, 256) % 256 == 0
    assert L.b3gs_kmeans_workspace_bytes(10 ** 6, 48, 4096) < 200 * 10 ** 6
    for N, D, K in ((10, 0, 4), (10, 65, 4), (10, 7, 0), (10, 7, 65537), (-1, 7, 4)):
        assert L.b3gs_kmeans_workspace_bytes(N, D, K) == 0
        assert L.b3gs_kmeans_assign(N, D, K, p, p, p, p, None) == ERR_ARG
        assert L.b3gs_kmeans(N, D, K, 1, p, None, p, p, p, p, p, None) == ERR_ARG
    assert b"D <= 64" in L.b3gs_last_error() or b"N must" in L.b3gs_last_error()
    assert L.b3gs_kmeans(10, 7, 4, -1, p, None, p, p, p, p, p, None) == ERR_ARG and b"iters" in L.b3gs_last_error()
    for hole in range(4):                                # x, codebook, codes, workspace
        a = [p, p, p, p]
        a[hole] = None
        assert L.b3gs_kmeans_assign(10, 7, 4, a[0], a[1], a[2], a[3], None) == ERR_ARG and b"NULL" in L.b3gs_last_error()
    for hole in range(6):                                # x, codebook, codes, counts, distortion, workspace (weights may be NULL)
        a = [p, p, p, p, p, p]
        a[hole] = None
        assert L.b3gs_kmeans(10, 7, 4, 1, a[0], None, a[1], a[2], a[3], a[4], a[5], None) == ERR_ARG
    assert L.b3gs_kmeans_assign(10, 7, 4, p, p, p, C.c_void_p(264), None) == ERR_ARG and b"aligned" in L.b3gs_last_error()
    assert L.b3gs_kmeans_assign(0, 7, 4, None, None, None, None, None) == 0            # no rows: nothing to do
    assert L.b3gs_kmeans(0, 7, 4, 3, None, None, None, None, None, None, None, None) == 0
    with pytest.raises(_lib.B3gsError):
        _lib.check(L.b3gs_kmeans_assign(10, 0, 4, p, p, p, p, None), "b3gs_kmeans_assign")


def test_python_surface_refuses_host_tensors():
    import torch
    from binocular3dgs_amd import _lib, compress
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        compress.assign(torch.zeros(5, 3), torch.zeros(2, 3))
    with pytest.raises(_lib.B3gsError, match="HIP device only"):
        compress.kmeans(torch.zeros(5, 3), 2)
    q = compress.canonical_rotation(torch.tensor([[-2.0, 0.0, 0.0, 0.0], [0.0, 0.0, -3.0, 4.0], [1.0, -1.0, 1.0, -1.0]]))
    assert torch.equal(q, torch.tensor([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.6, -0.8], [0.5, -0.5, 0.5, -0.5]]))
