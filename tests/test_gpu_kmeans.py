"""GPU: weighted k-means on the device (binocular3dgs_amd/compress.py, csrc/kmeans.hip) against the float64 yardstick
tests/kmeans_ref.py.

  1. assignment bit for bit on integer data (every float32 chain is exact): ties to the lower code, K = 1, N < K, N = 1, N and K
     around the kernel's row tile (512) and code tile (128), every instantiated depth;
  2. assignment on random float data: decided rows exactly, undecided rows within the rounding bound of the best;
  3. the update bit for bit: weighted rows, zero-weight rows, an all-zero w, empty codes, codes of more than one chunk;
  4. the loop: iters = 4 equals four chained iters = 1 calls, counts, the distortion and its monotony, call-to-call bits;
  5. the lossless limit k >= N."""
import functools

import numpy as np
import pytest
import torch

import kmeans_ref as ref
from binocular3dgs_amd import compress

pytestmark = pytest.mark.gpu

RT, CT = ref.ROW_TILE, ref.CODE_TILE
INTEGER_CASES = (
    [(300, 64, 12, True), (200, 1, 7, False), (5, 40, 12, False), (1, 33, 7, False)]
    + [(n, 33, 12, False) for n in (RT - 1, RT, RT + 1, 2 * RT + 1)]
    + [(300, k, 7, False) for k in (CT - 1, CT, CT + 1, 257)]
    + [(300, 40, d, True) for d in (1, 7, 12, 47, 48, 64)])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N,K,D,dup", INTEGER_CASES)
def test_assignment_is_exact_on_integer_data(N, K, D, dup):
    x, c = ref.integer_case(N, K, D, 1000 + N + 7 * K + 13 * D, duplicates=dup)
    best = ref.assign(x, c)[0]
    codes = host(compress.assign(dev(x), dev(c)))
    assert codes.dtype == np.int32 and codes.shape == (N,)
    assert np.array_equal(codes, best), f"{int((codes != best).sum())} of {N} rows differ"
    if dup and K > 1:
        assert codes.max() < K // 2 or not np.array_equal(c[K // 2:K // 2 * 2], c[:K // 2])


@pytest.mark.parametrize("N,K,D,seed", ref.FLOAT_CASES)
def test_assignment_on_float_data_is_decided_or_within_the_bound(N, K, D, seed):
    x, c = ref.float_case(N, K, D, seed)
    best, decided, S, E = ref.assign(x, c)
    codes = host(compress.assign(dev(x), dev(c))).astype(np.int64)
    print(f"undecided {int((~decided).sum())} of {N}, differing from the fp64 best {int((codes != best).sum())}")
    assert (~decided).sum() <= 0.01 * N
    assert codes.min() >= 0 and codes.max() < K
    assert np.array_equal(codes[decided], best[decided])
    assert np.all(ref.admissible(codes, best, S, E))


@functools.lru_cache(maxsize=None)
def _update_case():
    """3000 rows in two clumps, 6 codes (a code holds more than one chunk of 256 members) and a seventh far away (no member)."""
    g = np.random.default_rng(21)
    N, D = 3000, 12
    x = g.standard_normal((N, D)).astype(np.float32)
    x[:1700] += 3.0
    c = np.concatenate([x[g.choice(N, 6, replace=False)], np.full((1, D), 60.0, np.float32)]).astype(np.float32)
    w = (g.random(N) * 3.0).astype(np.float32)
    w[g.choice(N, 400, replace=False)] = 0.0
    codes0 = host(compress.assign(dev(x), dev(c)))
    return x, c, w, codes0


@pytest.mark.parametrize("weights", ["none", "weighted", "zero"])
def test_update_equals_the_yardstick_bit_for_bit(weights):
    x, c, w, codes0 = _update_case()
    w = {"none": None, "weighted": w, "zero": np.zeros_like(w)}[weights]
    counts0 = np.bincount(codes0, minlength=c.shape[0])
    assert counts0.max() > ref.CHUNK and counts0[6] == 0
    want = ref.update(x, w, codes0, c)
    cb, codes, counts, dist = compress.kmeans(dev(x), c.shape[0], None if w is None else dev(w), iters=1, init=dev(c))
    cb = host(cb)
    assert same_bits(cb, want), f"largest difference {np.abs(cb.astype(np.float64) - want).max()}"
    assert same_bits(cb[6], c[6])                         # the empty code keeps its centroid
    if weights == "zero":
        assert same_bits(cb, c) and np.array_equal(host(dist), np.zeros(2))
    else:
        assert not np.array_equal(cb[:6], c[:6])
    assert same_bits(host(codes), host(compress.assign(dev(x), dev(cb))))     # the codes belong to the returned codebook
    assert same_bits(host(dev(c)), c)                     # init is not written


def test_loop_outputs():
    x, c, w, codes0 = _update_case()
    K = c.shape[0]
    xd, wd = dev(x), dev(w)
    cb4, codes4, counts4, dist4 = compress.kmeans(xd, K, wd, iters=4, init=dev(c))
    chain, cur, d = [c], dev(c), []
    for _ in range(4):
        cur, codes1, counts1, dist1 = compress.kmeans(xd, K, wd, iters=1, init=cur)
        chain.append(host(cur))
        d.append(host(dist1))
    assert same_bits(host(cb4), chain[-1]) and same_bits(host(codes4), host(codes1)) and same_bits(host(counts4), host(counts1))
    dist4 = host(dist4)
    assert dist4.dtype == np.float64 and dist4.shape == (5,)
    assert same_bits(dist4, np.array([d[0][0], d[1][0], d[2][0], d[3][0], d[3][1]]))
    codes4 = host(codes4)
    assert host(counts4).dtype == np.int32 and np.array_equal(host(counts4), np.bincount(codes4, minlength=K))
    first, last = ref.distortion(x, w, c, codes0), ref.distortion(x, w, chain[-1], codes4)
    print(f"distortion {dist4}; yardstick first {first} last {last}")
    assert abs(dist4[0] - first) <= 1e-12 * first and abs(dist4[4] - last) <= 1e-12 * last
    for i in range(4):
        assert dist4[i + 1] <= dist4[i] + ref.step_bound(x, chain[i + 1], w), i
    assert dist4[4] < 0.9 * dist4[0]
    # iters = 0: the assignment and its distortion alone
    cb0, codes_0, _counts, dist0 = compress.kmeans(xd, K, wd, iters=0, init=dev(c))
    assert same_bits(host(cb0), c) and same_bits(host(codes_0), codes0) and same_bits(host(dist0), dist4[:1])
    # the same bits on a second stream, and with the rows given in two unequal parts
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = compress.kmeans(xd, K, wd, iters=4, init=dev(c))
    side.synchronize()
    for a, b in zip(again, (cb4, codes4, counts4, dist4)):
        assert same_bits(host(a), b if isinstance(b, np.ndarray) else host(b))
    whole = host(compress.assign(xd, cb4))
    parts = np.concatenate([host(compress.assign(xd[:1100], cb4)), host(compress.assign(xd[1100:], cb4))])
    assert same_bits(whole, parts) and same_bits(whole, codes4)


def test_default_init_and_the_lossless_limit():
    g = np.random.default_rng(5)
    N, D = 300, 7
    x = g.standard_normal((N, D)).astype(np.float32)
    w = (0.5 + g.random(N)).astype(np.float32)
    for weights in (None, dev(w)):
        cb, codes, counts, dist = compress.kmeans(dev(x), N + 5, weights, iters=3)
        assert same_bits(host(cb), x) and np.array_equal(host(codes), np.arange(N)) and np.array_equal(host(counts), np.ones(N))
        assert np.array_equal(host(dist), np.zeros(4))
    # k < N: the rows at the sorted first k entries of a seeded CPU permutation
    idx = torch.sort(torch.randperm(N, generator=torch.Generator().manual_seed(9))[:16]).values.numpy()
    cb, _codes, _counts, _dist = compress.kmeans(dev(x), 16, iters=0, seed=9)
    assert same_bits(host(cb), x[idx])
    with pytest.raises(ValueError):
        compress.kmeans(dev(x), 70000, init=dev(np.zeros((70000, D), np.float32)))
    with pytest.raises(ValueError):
        compress.kmeans(dev(np.zeros((4, 65), np.float32)), 2)
