// Weighted k-means codebooks of a trained model's rows (added to ABI 18; binocular3dgs_amd/compress.py): the vector
// quantisation of Niedermayr et al., "Compressed 3D Gaussian Splatting" (2024), and of LightGaussian's VecTree step.
//
// ASSIGNMENT (N rows [N,D] against K codes [K,D]; tests/kmeans_ref.py is the fp64 yardstick)
//   h_k    = float32( 0.5 * sum_d c_kd^2 ), the sum in fp64 with d ascending
//   a_0    = -h_k,  a_{d+1} = fmaf(x_nd, c_kd, a_d)  for d = 0 .. D-1        (float32)
//   code_n = the smallest k whose a_D is largest                              (argmin of |x - c|^2 = argmax of x.c - |c|^2 / 2)
// D is padded with zeros to the MFMA's k-step (and to the instantiated depth): fmaf(0, 0, a) = a, the chain is unchanged.
// NaN and Inf inputs are undefined.
// The chain is v_mfma_f32_32x32x2_f32 with the accumulator carried through all steps of a (row tile, code tile) pair: rows of
// the accumulator tile are codes, columns are data rows.  A wave owns RT = 4 tiles of 32 data rows (its x values stay in
// registers: four independent accumulators hide the instruction's dependent latency) and walks the codes 32 at a time in
// ascending order; a workgroup is four waves = ROWS = 512 data rows, and stages CT = 128 codes (transposed, with their h) in
// LDS per step.  Every lane keeps a running (best, k) over its 16 accumulator registers with a strict compare in ascending
// k; the two half-waves (which hold the codes 4 (l >> 5) + .. of the same data row) are merged once per row tile.
//
// UPDATE (fp64, no floating-point atomic, the order does not depend on the launch shape)
//   The codes are sorted with the stable radix sort: a code's members come in row order.  The members of a code are cut into
//   chunks of CHUNK = 256 members; a chunk's sums  s_d = s_d + w_n x_nd  (and s_w = s_w + w_n) run in member order from 0,
//   a code's sums are its chunk sums added in chunk order from 0.  w and x are float32, every product is exact in fp64.
//   c_kd = float32( S_d / S_w ).  A code with no member or with S_w == 0 keeps its centroid.  w == NULL is w_n = 1.
//
// DISTORTION of an assignment:  v_n = w_n * sum_d (x_nd - c_kd)^2, k = code_n: differences, squares and the sum over d
//   (ascending, from 0) in fp64.  B = min(ceil(N / 256), 256) workgroups; thread t of workgroup b adds the rows
//   256 b + t + 256 B j, j ascending; the workgroup's sum and the fold of the B partials are b3gs_block_sum_f64 /
//   b3gs_wave_fold_f64 (the trees of csrc/metrics.hip and the LPIPS taps).
#include "b3gs_internal.h"

#include <limits>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TPB = 256;
constexpr int RT = 4;                    // row tiles (of 32 data rows) per wave
constexpr int ROWS = 4 * RT * 32;        // data rows of a workgroup: 512
constexpr int CT = 128;                  // codes staged per step
constexpr int CHUNK = 256;               // members of an update chunk
constexpr int DBLOCKS = 256;             // most distortion partials
constexpr int MAXD = 64, MAXK = 65536;

// k-steps (of two dimensions) of the instantiated kernels: D <= 8, 12, 16, 32, 48, 64
static int ksteps_of(int D) { return D <= 8 ? 4 : D <= 12 ? 6 : D <= 16 ? 8 : D <= 32 ? 16 : D <= 48 ? 24 : 32; }
static int padded_codes(int K) { return (K + CT - 1) / CT * CT; }

// thread = code k < Kp: h[k] and column k of the transposed codebook ct[Dp][Kp]; codes beyond K: zeros and h = +inf (their
// score is -inf: never the strict maximum of a row)
__global__ void __launch_bounds__(TPB) prep_kernel(const float* __restrict__ cb, int D, int K, int Dp, int Kp, float* __restrict__ ct,
                                                   float* __restrict__ h) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= Kp) return;
  double s = 0.0;
  for (int d = 0; d < Dp; d++) {
    const float c = (k < K && d < D) ? cb[(size_t)k * D + d] : 0.f;
    ct[(size_t)d * Kp + k] = c;
    s += (double)c * (double)c;
  }
  h[k] = k < K ? (float)(0.5 * s) : std::numeric_limits<float>::infinity();
}

// MFMA operands (one VGPR each): lane l gives A[row = l & 31][k = l >> 5] and B[k = l >> 5][col = l & 31]; accumulator register
// e of lane l is D[row = (e & 3) + 8 (e >> 2) + 4 (l >> 5)][col = l & 31].  Rows are codes, columns data rows.
template <int KS>
__global__ void __launch_bounds__(TPB) assign_kernel(int N, int D, int K, int Kp, const float* __restrict__ x,
                                                     const float* __restrict__ ct, const float* __restrict__ hs,
                                                     int32_t* __restrict__ codes) {
  constexpr int DP = 2 * KS;
  __shared__ float As[DP * CT];
  __shared__ float Hs[CT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS + wave * (RT * 32);

  // this lane's B operands: x[row][2 i + h] of its RT data rows (zero beyond D and beyond N)
  float xr[RT][KS];
#pragma unroll
  for (int q = 0; q < RT; q++) {
    const int64_t row = row0 + q * 32 + r;
    const float* __restrict__ xp = x + (size_t)(row < N ? row : 0) * D;
#pragma unroll
    for (int i = 0; i < KS; i++) {
      const int d = 2 * i + h;
      xr[q][i] = (row < N && d < D) ? xp[d] : 0.f;
    }
  }
  float best[RT];
  int bk[RT];
#pragma unroll
  for (int q = 0; q < RT; q++) {
    best[q] = -std::numeric_limits<float>::infinity();
    bk[q] = 0;
  }

  for (int c0 = 0; c0 < Kp; c0 += CT) {
    __syncthreads();
    for (int idx = tid; idx < DP * CT; idx += TPB) {
      const int d = idx / CT, c = idx - d * CT;
      As[idx] = ct[(size_t)d * Kp + c0 + c];
    }
    if (tid < CT) Hs[tid] = hs[c0 + tid];
    __syncthreads();
    for (int t = 0; t < CT / 32; t++) {
      if (c0 + t * 32 >= K) break;       // (uniform) a sub-tile of padding only
      f32x16 acc[RT];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const float a0 = -Hs[t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h];
#pragma unroll
        for (int q = 0; q < RT; q++) acc[q][e] = a0;
      }
#pragma unroll
      for (int i = 0; i < KS; i++) {
        const float av = As[(2 * i + h) * CT + t * 32 + r];
#pragma unroll
        for (int q = 0; q < RT; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xr[q][i], acc[q], 0, 0, 0);
      }
      const int kb = c0 + t * 32 + 4 * h;
#pragma unroll
      for (int q = 0; q < RT; q++)
#pragma unroll
        for (int e = 0; e < 16; e++) {   // ascending k: the strict compare keeps the first of equal scores
          const float v = acc[q][e];
          if (v > best[q]) {
            best[q] = v;
            bk[q] = kb + (e & 3) + 8 * (e >> 2);
          }
        }
    }
  }
  // the other half-wave holds the other codes of the same data row
#pragma unroll
  for (int q = 0; q < RT; q++) {
    const float ob = __shfl_xor(best[q], 32, B3GS_WAVE);
    const int ok = __shfl_xor(bk[q], 32, B3GS_WAVE);
    if (ob > best[q] || (ob == best[q] && ok < bk[q])) bk[q] = ok;
    const int64_t row = row0 + q * 32 + r;
    if (h == 0 && row < N) codes[row] = bk[q] < K ? bk[q] : K - 1;
  }
}

// thread = code k <= K: first position of k in the sorted codes (lower bound; start[K] = N)
__global__ void __launch_bounds__(TPB) bounds_kernel(const uint32_t* __restrict__ skey, int N, int K, uint32_t* __restrict__ start) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k > K) return;
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (skey[mid] < (uint32_t)k) lo = mid + 1; else hi = mid;
  }
  start[k] = (uint32_t)lo;
}
// thread = code k < K: its number of chunks (scanned in place afterwards), and optionally its member count
__global__ void __launch_bounds__(TPB) chunk_count_kernel(const uint32_t* __restrict__ start, int K, uint32_t* __restrict__ choff,
                                                          int32_t* __restrict__ counts) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= K) return;
  const uint32_t n = start[k + 1] - start[k];
  if (choff) choff[k] = (n + CHUNK - 1) / CHUNK;
  if (counts) counts[k] = (int32_t)n;
}
__global__ void __launch_bounds__(B3GS_SCAN_TPB) chunk_scan_kernel(uint32_t* choff, int K, uint32_t* total) {
  b3gs_scan_block_sums(choff, K, total);
}

// wave = chunk g of the scanned chunk table; lane d < D sums dimension d, lane D the weights, in member order
__global__ void __launch_bounds__(TPB) chunk_sum_kernel(int D, int K, const float* __restrict__ x, const float* __restrict__ w,
                                                        const uint32_t* __restrict__ sval, const uint32_t* __restrict__ start,
                                                        const uint32_t* __restrict__ choff, const uint32_t* __restrict__ total,
                                                        uint32_t max_chunks, double* __restrict__ part) {
  const uint32_t g = blockIdx.x * (TPB / B3GS_WAVE) + threadIdx.x / B3GS_WAVE;
  const int lane = threadIdx.x & (B3GS_WAVE - 1);
  if (g >= *total || g >= max_chunks) return;
  // the last k with choff[k] <= g: codes without a chunk share their successor's offset
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (choff[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t m0 = start[lo] + (g - choff[lo]) * CHUNK;
  const uint32_t m1 = min(m0 + (uint32_t)CHUNK, start[lo + 1]);
  for (int d = lane; d <= D; d += B3GS_WAVE) {     // (D == 64: lane 0 takes the weights in a second turn)
    double s = 0.0;
    for (uint32_t m = m0; m < m1; m++) {
      const uint32_t row = sval[m];
      const double wn = w ? (double)w[row] : 1.0;
      s += d < D ? wn * (double)x[(size_t)row * D + d] : wn;
    }
    part[(size_t)g * (D + 1) + d] = s;
  }
}

// thread = (code, dimension): the chunk sums in order, then the centroid
__global__ void __launch_bounds__(TPB) centroid_kernel(int D, int K, const uint32_t* __restrict__ start, const uint32_t* __restrict__ choff,
                                                       const double* __restrict__ part, float* __restrict__ cb) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= (int64_t)K * D) return;
  const int k = (int)(i / D), d = (int)(i - (int64_t)k * D);
  const uint32_t n = start[k + 1] - start[k];
  const uint32_t nch = (n + CHUNK - 1) / CHUNK, g0 = choff[k];
  double S = 0.0, W = 0.0;
  for (uint32_t j = 0; j < nch; j++) {
    S += part[(size_t)(g0 + j) * (D + 1) + d];
    W += part[(size_t)(g0 + j) * (D + 1) + D];
  }
  if (n > 0 && W != 0.0) cb[i] = (float)(S / W);
}

__global__ void __launch_bounds__(TPB) distortion_partial_kernel(int N, int D, const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ cb, const int32_t* __restrict__ codes,
                                                                 double* __restrict__ part) {
  double s = 0.0;
  for (int64_t n = (int64_t)blockIdx.x * TPB + threadIdx.x; n < N; n += (int64_t)gridDim.x * TPB) {
    const float* __restrict__ xp = x + (size_t)n * D;
    const float* __restrict__ cp = cb + (size_t)codes[n] * D;
    double a = 0.0;
    for (int d = 0; d < D; d++) {
      const double df = (double)xp[d] - (double)cp[d];
      a += df * df;
    }
    s += (w ? (double)w[n] : 1.0) * a;
  }
  __shared__ double red[TPB / B3GS_WAVE][1];
  const double q[1] = {s};
  b3gs_block_sum_f64<TPB>(q, red, part + blockIdx.x);
}
__global__ void __launch_bounds__(B3GS_WAVE) distortion_fold_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  const double a = b3gs_wave_fold_f64(part, nb, 1);
  if (threadIdx.x == 0) *out = a;
}

struct Ws {
  float* ct;            // [Dp][Kp]
  float* h;             // [Kp]
  uint32_t* skey[2];    // [N]
  uint32_t* sval[2];    // [N]
  uint32_t* hist;       // sort scratch
  uint32_t* start;      // [K + 1]
  uint32_t* choff;      // [K] + the total
  double* part;         // [max_chunks][D + 1]
  double* dpart;        // [DBLOCKS]
  uint32_t max_chunks;
};
static size_t carve(char* base, int32_t N, int32_t D, int32_t K, Ws* out) {
  char* cur = base;
  const size_t n = (size_t)(N > 0 ? N : 1), Kp = (size_t)padded_codes(K), Dp = 2 * (size_t)ksteps_of(D);
  Ws w;
  w.ct = b3gs_carve<float>(cur, Dp * Kp);
  w.h = b3gs_carve<float>(cur, Kp);
  for (int i = 0; i < 2; i++) w.skey[i] = b3gs_carve<uint32_t>(cur, n);
  for (int i = 0; i < 2; i++) w.sval[i] = b3gs_carve<uint32_t>(cur, n);
  w.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)n));
  w.start = b3gs_carve<uint32_t>(cur, (size_t)K + 1);
  w.choff = b3gs_carve<uint32_t>(cur, (size_t)K + 1);
  // sum_k ceil(n_k / CHUNK) <= N / CHUNK + (codes with a member)
  w.max_chunks = (uint32_t)(n / CHUNK + ((size_t)K < n ? (size_t)K : n));
  w.part = b3gs_carve<double>(cur, (size_t)w.max_chunks * (D + 1));
  w.dpart = b3gs_carve<double>(cur, DBLOCKS);
  if (out) *out = w;
  return (size_t)(cur - base);
}

static unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

static void launch_assign(int N, int D, int K, const float* x, const float* cb, int32_t* codes, const Ws& w, hipStream_t s) {
  const int KS = ksteps_of(D), Kp = padded_codes(K);
  hipLaunchKernelGGL(prep_kernel, dim3(blocks_of(Kp)), dim3(TPB), 0, s, cb, D, K, 2 * KS, Kp, w.ct, w.h);
  const dim3 grid((unsigned)(((int64_t)N + ROWS - 1) / ROWS));
#define B3GS_KMEANS_ASSIGN(KS_) \
  hipLaunchKernelGGL((assign_kernel<KS_>), grid, dim3(TPB), 0, s, N, D, K, Kp, x, (const float*)w.ct, (const float*)w.h, codes)
  switch (KS) {
    case 4: B3GS_KMEANS_ASSIGN(4); break;
    case 6: B3GS_KMEANS_ASSIGN(6); break;
    case 8: B3GS_KMEANS_ASSIGN(8); break;
    case 16: B3GS_KMEANS_ASSIGN(16); break;
    case 24: B3GS_KMEANS_ASSIGN(24); break;
    default: B3GS_KMEANS_ASSIGN(32); break;
  }
#undef B3GS_KMEANS_ASSIGN
}

// sorted codes, segment starts; update: the chunk table too
static void launch_segments(int N, int K, const int32_t* codes, const Ws& w, bool chunks, int32_t* counts, hipStream_t s) {
  b3gs_launch_sort_u32_index(reinterpret_cast<const uint32_t*>(codes), w.skey, w.sval, (uint32_t)N, w.hist, s);
  hipLaunchKernelGGL(bounds_kernel, dim3(blocks_of(K + 1)), dim3(TPB), 0, s, (const uint32_t*)w.skey[0], N, K, w.start);
  hipLaunchKernelGGL(chunk_count_kernel, dim3(blocks_of(K)), dim3(TPB), 0, s, (const uint32_t*)w.start, K, chunks ? w.choff : nullptr,
                     counts);
  if (chunks) hipLaunchKernelGGL(chunk_scan_kernel, dim3(1), dim3(B3GS_SCAN_TPB), 0, s, w.choff, K, w.choff + K);
}

static void launch_update(int N, int D, int K, const float* x, const float* wt, float* cb, const int32_t* codes, const Ws& w,
                          hipStream_t s) {
  launch_segments(N, K, codes, w, true, nullptr, s);
  const unsigned waves = TPB / B3GS_WAVE;
  hipLaunchKernelGGL(chunk_sum_kernel, dim3((w.max_chunks + waves - 1) / waves), dim3(TPB), 0, s, D, K, x, wt,
                     (const uint32_t*)w.sval[0], (const uint32_t*)w.start, (const uint32_t*)w.choff, (const uint32_t*)(w.choff + K),
                     w.max_chunks, w.part);
  hipLaunchKernelGGL(centroid_kernel, dim3(blocks_of((int64_t)K * D)), dim3(TPB), 0, s, D, K, (const uint32_t*)w.start,
                     (const uint32_t*)w.choff, (const double*)w.part, cb);
}

static void launch_distortion(int N, int D, const float* x, const float* wt, const float* cb, const int32_t* codes, const Ws& w,
                              double* out, hipStream_t s) {
  const int64_t b = ((int64_t)N + TPB - 1) / TPB;
  const int nb = (int)(b > DBLOCKS ? DBLOCKS : b);
  hipLaunchKernelGGL(distortion_partial_kernel, dim3(nb), dim3(TPB), 0, s, N, D, x, wt, cb, codes, w.dpart);
  hipLaunchKernelGGL(distortion_fold_kernel, dim3(1), dim3(B3GS_WAVE), 0, s, (const double*)w.dpart, nb, out);
}

static const char* check_shape(int32_t N, int32_t D, int32_t K) {
  if (N < 0) return "N must not be negative";
  if (D < 1 || D > MAXD) return "1 <= D <= 64";
  if (K < 1 || K > MAXK) return "1 <= K <= 65536";
  return nullptr;
}

}  // namespace

extern "C" size_t b3gs_kmeans_workspace_bytes(int32_t N, int32_t D, int32_t K) {
  if (check_shape(N, D, K)) return 0;
  return carve(nullptr, N, D, K, nullptr);
}

extern "C" int b3gs_kmeans_assign(int32_t N, int32_t D, int32_t K, const float* x, const float* codebook, int32_t* codes,
                                  void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_kmeans_assign";
  if (const char* msg = check_shape(N, D, K)) return b3gs_fail(B3GS_ERR_ARG, what, msg);
  if (N == 0) return B3GS_OK;
  if (!x || !codebook || !codes || !workspace) return b3gs_fail(B3GS_ERR_ARG, what, "NULL x, codebook, codes or workspace");
  if ((uintptr_t)workspace & 255) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  Ws w;
  carve(static_cast<char*>(workspace), N, D, K, &w);
  launch_assign(N, D, K, x, codebook, codes, w, (hipStream_t)stream);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_kmeans(int32_t N, int32_t D, int32_t K, int32_t iters, const float* x, const float* weights, float* codebook,
                           int32_t* codes, int32_t* counts, double* distortion, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_kmeans";
  if (const char* msg = check_shape(N, D, K)) return b3gs_fail(B3GS_ERR_ARG, what, msg);
  if (iters < 0) return b3gs_fail(B3GS_ERR_ARG, what, "iters must not be negative");
  if (N == 0) return B3GS_OK;
  if (!x || !codebook || !codes || !counts || !distortion || !workspace)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL x, codebook, codes, counts, distortion or workspace");
  if ((uintptr_t)workspace & 255) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  Ws w;
  carve(static_cast<char*>(workspace), N, D, K, &w);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0;; i++) {
    launch_assign(N, D, K, x, codebook, codes, w, s);
    launch_distortion(N, D, x, weights, codebook, codes, w, distortion + i, s);
    if (i == iters) break;
    launch_update(N, D, K, x, weights, codebook, codes, w, s);
  }
  launch_segments(N, K, codes, w, false, counts, s);
  return b3gs_launch_status(what);
}
