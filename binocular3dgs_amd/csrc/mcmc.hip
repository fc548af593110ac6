// Fixed-budget training (added to ABI 18; binocular3dgs_amd/mcmc.py): Philox4x32-10, the position
// noise of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., NeurIPS 2024) and its relocation of dead
// Gaussians.  include/b3gs_raster.h states every rule; tests/mcmc_ref.py restates them in numpy and Python integers.
//   random     thread = one counter block = four output words
//   noise      thread = Gaussian: 11 floats in, 3 out, float32, the normals made in registers (two counter blocks at most)
//   relocate   classify (workgroup = 64 rows: local ranks and weight sums) -> scan of the block sums (ONE workgroup of 1024:
//              b3gs_scan_block_sums for the 32-bit dead counts, b3gs_block_exscan with a carry for the 64-bit weights) -> finish
//              (global ranks / inclusive weights) -> sample (binary search, one integer atomicAdd per dead row) -> correct (fp64,
//              into scratch rows) -> apply.  Correct and apply are two launches: a dead row reads its source's new opacity, which
//              the source itself replaces.  Apply only COPIES rows: lane w moves word w of the workgroup's block of features_rest
//              (the word-per-lane walk of edit.hip and lod.hip; a copy needs no LDS row in between), reads of a source row are
//              one contiguous run.  Nobody reads a row that anybody writes: sources are alive, and only xyz / rotation / features
//              of DEAD rows are written.
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int ROWS = 64;              // rows per workgroup of the scans: 64 * 2^24 fits a 32-bit partial with room
constexpr int NMAX = B3GS_MCMC_MAX_N;
constexpr int HEAD_WORDS = 32;        // int64: total weight, dead rows, status
enum { H_TOTAL = 0, H_DEAD = 1, H_STATUS = 2 };

static inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------
struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox(uint32_t index, uint32_t offset, uint32_t stream_id, uint64_t seed) {
  uint32_t c0 = index, c1 = offset, c2 = stream_id, c3 = 0u;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return Words{{c0, c1, c2, c3}};
}

// Box-Muller on one word pair, in fp64, ONE rounding to float32 per output
__device__ __forceinline__ void normal_pair(uint32_t a, uint32_t b, float* c, float* s) {
  const double u1 = ((double)a + 0.5) * 0x1p-32, u2 = ((double)b + 0.5) * 0x1p-32;
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  *c = (float)(r * cs), *s = (float)(r * sn);
}

__global__ void __launch_bounds__(TPB) random_kernel(int64_t n, uint64_t seed, uint32_t stream_id, uint32_t offset, int32_t kind,
                                                     uint32_t* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t e0 = 4 * b;
  if (e0 >= n) return;
  const Words x = philox((uint32_t)b, offset, stream_id, seed);
  uint32_t v[4];
  if (kind == B3GS_RANDOM_NORMAL) {
    float f[4];
    normal_pair(x.w[0], x.w[1], &f[0], &f[1]);
    normal_pair(x.w[2], x.w[3], &f[2], &f[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = __float_as_uint(f[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = x.w[k];
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (e0 + k < n) out[e0 + k] = v[k];
}

// elements 3 i, 3 i + 1, 3 i + 2 of the normal stream: two word pairs, one or two blocks
__device__ __forceinline__ void row_normals(int64_t i, uint64_t seed, uint32_t offset, float* n) {
  const uint64_t e0 = 3ull * (uint64_t)i;
  const uint64_t pa = e0 >> 1, pb = pa + 1ull;
  const uint32_t ba = (uint32_t)(pa >> 1), bb = (uint32_t)(pb >> 1);
  const Words xa = philox(ba, offset, 0u, seed);
  Words xb = xa;
  if (bb != ba) xb = philox(bb, offset, 0u, seed);
  const int wa = (int)(pa & 1ull) * 2, wb = (int)(pb & 1ull) * 2;
  float ca, sa, cb, sb;
  normal_pair(wa ? xa.w[2] : xa.w[0], wa ? xa.w[3] : xa.w[1], &ca, &sa);
  normal_pair(wb ? xb.w[2] : xb.w[0], wb ? xb.w[3] : xb.w[1], &cb, &sb);
  if (e0 & 1ull) n[0] = sa, n[1] = cb, n[2] = sb;
  else n[0] = ca, n[1] = sa, n[2] = cb;
}

// ---- the position noise ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) noise_kernel(int32_t P, const float* __restrict__ scaling, const float* __restrict__ rotation,
                                                    const float* __restrict__ opacity, float* __restrict__ xyz,
                                                    const float* __restrict__ normals, uint64_t seed, uint32_t iteration, float noise_lr,
                                                    float lr_xyz, const float* __restrict__ lr_dev) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= P) return;
  const float lr = lr_dev ? *lr_dev : lr_xyz;
  float n[3];
  if (normals) n[0] = normals[3 * i], n[1] = normals[3 * i + 1], n[2] = normals[3 * i + 2];
  else row_normals(i, seed, iteration, n);
  float w = rotation[4 * i], x = rotation[4 * i + 1], y = rotation[4 * i + 2], z = rotation[4 * i + 3];
  const float qn = sqrtf(((w * w + x * x) + y * y) + z * z);
  w = w / qn, x = x / qn, y = y / qn, z = z / qn;
  const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - w * z), 2.0f * (x * z + w * y)},
                         {2.0f * (x * y + w * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - w * x)},
                         {2.0f * (x * z - w * y), 2.0f * (y * z + w * x), 1.0f - 2.0f * (x * x + y * y)}};
  float t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float s = expf(scaling[3 * i + k]);
    const float v = s * s;
    t[k] = ((R[0][k] * n[0] + R[1][k] * n[1]) + R[2][k] * n[2]) * v;
  }
  const float o = 1.0f / (1.0f + expf(-opacity[i]));
  const float g = 1.0f / (1.0f + expf(100.0f * (o - 0.005f)));
  const float step = noise_lr * lr;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const float d = (R[j][0] * t[0] + R[j][1] * t[1]) + R[j][2] * t[2];
    xyz[3 * i + j] = xyz[3 * i + j] + (d * g) * step;
  }
}

// ---- relocation ------------------------------------------------------------------------------------------------------------
struct Ws {
  int64_t* head;
  int32_t *src, *count, *rank;
  uint64_t* wsum;
  float* fresh;                       // [P][4] corrected raw opacity, raw scaling
  uint8_t* dead;
  uint32_t* bdead;                    // [nb]
  uint64_t* bw;                       // [nb]
};

static size_t carve_ws(char* base, int32_t P, Ws* out) {
  char* cur = base;
  const size_t p = (size_t)(P > 0 ? P : 1), nb = blocks_of((int64_t)p, ROWS);
  Ws w;
  w.head = b3gs_carve<int64_t>(cur, HEAD_WORDS);
  w.src = b3gs_carve<int32_t>(cur, p);
  w.count = b3gs_carve<int32_t>(cur, p);
  w.rank = b3gs_carve<int32_t>(cur, p);
  w.wsum = b3gs_carve<uint64_t>(cur, p);
  w.fresh = b3gs_carve<float>(cur, 4 * p);
  w.dead = b3gs_carve<uint8_t>(cur, p);
  w.bdead = b3gs_carve<uint32_t>(cur, nb);
  w.bw = b3gs_carve<uint64_t>(cur, nb);
  if (out) *out = w;
  return (size_t)(cur - base);
}

__device__ __forceinline__ double sigmoid64(float raw) { return 1.0 / (1.0 + exp(-(double)raw)); }

__global__ void __launch_bounds__(ROWS) classify_kernel(int32_t P, int32_t P_old, float min_opacity, const float* __restrict__ opacity, Ws ws) {
  __shared__ uint32_t wave_d[ROWS / B3GS_WAVE];
  __shared__ unsigned long long wave_w[ROWS / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * ROWS + threadIdx.x;
  uint32_t dead = 0u, q = 0u;
  if (i < P) {
    const double o = sigmoid64(opacity[i]);
    dead = (o <= (double)min_opacity || i >= P_old) ? 1u : 0u;      // (a NaN opacity compares false: alive, weight 0)
    q = dead ? 0u : (uint32_t)(o * 16777216.0);
  }
  uint32_t nd;
  unsigned long long nw;
  const uint32_t before = b3gs_block_exscan<ROWS>(dead, wave_d, &nd);
  const unsigned long long wb = b3gs_block_exscan<ROWS>((unsigned long long)q, wave_w, &nw);
  if (i < P) {
    ws.dead[i] = (uint8_t)dead;
    ws.rank[i] = (int32_t)before;
    ws.wsum[i] = wb + q;
    ws.src[i] = -1;
    ws.count[i] = 0;
  }
  if (threadIdx.x == 0) ws.bdead[blockIdx.x] = nd, ws.bw[blockIdx.x] = nw;
}

__global__ void __launch_bounds__(B3GS_SCAN_TPB) scan_kernel(int nb, Ws ws) {
  b3gs_scan_block_sums(ws.bdead, nb, ws.head + H_DEAD);
  // the same walk for the 64-bit weight sums
  __shared__ unsigned long long wave_n[B3GS_SCAN_TPB / B3GS_WAVE];
  unsigned long long carry = 0ull;
  for (int b0 = 0; b0 < nb; b0 += B3GS_SCAN_TPB) {
    const int b = b0 + threadIdx.x;
    unsigned long long chunk;
    const unsigned long long before = b3gs_block_exscan<B3GS_SCAN_TPB>(b < nb ? (unsigned long long)ws.bw[b] : 0ull, wave_n, &chunk);
    if (b < nb) ws.bw[b] = carry + before;
    carry += chunk;
  }
  if (threadIdx.x == 0) {
    ws.head[H_TOTAL] = (int64_t)carry;
    ws.head[H_STATUS] = carry == 0ull ? 1 : 0;
  }
}

__global__ void __launch_bounds__(ROWS) finish_kernel(int32_t P, Ws ws) {
  const int64_t i = (int64_t)blockIdx.x * ROWS + threadIdx.x;
  if (i >= P) return;
  ws.rank[i] += (int32_t)ws.bdead[blockIdx.x];
  ws.wsum[i] += ws.bw[blockIdx.x];
}

__global__ void __launch_bounds__(TPB) sample_kernel(int32_t P, uint64_t seed, uint32_t offset, const uint64_t* __restrict__ draws, Ws ws) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= P || !ws.dead[i]) return;
  const uint64_t total = (uint64_t)ws.head[H_TOTAL];
  if (total == 0ull) return;
  const uint32_t j = (uint32_t)ws.rank[i];
  uint64_t u;
  if (draws) u = draws[j];                                           // (j < P: a rank)
  else {
    const Words x = philox(j, offset, 1u, seed);
    u = (uint64_t)x.w[0] | ((uint64_t)x.w[1] << 32);
  }
  const uint64_t t = __umul64hi(u, total);                           // < total
  int64_t lo = 0, hi = (int64_t)P - 1;                               // the first row with W > t (W_(P-1) = total > t)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ws.wsum[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  ws.src[i] = (int32_t)lo;
  atomicAdd(&ws.count[lo], 1);
}

// C(n, k), n <= 50: exact in fp64 (C(50, 25) < 2^47)
struct Binomials {
  double c[NMAX][NMAX];
  constexpr Binomials() : c{} {
    for (int n = 0; n < NMAX; n++) {
      c[n][0] = 1.0;
      for (int k = 1; k <= n; k++) c[n][k] = c[n - 1][k - 1] + (k <= n - 1 ? c[n - 1][k] : 0.0);
    }
  }
};
__device__ const Binomials BINOM = Binomials();

__global__ void __launch_bounds__(TPB) correct_kernel(int32_t P, int32_t n_max, float min_opacity, const float* __restrict__ opacity,
                                                      const float* __restrict__ scaling, Ws ws) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= P || ws.dead[i]) return;
  const int32_t cnt = ws.count[i];
  if (cnt <= 0) return;
  const int N = cnt + 1 < n_max ? cnt + 1 : n_max;
  const double o = sigmoid64(opacity[i]);
  const double inv = 1.0 / (double)N;
  const double rem = 1.0 - o;
  double on = 1.0 - pow(rem, inv);
  double denom = 0.0;
  for (int a = 1; a <= N; a++) {
    double p = on;
    for (int k = 0; k < a; k++) {
      const double num = BINOM.c[a - 1][k] * p;
      const double term = num / sqrt((double)(k + 1));
      denom = (k & 1) ? denom - term : denom + term;
      p = p * on;
    }
  }
  const double lo = (double)min_opacity, hi = 1.0 - 0x1p-24;
  on = on < lo ? lo : (on > hi ? hi : on);
  ws.fresh[4 * i] = (float)log(on / (1.0 - on));
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double s = exp((double)scaling[3 * i + k]);
    ws.fresh[4 * i + 1 + k] = (float)log((s * o) / denom);
  }
}

struct Rows {
  float* p[6];                        // xyz, features_dc, features_rest, scaling, rotation, opacity
  float* m[6];
  float* v[6];
};

__global__ void __launch_bounds__(TPB) apply_kernel(int32_t P, int32_t K, Rows r, Ws ws) {
  // what[t]: -2 the row stays, -1 an alive source (new opacity and scaling), >= 0 a dead row's source
  __shared__ int32_t what[TPB];
  const int64_t g0 = (int64_t)blockIdx.x * TPB;
  const int64_t i = g0 + threadIdx.x;
  const bool moments = r.m[0] != nullptr;
  int32_t act = -2;
  if (i < P && ws.head[H_TOTAL] != 0) {
    if (ws.dead[i]) {
      const int32_t s = ws.src[i];
      act = (s >= 0 && s < P) ? s : -2;
    } else if (ws.count[i] > 0) act = -1;
  }
  what[threadIdx.x] = act;
  if (act != -2) {
    const int64_t s = act >= 0 ? act : i;
    if (act >= 0) {
#pragma unroll
      for (int k = 0; k < 3; k++) r.p[0][3 * i + k] = r.p[0][3 * s + k], r.p[1][3 * i + k] = r.p[1][3 * s + k];
#pragma unroll
      for (int k = 0; k < 4; k++) r.p[4][4 * i + k] = r.p[4][4 * s + k];
    }
    r.p[5][i] = ws.fresh[4 * s];
#pragma unroll
    for (int k = 0; k < 3; k++) r.p[3][3 * i + k] = ws.fresh[4 * s + 1 + k];
    if (moments) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        r.m[0][3 * i + k] = 0.0f, r.v[0][3 * i + k] = 0.0f, r.m[1][3 * i + k] = 0.0f, r.v[1][3 * i + k] = 0.0f;
        r.m[3][3 * i + k] = 0.0f, r.v[3][3 * i + k] = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; k++) r.m[4][4 * i + k] = 0.0f, r.v[4][4 * i + k] = 0.0f;
      r.m[5][i] = 0.0f, r.v[5][i] = 0.0f;
    }
  }
  if (K <= 0) return;                                               // (uniform)
  __syncthreads();
  const int64_t left = (int64_t)P - g0;
  const int64_t nwords = (left < TPB ? left : (int64_t)TPB) * K;
  float* rest = r.p[2];
  for (int64_t w = threadIdx.x; w < nwords; w += TPB) {
    const int rl = (int)(w / K), ch = (int)(w % K);
    const int32_t a = what[rl];
    if (a == -2) continue;
    const size_t at = (size_t)(g0 + rl) * K + ch;
    if (a >= 0) rest[at] = rest[(size_t)a * K + ch];
    if (moments) r.m[2][at] = 0.0f, r.v[2][at] = 0.0f;
  }
}

static bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }

}  // namespace

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
extern "C" int b3gs_mcmc_random(int64_t n, uint64_t seed, uint32_t stream_id, uint32_t offset, int32_t kind, void* out, b3gs_stream_t stream) {
  static const char* what = "b3gs_mcmc_random";
  if (n < 0 || n > ((int64_t)1 << 32)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= n <= 2^32");
  if (kind != B3GS_RANDOM_U32 && kind != B3GS_RANDOM_NORMAL) return b3gs_fail(B3GS_ERR_ARG, what, "kind is B3GS_RANDOM_U32 or B3GS_RANDOM_NORMAL");
  if (n == 0) return B3GS_OK;
  if (!out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  hipLaunchKernelGGL(random_kernel, dim3(blocks_of((n + 3) / 4, TPB)), dim3(TPB), 0, (hipStream_t)stream, n, seed, stream_id, offset, kind,
                     static_cast<uint32_t*>(out));
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mcmc_noise(int32_t P, const float* scaling, const float* rotation, const float* opacity, float* xyz, const float* normals,
                               uint64_t seed, uint32_t iteration, float noise_lr, float lr_xyz, const float* lr_xyz_dev, b3gs_stream_t stream) {
  static const char* what = "b3gs_mcmc_noise";
  if (P < 0) return b3gs_fail(B3GS_ERR_ARG, what, "P >= 0");
  if (noise_lr != noise_lr || (!lr_xyz_dev && lr_xyz != lr_xyz)) return b3gs_fail(B3GS_ERR_ARG, what, "a learning rate is NaN");
  if (P == 0) return B3GS_OK;
  if (!scaling || !rotation || !opacity || !xyz) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  hipLaunchKernelGGL(noise_kernel, dim3(blocks_of(P, TPB)), dim3(TPB), 0, (hipStream_t)stream, P, scaling, rotation, opacity, xyz, normals, seed,
                     iteration, noise_lr, lr_xyz, lr_xyz_dev);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_mcmc_workspace_bytes(int32_t P) {
  if (P < 1) return 0;
  return carve_ws(nullptr, P, nullptr);
}

extern "C" int b3gs_mcmc_views(int32_t P, void* workspace, B3gsMcmcViews* out) {
  static const char* what = "b3gs_mcmc_views";
  if (P < 1) return b3gs_fail(B3GS_ERR_ARG, what, "P >= 1");
  if (!out || !aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
  Ws ws;
  carve_ws(static_cast<char*>(workspace), P, &ws);
  out->src = ws.src, out->count = ws.count, out->rank = ws.rank, out->weight_scan = ws.wsum, out->head = ws.head;
  return B3GS_OK;
}

extern "C" int b3gs_mcmc_relocate(const B3gsMcmcIO* io, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_mcmc_relocate";
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  const int32_t P = io->P, K = io->K;
  if (P < 0 || io->P_old < 0 || io->P_old > P) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= P_old <= P");
  if (K < 0 || K > 1024) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= K <= 1024");
  if (io->n_max < 1 || io->n_max > NMAX) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_max <= 51");
  if (!(io->min_opacity > 0.0f && io->min_opacity < 1.0f)) return b3gs_fail(B3GS_ERR_ARG, what, "min_opacity is in (0, 1)");
  if (P == 0) return B3GS_OK;
  bool any = false, all = true;
  for (int t = 0; t < 6; t++) {
    if (t == 2 && K == 0) continue;
    if (!io->param[t]) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    any = any || io->exp_avg[t] || io->exp_avg_sq[t];
    all = all && io->exp_avg[t] && io->exp_avg_sq[t];
  }
  if (any && !all) return b3gs_fail(B3GS_ERR_ARG, what, "the Adam moments: all of them, or none");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
  Ws ws;
  carve_ws(static_cast<char*>(workspace), P, &ws);
  Rows r;
  for (int t = 0; t < 6; t++) r.p[t] = io->param[t], r.m[t] = all ? io->exp_avg[t] : nullptr, r.v[t] = all ? io->exp_avg_sq[t] : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)blocks_of(P, ROWS);
  hipLaunchKernelGGL(classify_kernel, dim3(nb), dim3(ROWS), 0, s, P, io->P_old, io->min_opacity, (const float*)io->param[5], ws);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(B3GS_SCAN_TPB), 0, s, nb, ws);
  hipLaunchKernelGGL(finish_kernel, dim3(nb), dim3(ROWS), 0, s, P, ws);
  hipLaunchKernelGGL(sample_kernel, dim3(blocks_of(P, TPB)), dim3(TPB), 0, s, P, io->seed, io->offset, io->draws, ws);
  hipLaunchKernelGGL(correct_kernel, dim3(blocks_of(P, TPB)), dim3(TPB), 0, s, P, io->n_max, io->min_opacity, (const float*)io->param[5],
                     (const float*)io->param[3], ws);
  hipLaunchKernelGGL(apply_kernel, dim3(blocks_of(P, TPB)), dim3(TPB), 0, s, P, K, r, ws);
  return b3gs_launch_status(what);
}
