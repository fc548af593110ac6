// Merging Gaussians into moment-matched levels of detail (added to ABI 18; binocular3dgs_amd/lod.py).
// include/b3gs_raster.h states the rule statement by statement; tests/lod_ref.py restates it.  Every step is integer work, a
// stable sort, an ordered scan, one correctly rounded float32 operation per statement, or fp64 statements (+ - * / sqrt and
// comparisons; the library is built with -ffp-contract=off) executed by ONE thread in one fixed order: one fixed result.
//   count   finite    thread = word of features_rest: a row with a value that is not finite is flagged
//           bbox      partial minima / maxima per workgroup; rows that are not finite counted (each once)
//           origin    one wave folds the partials: origin and extent -> the head of the workspace
//           keys      thread = Gaussian: the cell key, NO_KEY for one that is not mergeable; rows past cell 1023 counted
//           sort      the project's radix sort (stable): members of a cluster stay in index order, the pass-throughs
//                     (NO_KEY) follow all clusters in index order
//           rows      head flags (every NO_KEY position is a head) -> block sums -> scan -> output row per Gaussian, first
//                     sorted position per row
//           members   thread = row: rows of two members or more add their size to the merged-member total
//   emit    moments   thread = row: one member -> a copy of its words; more -> the statements of the rule, members in order;
//                     the mass of every member and of the row go to the workspace for the colour kernel
//           colour    workgroup = 32 consecutive rows, whose members are ONE run of the sorted order: 64 members at a time,
//                     their features_dc / features_rest rows (12 .. 192 contiguous bytes each) are gathered into LDS by all
//                     256 threads, word by word (consecutive lanes, consecutive words of a row), then thread = (row, channel)
//                     adds its members of the chunk in order.  Row stride in LDS: channels | 1 words (odd).
#include "b3gs_internal.h"
#include <cfloat>
#include <cstdio>

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int MAX_DIM = 1024;                  // cells per axis: 10 bits of the key
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;       // a Gaussian that is not mergeable (cell keys stay below 2^30)
constexpr int MAX_PARTS = 256;
constexpr int SWEEPS = B3GS_MERGE_JACOBI_SWEEPS;
constexpr int ROWS_PER_BLOCK = 32;             // colour kernel
constexpr int CHUNK = 64;                      // members staged at a time

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// words of the totals (int64 each) at the head of the workspace; the first five are the public ones
enum { T_CLUSTERS = 0, T_PASS, T_MERGED, T_NONFINITE, T_OVER, T_ROWS, T_EXTENT_BITS, T_WORDS };

struct LGrid {                      // behind the totals (byte 128 of the workspace), written by origin_kernel
  float o[3];
  float extent;
};

struct LodWs {
  int64_t* totals;
  LGrid* grid;
  float* part;                      // [MAX_PARTS][6]
  uint32_t* skey[2];                // [P] sort ping / pong; skey[0], sval[0]: the sorted keys and their Gaussians
  uint32_t* sval[2];
  uint32_t* hist;
  uint32_t* vkey;                   // [P] cell key, or NO_KEY
  int32_t* vrow;                    // [P] output row per Gaussian
  uint32_t* cstart;                 // [P + 1] first sorted position of every row; cstart[rows] = P
  uint32_t* bsum;                   // [nb] head flags
  uint8_t* bad;                     // [P] features_rest of the row holds a value that is not finite
  double* mass;                     // [P] emit: m_i per sorted position (rows of two members or more)
  double* row_mass;                 // [P] emit: M per row
};

static size_t lod_carve(char* base, int64_t P, LodWs* w) {
  char* cur = base;
  const size_t p = (size_t)(P > 0 ? P : 1);
  LodWs t;
  t.totals = b3gs_carve<int64_t>(cur, 16);                         // 128 bytes, then the grid: one 256-byte head
  cur = base + 128;
  t.grid = b3gs_carve<LGrid>(cur, 1);
  cur = base + 256;
  t.part = b3gs_carve<float>(cur, 6 * MAX_PARTS);
  for (int k = 0; k < 2; k++) t.skey[k] = b3gs_carve<uint32_t>(cur, p);
  for (int k = 0; k < 2; k++) t.sval[k] = b3gs_carve<uint32_t>(cur, p);
  t.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)p));
  t.vkey = b3gs_carve<uint32_t>(cur, p);
  t.vrow = b3gs_carve<int32_t>(cur, p);
  t.cstart = b3gs_carve<uint32_t>(cur, p + 1);
  t.bsum = b3gs_carve<uint32_t>(cur, blocks_of((int64_t)p));
  t.bad = b3gs_carve<uint8_t>(cur, p);
  t.mass = b3gs_carve<double>(cur, p);
  t.row_mass = b3gs_carve<double>(cur, p);
  if (w) *w = t;
  return (size_t)(cur - base);
}

__device__ __forceinline__ void count_up(int64_t* word, unsigned long long n) {
  if (n) atomicAdd(reinterpret_cast<unsigned long long*>(word), n);
}
// every lane of the wave calls: the number of lanes with `flag` set goes to *word by one integer atomic
__device__ __forceinline__ void count_flags(int64_t* word, bool flag) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0) count_up(word, (unsigned long long)__popcll(m));
}
__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= FLT_MAX; }    // (false for NaN and either infinity)

struct InArgs {
  int32_t P, C;                     // C: floats of one features_rest row (0, 9, 24, 45)
  const float *pos, *scale, *quat, *alpha, *dc, *rest;
  const double* weight;             // or NULL
};

// ---- the grid ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) lod_rest_finite_kernel(int64_t nwords, int32_t C, const float* __restrict__ rest, uint8_t* bad) {
  const int64_t w = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (w >= nwords) return;
  if (!finite32(rest[w])) bad[w / C] = 1;                           // (the same byte from every writer)
}

__global__ void __launch_bounds__(TPB) lod_bbox_kernel(InArgs a, const uint8_t* __restrict__ bad, float* __restrict__ part, int64_t* totals) {
  __shared__ float red[TPB / 64][6];
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  unsigned long long nbad = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < a.P; i += (int64_t)gridDim.x * TPB) {
    bool fin = a.C > 0 ? !bad[i] : true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float v = a.pos[3 * i + k];
      fin = fin && finite32(v) && finite32(a.scale[3 * i + k]) && finite32(a.dc[3 * i + k]);
      lo[k] = fminf(lo[k], v);
      hi[k] = fmaxf(hi[k], v);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) fin = fin && finite32(a.quat[4 * i + k]);
    fin = fin && finite32(a.alpha[i]);
    if (a.weight) fin = fin && fabs(a.weight[i]) <= DBL_MAX;
    nbad += fin ? 0ull : 1ull;
  }
  nbad = b3gs_wave_sum(nbad);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0) count_up(totals + T_NONFINITE, nbad);
  const float v = b3gs_block_bbox<TPB>(lo, hi, red);
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = v;
}

__global__ void __launch_bounds__(64) lod_origin_kernel(const float* __restrict__ part, int nparts, LGrid* g, int64_t* totals) {
  __shared__ float bb[6];
  if (threadIdx.x < 6) {
    float v = part[threadIdx.x];
    for (int k = 1; k < nparts; k++) v = threadIdx.x < 3 ? fminf(v, part[k * 6 + threadIdx.x]) : fmaxf(v, part[k * 6 + threadIdx.x]);
    bb[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x) return;
  float ext = 0.0f;
  for (int k = 0; k < 3; k++) {
    g->o[k] = bb[k];
    ext = fmaxf(ext, __fsub_rn(bb[3 + k], bb[k]));
  }
  g->extent = ext;
  totals[T_EXTENT_BITS] = (int64_t)__float_as_uint(ext);
}

// the cell coordinate along one axis: two rounded float32 operations, then the floor (as in simplify.hip)
__device__ __forceinline__ float cell_coord(float x, float o, float h) { return floorf(__fdiv_rn(__fsub_rn(x, o), h)); }

__global__ void __launch_bounds__(TPB) lod_key_kernel(int32_t P, const float* __restrict__ pos, const float* __restrict__ scale,
                                                      const LGrid* __restrict__ gp, float cell, uint32_t* __restrict__ vkey, int64_t* totals) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool over = false, pass = false;
  if (i < P) {
    const LGrid g = *gp;
    uint32_t key = 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float c = cell_coord(pos[3 * i + k], g.o[k], cell);
      const bool ok = c >= 0.0f && c < (float)MAX_DIM;              // (false for NaN)
      over = over || !ok;
      key |= (ok ? (uint32_t)c : 0u) << (10 * k);
    }
    const float big = fmaxf(fmaxf(scale[3 * i], scale[3 * i + 1]), scale[3 * i + 2]);
    pass = !(big <= cell);
    vkey[i] = pass ? NO_KEY : (over ? 0u : key);
  }
  count_flags(totals + T_OVER, over);
  count_flags(totals + T_PASS, pass);
}

// ---- rows --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int head_flag(const uint32_t* __restrict__ skey, int64_t i, int32_t P) {
  if (i >= P) return 0;
  const uint32_t k = skey[i];
  return k == NO_KEY || i == 0 || k != skey[i - 1];
}

__global__ void __launch_bounds__(TPB) lod_head_count_kernel(int32_t P, const uint32_t* __restrict__ skey, uint32_t* __restrict__ bsum) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  b3gs_block_rank<TPB, 1>(head_flag(skey, i, P), wave_n, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(SCAN_TPB) lod_scan_kernel(uint32_t* bsum, int nb, int64_t* total) { b3gs_scan_block_sums(bsum, nb, total); }

// the row of sorted position i = the heads in front of it (its own included) - 1
__global__ void __launch_bounds__(TPB) lod_rows_kernel(int32_t P, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                                       const uint32_t* __restrict__ bsum, int64_t* totals, int32_t* __restrict__ vrow,
                                                       uint32_t* __restrict__ cstart) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = head_flag(skey, i, P);
  int total;
  const int64_t before = (int64_t)bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (i >= P) return;
  const int64_t r = before + flag - 1;
  const uint32_t v = sval[i];
  if (v < (uint32_t)P) vrow[v] = (int32_t)r;                        // (a permutation of 0 .. P-1: always)
  if (flag) cstart[r] = (uint32_t)i;
  if (i == 0) {
    cstart[totals[T_ROWS]] = (uint32_t)P;                           // (rows <= P: inside the P + 1 words)
    totals[T_CLUSTERS] = totals[T_ROWS] - totals[T_PASS];
  }
}

__global__ void __launch_bounds__(TPB) lod_members_kernel(int32_t P, const uint32_t* __restrict__ cstart, int64_t* totals) {
  const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
  unsigned long long n = 0ull;
  if (r < P && r < totals[T_ROWS]) {
    const uint32_t m = cstart[r + 1] - cstart[r];
    n = m >= 2u ? m : 0u;
  }
  n = b3gs_wave_sum(n);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0) count_up(totals + T_MERGED, n);
}

// ---- emit: the moments ---------------------------------------------------------------------------------------------------
struct MomentArgs {
  InArgs in;
  const int64_t* totals;
  const uint32_t* order;            // sorted position -> Gaussian
  const uint32_t* cstart;
  int64_t rows;
  double* mass;
  double* row_mass;
  float *out_pos, *out_scale, *out_quat, *out_alpha;
  int32_t* members;
};

// one Jacobi rotation in the plane (p, q); r is the third index.  Every statement is one operation.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&V)[3][3], int p, int q) {
  if (apq == 0.0) return;
  const double diff = aqq - app;
  const double den = 2.0 * apq;
  const double theta = diff / den;
  const double th2 = theta * theta;
  const double rt = sqrt(th2 + 1.0);
  const double sg = theta >= 0.0 ? 1.0 : -1.0;
  const double t = sg / (fabs(theta) + rt);
  const double t2 = t * t;
  const double c = 1.0 / sqrt(t2 + 1.0);
  const double s = t * c;
  const double tau = t * apq;
  app = app - tau;
  aqq = aqq + tau;
  apq = 0.0;
  const double rp = c * arp - s * arq;
  const double rq = s * arp + c * arq;
  arp = rp, arq = rq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double vp = c * V[k][p] - s * V[k][q];
    const double vq = s * V[k][p] + c * V[k][q];
    V[k][p] = vp, V[k][q] = vq;
  }
}

__device__ __forceinline__ void swap_columns(double (&lam)[3], double (&V)[3][3], int x, int y) {
  const double l = lam[x];
  lam[x] = lam[y], lam[y] = l;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double v = V[k][x];
    V[k][x] = V[k][y], V[k][y] = v;
  }
}

// Thread = output row; members in index order; tests/lod_ref.py walks the same statements.
__global__ void __launch_bounds__(TPB) lod_moment_kernel(MomentArgs a) {
  const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (r >= a.rows || r >= a.totals[T_ROWS]) return;                 // (the outputs hold `rows` rows)
  const InArgs& in = a.in;
  const uint32_t P = (uint32_t)in.P;
  uint32_t j0 = a.cstart[r], j1 = a.cstart[r + 1];
  if (j1 > P) j1 = P;                                               // (cstart is strictly increasing up to P: never taken)
  if (j0 >= j1) return;
  const uint32_t n = j1 - j0;
  a.members[r] = (int32_t)n;
  if (n == 1u) {
    uint32_t g = a.order[j0];
    if (g >= P) g = 0u;
    const size_t i = g;
#pragma unroll
    for (int k = 0; k < 3; k++) a.out_pos[3 * r + k] = in.pos[3 * i + k], a.out_scale[3 * r + k] = in.scale[3 * i + k];
#pragma unroll
    for (int k = 0; k < 4; k++) a.out_quat[4 * r + k] = in.quat[4 * i + k];
    a.out_alpha[r] = in.alpha[i];
    return;
  }
  // masses: a_i = alpha_i (s0 s1) s2, m_i = w_i a_i
  double sum_a = 0.0, sum_m = 0.0;
  float smin = FLT_MAX;
  for (uint32_t j = j0; j < j1; j++) {
    uint32_t g = a.order[j];
    if (g >= P) g = 0u;
    const size_t i = g;
    const float f0 = in.scale[3 * i], f1 = in.scale[3 * i + 1], f2 = in.scale[3 * i + 2];
    smin = fminf(smin, fminf(fminf(f0, f1), f2));
    const double v = ((double)f0 * (double)f1) * (double)f2;
    const double ai = (double)in.alpha[i] * v;
    sum_a = sum_a + ai;
    if (in.weight) sum_m = sum_m + in.weight[i] * ai;
  }
  const bool weighted = in.weight && sum_m != 0.0;
  const double M = weighted ? sum_m : sum_a;
  a.row_mass[r] = M;
  // first pass: the mean
  double S[3] = {0.0, 0.0, 0.0};
  for (uint32_t j = j0; j < j1; j++) {
    uint32_t g = a.order[j];
    if (g >= P) g = 0u;
    const size_t i = g;
    const double v = ((double)in.scale[3 * i] * (double)in.scale[3 * i + 1]) * (double)in.scale[3 * i + 2];
    const double ai = (double)in.alpha[i] * v;
    const double m = weighted ? in.weight[i] * ai : ai;
    a.mass[j] = m;
#pragma unroll
    for (int k = 0; k < 3; k++) S[k] = S[k] + m * (double)in.pos[3 * i + k];
  }
  const double mu[3] = {S[0] / M, S[1] / M, S[2] / M};
  // second pass: the covariance, six unique entries (00, 01, 02, 11, 12, 22)
  double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t j = j0; j < j1; j++) {
    uint32_t g = a.order[j];
    if (g >= P) g = 0u;
    const size_t i = g;
    const double m = a.mass[j];                                     // (this thread wrote it)
    double qw = in.quat[4 * i], qx = in.quat[4 * i + 1], qy = in.quat[4 * i + 2], qz = in.quat[4 * i + 3];
    const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
    qw = qw / qn, qx = qx / qn, qy = qy / qn, qz = qz / qn;
    const double R[3][3] = {{1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)},
                            {2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)},
                            {2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)}};
    double var[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double s = (double)in.scale[3 * i + k];
      var[k] = s * s;
      d[k] = (double)in.pos[3 * i + k] - mu[k];
    }
    int e = 0;
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
      for (int y = x; y < 3; y++) {
        const double cov = ((R[x][0] * var[0]) * R[y][0] + (R[x][1] * var[1]) * R[y][1]) + (R[x][2] * var[2]) * R[y][2];
        C[e] = C[e] + m * (cov + d[x] * d[y]);
        e++;
      }
  }
  double a00 = C[0] / M, a01 = C[1] / M, a02 = C[2] / M, a11 = C[3] / M, a12 = C[4] / M, a22 = C[5] / M;
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < SWEEPS; sweep++) {
    jacobi_rotate(a00, a11, a01, a02, a12, V, 0, 1);
    jacobi_rotate(a00, a22, a02, a01, a12, V, 0, 2);
    jacobi_rotate(a11, a22, a12, a01, a02, V, 1, 2);
  }
  double lam[3] = {a00, a11, a22};
  if (lam[1] > lam[0]) swap_columns(lam, V, 0, 1);                  // insertion sort, descending, ties keep column order
  if (lam[2] > lam[1]) {
    swap_columns(lam, V, 1, 2);
    if (lam[1] > lam[0]) swap_columns(lam, V, 0, 1);
  }
  const double det = (V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0])) +
                     V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  if (det < 0.0) V[0][2] = -V[0][2], V[1][2] = -V[1][2], V[2][2] = -V[2][2];
  const double fl = (double)smin * (double)smin;
  double sc[3];
#pragma unroll
  for (int k = 0; k < 3; k++) sc[k] = sqrt(lam[k] < fl ? fl : lam[k]);
  // the quaternion of V (Shepperd), normalised, w >= 0
  const double tr = (V[0][0] + V[1][1]) + V[2][2];
  double qw, qx, qy, qz;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    qw = 0.25 * s, qx = (V[2][1] - V[1][2]) / s, qy = (V[0][2] - V[2][0]) / s, qz = (V[1][0] - V[0][1]) / s;
  } else if (V[0][0] > V[1][1] && V[0][0] > V[2][2]) {
    const double s = sqrt(((1.0 + V[0][0]) - V[1][1]) - V[2][2]) * 2.0;
    qw = (V[2][1] - V[1][2]) / s, qx = 0.25 * s, qy = (V[0][1] + V[1][0]) / s, qz = (V[0][2] + V[2][0]) / s;
  } else if (V[1][1] > V[2][2]) {
    const double s = sqrt(((1.0 + V[1][1]) - V[0][0]) - V[2][2]) * 2.0;
    qw = (V[0][2] - V[2][0]) / s, qx = (V[0][1] + V[1][0]) / s, qy = 0.25 * s, qz = (V[1][2] + V[2][1]) / s;
  } else {
    const double s = sqrt(((1.0 + V[2][2]) - V[0][0]) - V[1][1]) * 2.0;
    qw = (V[1][0] - V[0][1]) / s, qx = (V[0][2] + V[2][0]) / s, qy = (V[1][2] + V[2][1]) / s, qz = 0.25 * s;
  }
  const double qn = sqrt(((qw * qw + qx * qx) + qy * qy) + qz * qz);
  qw = qw / qn, qx = qx / qn, qy = qy / qn, qz = qz / qn;
  if (qw < 0.0) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
  const double vol = (sc[0] * sc[1]) * sc[2];
  double al = sum_a / vol;
  const double al_lo = 1.0 / 255.0, al_hi = 0.99;
  al = al < al_lo ? al_lo : (al > al_hi ? al_hi : al);
#pragma unroll
  for (int k = 0; k < 3; k++) a.out_pos[3 * r + k] = (float)mu[k], a.out_scale[3 * r + k] = (float)sc[k];
  a.out_quat[4 * r] = (float)qw, a.out_quat[4 * r + 1] = (float)qx, a.out_quat[4 * r + 2] = (float)qy, a.out_quat[4 * r + 3] = (float)qz;
  a.out_alpha[r] = (float)al;
}

// ---- emit: the colour rows -------------------------------------------------------------------------------------------------
struct ColourArgs {
  int32_t P;
  const float *dc, *rest;
  const int64_t* totals;
  const uint32_t* order;
  const uint32_t* cstart;
  const double* mass;
  const double* row_mass;
  int64_t rows;
  float *out_dc, *out_rest;
};

// C: floats of one features_rest row; CT = C + 3 channels per Gaussian, features_dc first
template <int C>
__global__ void __launch_bounds__(TPB) lod_colour_kernel(ColourArgs a) {
  constexpr int CT = C + 3, CP = CT | 1;
  constexpr int NPAIR = (ROWS_PER_BLOCK * CT + TPB - 1) / TPB;      // (row, channel) pairs per thread
  __shared__ float rows_lds[CHUNK * CP];
  __shared__ double mass_lds[CHUNK];
  const int64_t nrows_all = a.rows < a.totals[T_ROWS] ? a.rows : a.totals[T_ROWS];
  const int64_t r0 = (int64_t)blockIdx.x * ROWS_PER_BLOCK;
  if (r0 >= nrows_all) return;                                      // (uniform: the whole workgroup)
  const int nrows = (int)(nrows_all - r0 < ROWS_PER_BLOCK ? nrows_all - r0 : ROWS_PER_BLOCK);
  const uint32_t P = (uint32_t)a.P;
  uint32_t p0 = a.cstart[r0], pend = a.cstart[r0 + nrows];
  if (pend > P) pend = P;
  double acc[NPAIR];
  float first[NPAIR];
  uint32_t lo[NPAIR], hi[NPAIR];
#pragma unroll
  for (int u = 0; u < NPAIR; u++) {
    const int q = threadIdx.x + u * TPB, rl = q / CT;
    acc[u] = 0.0, first[u] = 0.0f, lo[u] = 0u, hi[u] = 0u;
    if (rl < nrows) {
      lo[u] = a.cstart[r0 + rl], hi[u] = a.cstart[r0 + rl + 1];
      if (hi[u] > pend) hi[u] = pend;
    }
  }
  for (; p0 < pend; p0 += CHUNK) {
    const int nm = (int)(pend - p0 < (uint32_t)CHUNK ? pend - p0 : (uint32_t)CHUNK);
    for (int w = threadIdx.x; w < nm * CT; w += TPB) {
      const int mem = w / CT, ch = w % CT;
      uint32_t g = a.order[p0 + mem];
      if (g >= P) g = 0u;
      rows_lds[mem * CP + ch] = ch < 3 ? a.dc[(size_t)g * 3 + ch] : a.rest[(size_t)g * C + (ch - 3)];
    }
    if (threadIdx.x < nm) mass_lds[threadIdx.x] = a.mass[p0 + threadIdx.x];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NPAIR; u++) {
      const int ch = (threadIdx.x + u * TPB) % CT;
      const uint32_t b = lo[u] > p0 ? lo[u] : p0, e = hi[u] < p0 + nm ? hi[u] : p0 + nm;
      const bool one = hi[u] - lo[u] == 1u;
      for (uint32_t j = b; j < e; j++) {
        const float f = rows_lds[(j - p0) * CP + ch];
        if (one) first[u] = f;
        else acc[u] = acc[u] + mass_lds[j - p0] * (double)f;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < NPAIR; u++) {
    const int q = threadIdx.x + u * TPB, rl = q / CT, ch = q % CT;
    if (rl >= nrows || hi[u] <= lo[u]) continue;
    const int64_t r = r0 + rl;
    const float v = hi[u] - lo[u] == 1u ? first[u] : (float)(acc[u] / a.row_mass[r]);
    if (ch < 3) a.out_dc[3 * r + ch] = v;
    else a.out_rest[(size_t)r * C + (ch - 3)] = v;
  }
}

static bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }
static int rest_floats(int32_t K) { return (K == 0 || K == 3 || K == 8 || K == 15) ? 3 * K : -1; }

static int check_common(const char* what, int32_t P, int32_t K, const float* pos, const float* scale, const float* quat, const float* alpha,
                        const float* dc, const float* rest, float cell, const void* workspace) {
  if (P < 0 || P >= (1 << 24)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= P < 2^24");
  if (rest_floats(K) < 0) return b3gs_fail(B3GS_ERR_ARG, what, "K (features_rest coefficients per channel) is 0, 3, 8 or 15");
  if (!(cell > 0.0f) || !(cell <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "the cell is positive and finite");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (P > 0 && (!pos || !scale || !quat || !alpha || !dc || (K > 0 && !rest))) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  return B3GS_OK;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_gaussian_merge_workspace_bytes(int64_t P, int32_t K) {
  if (P < 0 || P >= (1 << 24) || rest_floats(K) < 0) return 0;
  return lod_carve(nullptr, P, nullptr);
}

extern "C" int b3gs_gaussian_merge_count(int32_t P, int32_t K, const float* positions, const float* scales, const float* quaternions,
                                         const float* opacities, const float* features_dc, const float* features_rest,
                                         const double* weights, float cell, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_gaussian_merge_count";
  if (int rc = check_common(what, P, K, positions, scales, quaternions, opacities, features_dc, features_rest, cell, workspace)) return rc;
  LodWs w;
  lod_carve(static_cast<char*>(workspace), P, &w);
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(workspace, 0, 256, s);
  if (P == 0) return b3gs_launch_status(what);
  const int C = rest_floats(K);
  const unsigned nb = blocks_of(P);
  const int nparts = (int)(nb < (unsigned)MAX_PARTS ? nb : (unsigned)MAX_PARTS);
  InArgs in = {P, C, positions, scales, quaternions, opacities, features_dc, features_rest, weights};
  if (C > 0) {
    const int64_t nwords = (int64_t)P * C;
    (void)hipMemsetAsync(w.bad, 0, (size_t)P, s);
    hipLaunchKernelGGL(lod_rest_finite_kernel, dim3(blocks_of(nwords)), dim3(TPB), 0, s, nwords, (int32_t)C, features_rest, w.bad);
  }
  hipLaunchKernelGGL(lod_bbox_kernel, dim3(nparts), dim3(TPB), 0, s, in, (const uint8_t*)w.bad, w.part, w.totals);
  hipLaunchKernelGGL(lod_origin_kernel, dim3(1), dim3(64), 0, s, (const float*)w.part, nparts, w.grid, w.totals);
  hipLaunchKernelGGL(lod_key_kernel, dim3(nb), dim3(TPB), 0, s, P, positions, scales, (const LGrid*)w.grid, cell, w.vkey, w.totals);
  b3gs_launch_sort_u32_index(w.vkey, w.skey, w.sval, (uint32_t)P, w.hist, s);
  hipLaunchKernelGGL(lod_head_count_kernel, dim3(nb), dim3(TPB), 0, s, P, (const uint32_t*)w.skey[0], w.bsum);
  hipLaunchKernelGGL(lod_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, w.bsum, (int)nb, w.totals + T_ROWS);
  hipLaunchKernelGGL(lod_rows_kernel, dim3(nb), dim3(TPB), 0, s, P, (const uint32_t*)w.skey[0], (const uint32_t*)w.sval[0],
                     (const uint32_t*)w.bsum, w.totals, w.vrow, w.cstart);
  hipLaunchKernelGGL(lod_members_kernel, dim3(nb), dim3(TPB), 0, s, P, (const uint32_t*)w.cstart, w.totals);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_gaussian_merge_emit(int32_t P, int32_t K, const float* positions, const float* scales, const float* quaternions,
                                        const float* opacities, const float* features_dc, const float* features_rest,
                                        const double* weights, float cell, void* workspace, const int64_t* totals, float* out_positions,
                                        float* out_scales, float* out_quaternions, float* out_opacities, float* out_features_dc,
                                        float* out_features_rest, int32_t* cluster_of, int32_t* members, b3gs_stream_t stream) {
  static const char* what = "b3gs_gaussian_merge_emit";
  if (int rc = check_common(what, P, K, positions, scales, quaternions, opacities, features_dc, features_rest, cell, workspace)) return rc;
  if (!totals) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  char msg[160];
  if (totals[T_NONFINITE]) {
    snprintf(msg, sizeof msg, "%lld rows hold a value that is not finite", (long long)totals[T_NONFINITE]);
    return b3gs_fail(B3GS_ERR_ARG, what, msg);
  }
  if (totals[T_OVER]) {
    snprintf(msg, sizeof msg, "%lld rows lie beyond the %d cells of an axis", (long long)totals[T_OVER], MAX_DIM);
    return b3gs_fail(B3GS_ERR_ARG, what, msg);
  }
  const int64_t rows = totals[T_CLUSTERS] + totals[T_PASS];
  if (totals[T_CLUSTERS] < 0 || totals[T_PASS] < 0 || rows > P || (P > 0 && rows < 1))
    return b3gs_fail(B3GS_ERR_ARG, what, "the totals are those the count call left");
  if (P == 0) return B3GS_OK;
  if (!out_positions || !out_scales || !out_quaternions || !out_opacities || !out_features_dc || (K > 0 && !out_features_rest) || !cluster_of ||
      !members)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  LodWs w;
  lod_carve(static_cast<char*>(workspace), P, &w);
  hipStream_t s = (hipStream_t)stream;
  const int C = rest_floats(K);
  (void)hipMemcpyAsync(cluster_of, w.vrow, (size_t)P * sizeof(int32_t), hipMemcpyDeviceToDevice, s);
  MomentArgs m = {};
  m.in = {P, C, positions, scales, quaternions, opacities, features_dc, features_rest, weights};
  m.totals = w.totals, m.order = w.sval[0], m.cstart = w.cstart, m.rows = rows, m.mass = w.mass, m.row_mass = w.row_mass;
  m.out_pos = out_positions, m.out_scale = out_scales, m.out_quat = out_quaternions, m.out_alpha = out_opacities, m.members = members;
  hipLaunchKernelGGL(lod_moment_kernel, dim3(blocks_of(rows)), dim3(TPB), 0, s, m);
  ColourArgs c = {};
  c.P = P, c.dc = features_dc, c.rest = features_rest, c.totals = w.totals, c.order = w.sval[0], c.cstart = w.cstart, c.mass = w.mass;
  c.row_mass = w.row_mass, c.rows = rows, c.out_dc = out_features_dc, c.out_rest = out_features_rest;
  const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(TPB);
  switch (C) {
    case 0: hipLaunchKernelGGL(lod_colour_kernel<0>, grid, block, 0, s, c); break;
    case 9: hipLaunchKernelGGL(lod_colour_kernel<9>, grid, block, 0, s, c); break;
    case 24: hipLaunchKernelGGL(lod_colour_kernel<24>, grid, block, 0, s, c); break;
    default: hipLaunchKernelGGL(lod_colour_kernel<45>, grid, block, 0, s, c); break;
  }
  return b3gs_launch_status(what);
}
