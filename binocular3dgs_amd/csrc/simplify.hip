// Simplifying an extracted mesh by vertex clustering (binocular3dgs_amd/mesh_tools.py).
// include/b3gs_raster.h states the rule statement by statement; tests/simplify_ref.py restates it.  Every step is integer
// work, a stable sort, an ordered scan, one correctly rounded float32 operation per statement, or fp64 statements executed
// by ONE thread in one fixed order, so every output is one fixed result.
//   count   bbox      partial minima / maxima per workgroup, non-finite coordinates counted
//           origin    one wave folds the partials: origin and extent -> the head of the workspace
//           keys      thread = vertex: the cell key; a coordinate past cell 1023 is counted
//           sort      the project's radix sort (stable): members of a cluster stay in vertex-index order
//           clusters  head flags of the sorted keys -> block sums -> scan -> cluster id per vertex, first member per cluster
//           faces     thread = face: cluster ids of the corners, (min, mid, max); degenerate faces counted
//           3 sorts   by max, then mid, then min (each stable, the orders composed): equal triples are adjacent, in
//                     face-index order; the first of a run survives
//           ranks     a survive flag per face and a used flag per cluster -> block sums -> scans -> the two totals
//   emit    faces     rank = block offset + ballot rank -> rows in input order, corners mapped to the new cluster ids
//           incidence (quadric only) three (cluster, face) slots per face, a cluster named twice keeps one, sorted stably by
//                     cluster: per cluster its faces in face-index order
//           place     thread = cluster: colour, fp64 mean in member order, the quadric in face-index order, the 3 x 3 Cholesky
#include "b3gs_internal.h"
#include <cfloat>

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int MAX_DIM = 1024;                  // cells per axis: 10 bits of the key
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;       // a face or an incidence slot that takes no part (cluster ids stay below 2^31)
constexpr int MAX_PARTS = 256;

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// words of the totals (int64 each) at the head of the workspace
enum { T_NVERTS = 0, T_NTRIS, T_BAD_FACES, T_NONFINITE, T_OVER, T_CLUSTERS, T_DEGENERATE, T_DUPLICATE, T_EXTENT_BITS, T_WORDS };

struct SGrid {                      // behind the totals (byte 128 of the workspace), written by origin_kernel
  float o[3];
  float extent;                     // the largest of the three box edges
};

struct SimpWs {
  int64_t* totals;
  SGrid* grid;
  float* part;                      // [MAX_PARTS][6]
  uint32_t* skey[2];                // [N] sort ping / pong, N = max(V, 3 F, 1)
  uint32_t* sval[2];
  uint32_t* hist;
  uint32_t* vkey;                   // [V] cell key per vertex
  uint32_t* members;                // [V] vertex indices in (cluster, vertex index) order
  int32_t* vcluster;                // [V] cluster id per vertex
  uint32_t* cstart;                 // [V + 1] first member of every cluster; cstart[clusters] = V
  int32_t* used;                    // [V] cluster k is named by a surviving face
  int32_t* newid;                   // [V] emit: the new id of cluster k, or -1
  uint32_t* bsum_c;                 // [nbv] head flags
  uint32_t* bsum_v;                 // [nbv] used flags
  uint32_t* bsum_f;                 // [nbf] survive flags
  uint32_t* fk[3];                  // [F] min, mid, max cluster id per face (NO_KEY: degenerate or naming no vertex)
  uint32_t* gkey;                   // [F] the keys of the next sort, gathered in the order so far
  uint32_t* ord[2];                 // [F] the composed order after sort 1 / sort 2
  uint8_t* survive;                 // [F]
  uint2* inc;                       // [V] emit: {first, one past last} incidence of every cluster in the sorted slots
};

static size_t simp_carve(char* base, int64_t V, int64_t F, SimpWs* w) {
  char* cur = base;
  const size_t v = (size_t)(V > 0 ? V : 1), f = (size_t)(F > 0 ? F : 1);
  const size_t n = v > 3 * f ? v : 3 * f;
  SimpWs t;
  t.totals = b3gs_carve<int64_t>(cur, 16);                         // 128 bytes, then the grid: one 256-byte head
  cur = base + 128;
  t.grid = b3gs_carve<SGrid>(cur, 1);
  cur = base + 256;
  t.part = b3gs_carve<float>(cur, 6 * MAX_PARTS);
  for (int k = 0; k < 2; k++) t.skey[k] = b3gs_carve<uint32_t>(cur, n);
  for (int k = 0; k < 2; k++) t.sval[k] = b3gs_carve<uint32_t>(cur, n);
  t.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)n));
  t.vkey = b3gs_carve<uint32_t>(cur, v);
  t.members = b3gs_carve<uint32_t>(cur, v);
  t.vcluster = b3gs_carve<int32_t>(cur, v);
  t.cstart = b3gs_carve<uint32_t>(cur, v + 1);
  t.used = b3gs_carve<int32_t>(cur, v);
  t.newid = b3gs_carve<int32_t>(cur, v);
  t.bsum_c = b3gs_carve<uint32_t>(cur, blocks_of((int64_t)v));
  t.bsum_v = b3gs_carve<uint32_t>(cur, blocks_of((int64_t)v));
  t.bsum_f = b3gs_carve<uint32_t>(cur, blocks_of((int64_t)f));
  for (int k = 0; k < 3; k++) t.fk[k] = b3gs_carve<uint32_t>(cur, f);
  t.gkey = b3gs_carve<uint32_t>(cur, f);
  for (int k = 0; k < 2; k++) t.ord[k] = b3gs_carve<uint32_t>(cur, f);
  t.survive = b3gs_carve<uint8_t>(cur, f);
  t.inc = b3gs_carve<uint2>(cur, v);
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

// ---- the grid ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) simp_bbox_kernel(int32_t V, const float* __restrict__ pts, float* __restrict__ part, int64_t* totals) {
  __shared__ float red[TPB / 64][6];
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  unsigned long long bad = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < V; i += (int64_t)gridDim.x * TPB) {
    bool fin = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float v = pts[3 * i + a];
      fin = fin && fabsf(v) <= FLT_MAX;                              // (false for NaN and for either infinity)
      lo[a] = fminf(lo[a], v);
      hi[a] = fmaxf(hi[a], v);
    }
    bad += fin ? 0ull : 1ull;
  }
  bad = b3gs_wave_sum(bad);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0) count_up(totals + T_NONFINITE, bad);
  const float v = b3gs_block_bbox<TPB>(lo, hi, red);
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = v;
}

__global__ void __launch_bounds__(64) simp_origin_kernel(const float* __restrict__ part, int nparts, SGrid* g, int64_t* totals) {
  __shared__ float bb[6];
  if (threadIdx.x < 6) {
    float v = part[threadIdx.x];
    for (int k = 1; k < nparts; k++) v = threadIdx.x < 3 ? fminf(v, part[k * 6 + threadIdx.x]) : fmaxf(v, part[k * 6 + threadIdx.x]);
    bb[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x) return;
  float ext = 0.0f;
  for (int a = 0; a < 3; a++) {
    g->o[a] = bb[a];
    ext = fmaxf(ext, __fsub_rn(bb[3 + a], bb[a]));
  }
  g->extent = ext;
  totals[T_EXTENT_BITS] = (int64_t)__float_as_uint(ext);
}

// the cell coordinate along one axis: two rounded float32 operations, then the floor (the idiom of the nearest-distance grid)
__device__ __forceinline__ float cell_coord(float x, float o, float h) { return floorf(__fdiv_rn(__fsub_rn(x, o), h)); }

__global__ void __launch_bounds__(TPB) simp_key_kernel(int32_t V, const float* __restrict__ pts, const SGrid* __restrict__ gp, float cell,
                                                       uint32_t* __restrict__ vkey, int64_t* totals) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool over = false;
  if (i < V) {
    const SGrid g = *gp;
    uint32_t key = 0u;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const float c = cell_coord(pts[3 * i + a], g.o[a], cell);
      const bool ok = c >= 0.0f && c < (float)MAX_DIM;              // (false for NaN)
      over = over || !ok;
      key |= (ok ? (uint32_t)c : 0u) << (10 * a);
    }
    vkey[i] = over ? 0u : key;
  }
  count_flags(totals + T_OVER, over);
}

// ---- clusters ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int head_flag(const uint32_t* __restrict__ skey, int64_t i, int32_t V) {
  return i < V && (i == 0 || skey[i] != skey[i - 1]);
}

__global__ void __launch_bounds__(TPB) simp_head_count_kernel(int32_t V, const uint32_t* __restrict__ skey, uint32_t* __restrict__ bsum) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  b3gs_block_rank<TPB, 1>(head_flag(skey, i, V), wave_n, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(SCAN_TPB) simp_scan_kernel(uint32_t* bsum, int nb, int64_t* total) { b3gs_scan_block_sums(bsum, nb, total); }

// the cluster id of sorted position i = the heads in front of it (its own included) - 1
__global__ void __launch_bounds__(TPB) simp_cluster_kernel(int32_t V, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                                           const uint32_t* __restrict__ bsum, const int64_t* __restrict__ totals,
                                                           uint32_t* __restrict__ members, int32_t* __restrict__ vcluster,
                                                           uint32_t* __restrict__ cstart) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = head_flag(skey, i, V);
  int total;
  const int64_t before = (int64_t)bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (i >= V) return;
  const int64_t k = before + flag - 1;
  const uint32_t v = sval[i];
  members[i] = v;
  if (v < (uint32_t)V) vcluster[v] = (int32_t)k;
  if (flag) cstart[k] = (uint32_t)i;
  if (i == 0) cstart[totals[T_CLUSTERS]] = (uint32_t)V;             // (clusters <= V: inside the V + 1 words)
}

// ---- faces -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool face_ok(const int32_t* f, int32_t V) {
  return (uint32_t)f[0] < (uint32_t)V && (uint32_t)f[1] < (uint32_t)V && (uint32_t)f[2] < (uint32_t)V;
}

__global__ void __launch_bounds__(TPB) simp_face_key_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ vcluster, uint32_t* __restrict__ kmin,
                                                            uint32_t* __restrict__ kmid, uint32_t* __restrict__ kmax, int64_t* totals) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool bad = false, degenerate = false;
  if (t < F) {
    const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    uint32_t lo = NO_KEY, md = NO_KEY, hi = NO_KEY;
    bad = !face_ok(f, V);
    if (!bad) {
      const uint32_t a = (uint32_t)vcluster[f[0]], b = (uint32_t)vcluster[f[1]], c = (uint32_t)vcluster[f[2]];
      degenerate = a == b || b == c || a == c;
      if (!degenerate) {
        lo = min(a, min(b, c));
        hi = max(a, max(b, c));
        md = a ^ b ^ c ^ lo ^ hi;                                   // the one that is neither
      }
    }
    kmin[t] = lo, kmid[t] = md, kmax[t] = hi;
  }
  count_flags(totals + T_BAD_FACES, bad);
  count_flags(totals + T_DEGENERATE, degenerate);
}

// order_out[i] = order_in[perm[i]] (order_in null: the identity), key_out[i] = key[order_out[i]]
__global__ void __launch_bounds__(TPB) simp_compose_kernel(int64_t F, const uint32_t* __restrict__ order_in, const uint32_t* __restrict__ perm,
                                                           const uint32_t* __restrict__ key, uint32_t* __restrict__ order_out,
                                                           uint32_t* __restrict__ key_out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= F) return;
  uint32_t p = perm[i];
  if (p >= (uint64_t)F) p = 0u;                                      // (a permutation of 0 .. F-1: never taken)
  const uint32_t f = order_in ? order_in[p] : p;
  order_out[i] = f;
  if (key_out) key_out[i] = key[f < (uint64_t)F ? f : 0u];
}

// sorted position i holds face order[perm[i]]; it survives when it is not degenerate and the position in front holds another triple
__global__ void __launch_bounds__(TPB) simp_boundary_kernel(int64_t F, const uint32_t* __restrict__ order, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ kmin, const uint32_t* __restrict__ kmid,
                                                            const uint32_t* __restrict__ kmax, uint8_t* __restrict__ survive,
                                                            int32_t* __restrict__ used, int64_t* totals) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool dup = false;
  if (i < F) {
    uint32_t p = perm[i];
    if (p >= (uint64_t)F) p = 0u;
    const uint32_t f = order[p];
    const uint32_t lo = kmin[f], md = kmid[f], hi = kmax[f];
    bool first = true;
    if (i > 0) {
      uint32_t q = perm[i - 1];
      if (q >= (uint64_t)F) q = 0u;
      const uint32_t g = order[q];
      first = kmin[g] != lo || kmid[g] != md || kmax[g] != hi;
    }
    const bool live = lo != NO_KEY;
    survive[f] = live && first;
    dup = live && !first;
    if (live && first) used[lo] = 1, used[md] = 1, used[hi] = 1;    // (the same word from every writer)
  }
  count_flags(totals + T_DUPLICATE, dup);
}

__global__ void __launch_bounds__(TPB) simp_fcount_kernel(int64_t F, const uint8_t* __restrict__ survive, uint32_t* __restrict__ bsum) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  b3gs_block_rank<TPB, 1>(t < F ? survive[t] : 0, wave_n, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(TPB) simp_vcount_kernel(int32_t V, const int32_t* __restrict__ used, uint32_t* __restrict__ bsum) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  b3gs_block_rank<TPB, 1>(k < V ? used[k] != 0 : 0, wave_n, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)total;
}

// ---- emit --------------------------------------------------------------------------------------------------------------
// the new id of cluster k, or -1
__global__ void __launch_bounds__(TPB) simp_newid_kernel(int32_t V, const int32_t* __restrict__ used, const uint32_t* __restrict__ bsum,
                                                         int32_t* __restrict__ newid) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = k < V ? used[k] != 0 : 0;
  int total;
  const int64_t id = (int64_t)bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (k < V) newid[k] = flag ? (int32_t)id : -1;
}

__global__ void __launch_bounds__(TPB) simp_femit_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces, const int32_t* __restrict__ vcluster,
                                                         const int32_t* __restrict__ newid, const uint8_t* __restrict__ survive,
                                                         const uint32_t* __restrict__ bsum, int64_t ntris, int32_t* __restrict__ out_faces) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = t < F ? survive[t] : 0;
  int total;
  const int64_t id = (int64_t)bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (!flag || id >= ntris) return;                                 // (the output holds ntris rows)
#pragma unroll
  for (int x = 0; x < 3; x++) out_faces[3 * id + x] = newid[vcluster[faces[3 * t + x]]];   // (a surviving face names vertices)
}

// slot 3 t + x: the cluster of corner x of face t, unless an earlier corner of the face names it already
__global__ void __launch_bounds__(TPB) simp_incidence_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ vcluster, uint32_t* __restrict__ slots) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= F) return;
  const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
  uint32_t a = NO_KEY, b = NO_KEY, c = NO_KEY;
  if (face_ok(f, V)) {
    a = (uint32_t)vcluster[f[0]], b = (uint32_t)vcluster[f[1]], c = (uint32_t)vcluster[f[2]];
    if (c == a || c == b) c = NO_KEY;
    if (b == a) b = NO_KEY;
  }
  slots[3 * t] = a, slots[3 * t + 1] = b, slots[3 * t + 2] = c;
}

__global__ void __launch_bounds__(TPB) simp_inc_range_kernel(int64_t n, int32_t V, const uint32_t* __restrict__ skey, uint2* __restrict__ inc) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = skey[i];
  if (key >= (uint32_t)V) return;                                   // (NO_KEY slots sort behind every cluster)
  if (i == 0 || skey[i - 1] != key) inc[key].x = (uint32_t)i;
  if (i == n - 1 || skey[i + 1] != key) inc[key].y = (uint32_t)(i + 1);
}

struct PlaceArgs {
  int32_t V;
  int64_t F;
  const float* vertices;
  const uint8_t* colours;
  const int32_t* faces;
  float cell;
  int32_t quadric;
  const int64_t* totals;
  const uint32_t* members;
  const uint32_t* cstart;
  const int32_t* newid;
  const uint2* inc;
  const uint32_t* slot_of;          // sorted incidence -> slot 3 t + x
  int64_t nverts;
  float* out_vertices;
  uint8_t* out_colours;
};

// Thread = cluster; every fp64 statement below is one operation (the file is compiled with -ffp-contract=off), executed in the
// order written, members in vertex-index order and faces in face-index order: tests/simplify_ref.py walks the same statements.
__global__ void __launch_bounds__(TPB) simp_place_kernel(PlaceArgs a) {
  const int64_t k = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (k >= a.V || k >= a.totals[T_CLUSTERS]) return;
  const int64_t id = a.newid[k];
  if (id < 0 || id >= a.nverts) return;                             // (the outputs hold nverts rows)
  const uint32_t m0 = a.cstart[k], m1 = a.cstart[k + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  unsigned long long cr = 0ull, cg = 0ull, cb = 0ull;
  for (uint32_t j = m0; j < m1; j++) {
    const size_t v = a.members[j];
    sx += (double)a.vertices[3 * v], sy += (double)a.vertices[3 * v + 1], sz += (double)a.vertices[3 * v + 2];
    cr += a.colours[3 * v], cg += a.colours[3 * v + 1], cb += a.colours[3 * v + 2];
  }
  const unsigned long long n = m1 - m0, n2 = 2ull * n;              // n >= 1: cstart is strictly increasing
  a.out_colours[3 * id] = (uint8_t)((2ull * cr + n) / n2);
  a.out_colours[3 * id + 1] = (uint8_t)((2ull * cg + n) / n2);
  a.out_colours[3 * id + 2] = (uint8_t)((2ull * cb + n) / n2);
  const double dn = (double)n;
  const double mx = sx / dn, my = sy / dn, mz = sz / dn;
  double y0 = 0.0, y1 = 0.0, y2 = 0.0;
  if (a.quadric) {
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, r0 = 0.0, r1 = 0.0, r2 = 0.0;
    const uint2 range = a.inc[k];
    for (uint32_t j = range.x; j < range.y; j++) {
      const size_t t = a.slot_of[j] / 3u;
      if (t >= (size_t)a.F) continue;
      const size_t i0 = (size_t)a.faces[3 * t], i1 = (size_t)a.faces[3 * t + 1], i2 = (size_t)a.faces[3 * t + 2];
      const double p0x = (double)a.vertices[3 * i0], p0y = (double)a.vertices[3 * i0 + 1], p0z = (double)a.vertices[3 * i0 + 2];
      const double ux = (double)a.vertices[3 * i1] - p0x, uy = (double)a.vertices[3 * i1 + 1] - p0y, uz = (double)a.vertices[3 * i1 + 2] - p0z;
      const double vx = (double)a.vertices[3 * i2] - p0x, vy = (double)a.vertices[3 * i2 + 1] - p0y, vz = (double)a.vertices[3 * i2 + 2] - p0z;
      const double nx = uy * vz - uz * vy;
      const double ny = uz * vx - ux * vz;
      const double nz = ux * vy - uy * vx;
      const double qx = p0x - mx, qy = p0y - my, qz = p0z - mz;
      const double d = (nx * qx + ny * qy) + nz * qz;
      A00 += nx * nx, A01 += nx * ny, A02 += nx * nz, A11 += ny * ny, A12 += ny * nz, A22 += nz * nz;
      r0 += d * nx, r1 += d * ny, r2 += d * nz;
    }
    const double lam = 1e-3 * ((A00 + A11) + A22);
    if (lam != 0.0) {
      const double a00 = A00 + lam, a11 = A11 + lam, a22 = A22 + lam;
      const double l00 = sqrt(a00);
      const double l10 = A01 / l00;
      const double l20 = A02 / l00;
      const double l11 = sqrt(a11 - l10 * l10);
      const double l21 = (A12 - l20 * l10) / l11;
      const double l22 = sqrt((a22 - l20 * l20) - l21 * l21);
      const double z0 = r0 / l00;
      const double z1 = (r1 - l10 * z0) / l11;
      const double z2 = ((r2 - l20 * z0) - l21 * z1) / l22;
      y2 = z2 / l22;
      y1 = (z1 - l21 * y2) / l11;
      y0 = ((z0 - l10 * y1) - l20 * y2) / l00;
      const double big = fmax(fabs(y0), fmax(fabs(y1), fabs(y2)));  // (fmax drops a NaN: the finite test below catches it)
      const double lim = (double)a.cell;
      const bool fin = fabs(y0) <= DBL_MAX && fabs(y1) <= DBL_MAX && fabs(y2) <= DBL_MAX;
      if (!fin || big > lim) y0 = 0.0, y1 = 0.0, y2 = 0.0;
    }
  }
  a.out_vertices[3 * id] = (float)(mx + y0);
  a.out_vertices[3 * id + 1] = (float)(my + y1);
  a.out_vertices[3 * id + 2] = (float)(mz + y2);
}

static bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }

static int check_common(const char* what, int32_t V, int64_t F, const float* vertices, const int32_t* faces, float cell, const void* workspace) {
  if (V < 0 || F < 0 || 3 * F > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V <= 2^31 - 1, 0 <= 3 F <= 2^31 - 1");
  if (!(cell > 0.0f) || !(cell <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "the cell is positive and finite");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if ((V > 0 && !vertices) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  return B3GS_OK;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_mesh_simplify_workspace_bytes(int64_t V, int64_t F) {
  if (V < 0 || F < 0 || V > INT32_MAX || 3 * F > INT32_MAX) return 0;
  return simp_carve(nullptr, V, F, nullptr);
}

extern "C" int b3gs_mesh_simplify_count(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float cell, void* workspace,
                                        b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_simplify_count";
  if (int rc = check_common(what, V, F, vertices, faces, cell, workspace)) return rc;
  SimpWs w;
  simp_carve(static_cast<char*>(workspace), V, F, &w);
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(workspace, 0, 256, s);
  if (V == 0) return b3gs_launch_status(what);                      // (every face then names no vertex: the caller sees F != 0)
  const unsigned nbv = blocks_of(V), nbf = blocks_of(F);
  const int nparts = (int)(nbv < (unsigned)MAX_PARTS ? nbv : (unsigned)MAX_PARTS);
  hipLaunchKernelGGL(simp_bbox_kernel, dim3(nparts), dim3(TPB), 0, s, V, vertices, w.part, w.totals);
  hipLaunchKernelGGL(simp_origin_kernel, dim3(1), dim3(64), 0, s, (const float*)w.part, nparts, w.grid, w.totals);
  hipLaunchKernelGGL(simp_key_kernel, dim3(nbv), dim3(TPB), 0, s, V, vertices, (const SGrid*)w.grid, cell, w.vkey, w.totals);
  b3gs_launch_sort_u32_index(w.vkey, w.skey, w.sval, (uint32_t)V, w.hist, s);
  hipLaunchKernelGGL(simp_head_count_kernel, dim3(nbv), dim3(TPB), 0, s, V, (const uint32_t*)w.skey[0], w.bsum_c);
  hipLaunchKernelGGL(simp_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, w.bsum_c, (int)nbv, w.totals + T_CLUSTERS);
  hipLaunchKernelGGL(simp_cluster_kernel, dim3(nbv), dim3(TPB), 0, s, V, (const uint32_t*)w.skey[0], (const uint32_t*)w.sval[0],
                     (const uint32_t*)w.bsum_c, (const int64_t*)w.totals, w.members, w.vcluster, w.cstart);
  (void)hipMemsetAsync(w.used, 0, (size_t)V * sizeof(int32_t), s);
  if (F > 0) {
    hipLaunchKernelGGL(simp_face_key_kernel, dim3(nbf), dim3(TPB), 0, s, V, F, faces, (const int32_t*)w.vcluster, w.fk[0], w.fk[1], w.fk[2],
                       w.totals);
    // stable sorts by max, then mid, then min: the last one decides, ties keep the order of the sorts before
    b3gs_launch_sort_u32_index(w.fk[2], w.skey, w.sval, (uint32_t)F, w.hist, s);
    hipLaunchKernelGGL(simp_compose_kernel, dim3(nbf), dim3(TPB), 0, s, F, (const uint32_t*)nullptr, (const uint32_t*)w.sval[0],
                       (const uint32_t*)w.fk[1], w.ord[0], w.gkey);
    b3gs_launch_sort_u32_index(w.gkey, w.skey, w.sval, (uint32_t)F, w.hist, s);
    hipLaunchKernelGGL(simp_compose_kernel, dim3(nbf), dim3(TPB), 0, s, F, (const uint32_t*)w.ord[0], (const uint32_t*)w.sval[0],
                       (const uint32_t*)w.fk[0], w.ord[1], w.gkey);
    b3gs_launch_sort_u32_index(w.gkey, w.skey, w.sval, (uint32_t)F, w.hist, s);
    hipLaunchKernelGGL(simp_boundary_kernel, dim3(nbf), dim3(TPB), 0, s, F, (const uint32_t*)w.ord[1], (const uint32_t*)w.sval[0],
                       (const uint32_t*)w.fk[0], (const uint32_t*)w.fk[1], (const uint32_t*)w.fk[2], w.survive, w.used, w.totals);
    hipLaunchKernelGGL(simp_fcount_kernel, dim3(nbf), dim3(TPB), 0, s, F, (const uint8_t*)w.survive, w.bsum_f);
    hipLaunchKernelGGL(simp_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, w.bsum_f, (int)nbf, w.totals + T_NTRIS);
  }
  hipLaunchKernelGGL(simp_vcount_kernel, dim3(nbv), dim3(TPB), 0, s, V, (const int32_t*)w.used, w.bsum_v);
  hipLaunchKernelGGL(simp_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, w.bsum_v, (int)nbv, w.totals + T_NVERTS);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_simplify_emit(int32_t V, int64_t F, const float* vertices, const uint8_t* colours, const int32_t* faces, float cell,
                                       int32_t placement, void* workspace, int64_t nverts, int64_t ntris, float* out_vertices,
                                       uint8_t* out_colours, int32_t* out_faces, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_simplify_emit";
  if (int rc = check_common(what, V, F, vertices, faces, cell, workspace)) return rc;
  if (placement != B3GS_SIMPLIFY_QUADRIC && placement != B3GS_SIMPLIFY_MEAN) return b3gs_fail(B3GS_ERR_ARG, what, "unknown placement");
  if (nverts < 0 || ntris < 0 || nverts > V || ntris > F) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= nverts <= V, 0 <= ntris <= F (int32 totals)");
  if ((V > 0 && !colours) || (nverts > 0 && (!out_vertices || !out_colours)) || (ntris > 0 && !out_faces))
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (nverts == 0 && ntris == 0) return B3GS_OK;
  SimpWs w;
  simp_carve(static_cast<char*>(workspace), V, F, &w);
  hipStream_t s = (hipStream_t)stream;
  const unsigned nbv = blocks_of(V), nbf = blocks_of(F);
  hipLaunchKernelGGL(simp_newid_kernel, dim3(nbv), dim3(TPB), 0, s, V, (const int32_t*)w.used, (const uint32_t*)w.bsum_v, w.newid);
  if (ntris > 0)
    hipLaunchKernelGGL(simp_femit_kernel, dim3(nbf), dim3(TPB), 0, s, V, F, faces, (const int32_t*)w.vcluster, (const int32_t*)w.newid,
                       (const uint8_t*)w.survive, (const uint32_t*)w.bsum_f, ntris, out_faces);
  const int quadric = placement == B3GS_SIMPLIFY_QUADRIC && F > 0;
  if (quadric) {
    const int64_t n = 3 * F;
    // the slots go to skey[0]: the first pass of the sort reads them there and writes skey[1], the second one replaces them
    hipLaunchKernelGGL(simp_incidence_kernel, dim3(nbf), dim3(TPB), 0, s, V, F, faces, (const int32_t*)w.vcluster, w.skey[0]);
    b3gs_launch_sort_u32_index(w.skey[0], w.skey, w.sval, (uint32_t)n, w.hist, s);
    (void)hipMemsetAsync(w.inc, 0, (size_t)V * sizeof(uint2), s);
    hipLaunchKernelGGL(simp_inc_range_kernel, dim3(blocks_of(n)), dim3(TPB), 0, s, n, V, (const uint32_t*)w.skey[0], w.inc);
  }
  if (nverts > 0) {
    PlaceArgs a = {};
    a.V = V, a.F = F, a.vertices = vertices, a.colours = colours, a.faces = faces, a.cell = cell, a.quadric = quadric;
    a.totals = w.totals, a.members = w.members, a.cstart = w.cstart, a.newid = w.newid, a.inc = w.inc, a.slot_of = w.sval[0];
    a.nverts = nverts, a.out_vertices = out_vertices, a.out_colours = out_colours;
    hipLaunchKernelGGL(simp_place_kernel, dim3(nbv), dim3(TPB), 0, s, a);
  }
  return b3gs_launch_status(what);
}
