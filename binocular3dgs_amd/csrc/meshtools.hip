// Cleaning and scoring an extracted mesh (ABI 18; binocular3dgs_amd/mesh_tools.py).
// include/b3gs_raster.h states the arithmetic; tests/meshtools_ref.py restates it.  Everything is integer work, a minimum over
// a set, or one correctly rounded float32 operation per statement, so every output is one fixed result.
//   components  init (labels[v] = v), hook (thread = triangle edge: lock-free union-find, find with path halving, the larger
//               root is hooked under the smaller by a compare-and-swap), flatten (thread = vertex: read-only find), count
//               (thread = triangle: one integer atomic at its label).  No thread waits for another: a failed swap means
//               another thread hooked that root, and every find walks strictly decreasing indices.
//   clean       count: a keep flag per vertex and per triangle -> block sums from one ballot, scan (b3gs_internal.h);
//               emit: rank = block offset + ballot rank -> new vertex ids (kept for the triangles), rows in order
//   sample      count: thread = triangle, (n1, n2) and the closed-form lattice count -> block sums, the exact 64-bit total by
//               integer atomics; emit: block offset + in-block scan, the thread writes its lattice in (i, j) order
//   nearest     grid: bounding box of b, the grid's origin / edge / dimensions computed ON THE DEVICE (no host read), cell id
//               per point, the project's radix sort, {start, end} per cell by a boundary pass, points copied in cell order;
//               query: thread = query point, Chebyshev shells of cells outward (see the bound at query_kernel)
//   score       per direction: fp64 partial sums per workgroup, folded in index order by one wave
#include "b3gs_internal.h"
#include <cfloat>

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int MAX_LATTICE = 1 << 15;          // n1, n2 stay below this
constexpr int GRID_MAX_DIM = 1024;            // cells per axis of the search grid
constexpr int64_t GRID_MAX_CELLS = (int64_t)1 << 24;

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// The correctly rounded float32 square root.  NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map that
// name to the native v_sqrt_f32, which is good to 1 ulp only; sqrtf (no fast-math) is the hardware estimate plus the fix-up.
__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }

// ---- connected components ----------------------------------------------------------------------------------------------
// The parent words are read and written by many workgroups inside one launch: agent-scope relaxed accesses.  parent[x] <= x
// always, with equality exactly at a root; a vertex that stopped being a root never becomes one again, so a stale value is
// still an ancestor and every decision taken on it is repeated on the real word by the compare-and-swap.
__device__ __forceinline__ int32_t ld_parent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_parent(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t find_halving(int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = ld_parent(parent + x);
    if (p == x) return x;
    const int32_t g = ld_parent(parent + p);
    if (g == p) return p;
    st_parent(parent + x, g);             // g < p < x: an ancestor
    x = g;
  }
}
__device__ __forceinline__ int32_t find_readonly(const int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = ld_parent(parent + x);
    if (p == x) return x;
    x = p;
  }
}
__device__ __forceinline__ bool face_ok(const int32_t* f, int32_t V) {
  return (uint32_t)f[0] < (uint32_t)V && (uint32_t)f[1] < (uint32_t)V && (uint32_t)f[2] < (uint32_t)V;
}

__global__ void __launch_bounds__(TPB) cc_init_kernel(int32_t V, int32_t* labels, int32_t* tri_count) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= V) return;
  labels[v] = (int32_t)v;
  tri_count[v] = 0;
}

__global__ void __launch_bounds__(TPB) cc_hook_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces, int32_t* parent) {
  const int64_t id = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (id >= 3 * F) return;
  const int64_t t = id / 3;
  const int e = (int)(id - 3 * t);
  const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
  if (!face_ok(f, V)) return;                                     // (a triangle that names no vertex connects nothing)
  const int32_t u = f[e], v = f[e == 2 ? 0 : e + 1];
  if (u == v) return;
  int32_t ru = find_halving(parent, u), rv = find_halving(parent, v);
  while (ru != rv) {
    if (ru < rv) { const int32_t s = ru; ru = rv; rv = s; }       // the larger root goes under the smaller
    const int32_t old = atomicCAS(parent + ru, ru, rv);
    if (old == ru) break;
    ru = find_halving(parent, old);                               // somebody else hooked ru: progress was made
    rv = find_halving(parent, rv);
  }
}

__global__ void __launch_bounds__(TPB) cc_flatten_kernel(int32_t V, int32_t* labels) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v >= V) return;
  st_parent(labels + v, find_readonly(labels, (int32_t)v));      // a root keeps itself; every other word becomes its root
}

__global__ void __launch_bounds__(TPB) cc_count_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ labels, int32_t* tri_count) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= F) return;
  const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
  if (face_ok(f, V)) atomicAdd(tri_count + labels[f[0]], 1);
}

// ---- clean -------------------------------------------------------------------------------------------------------------
struct CleanArgs {
  int32_t V;
  int64_t F;
  int32_t nbv, nbf;
  const int32_t* faces;
  const int32_t* labels;
  const int32_t* tri_count;
  const int32_t* threshold;         // device scalar
  int64_t* totals;                  // [0] vertices kept, [1] triangles kept, [2] triangles that name no vertex
  int32_t* newid;                   // [V]
  uint32_t* bsum_v;                 // [nbv]
  uint32_t* bsum_f;                 // [nbf]
  int64_t nverts, ntris;            // emit: rows of the outputs
  const float* vertices;
  const uint8_t* colours;
  float* out_vertices;
  uint8_t* out_colours;
  int32_t* out_faces;
};

// the component of vertex v survives and has a triangle
__device__ __forceinline__ int keep_vertex(const CleanArgs& a, int32_t v) {
  const int32_t l = a.labels[v];
  if ((uint32_t)l >= (uint32_t)a.V) return 0;
  const int32_t thr = *a.threshold;
  return a.tri_count[l] >= (thr > 1 ? thr : 1);
}
__device__ __forceinline__ int keep_face(const CleanArgs& a, int64_t t, bool* bad) {
  const int32_t f[3] = {a.faces[3 * t], a.faces[3 * t + 1], a.faces[3 * t + 2]};
  *bad = !face_ok(f, a.V);
  return *bad ? 0 : keep_vertex(a, f[0]);
}

__global__ void __launch_bounds__(TPB) clean_vcount_kernel(CleanArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = v < a.V ? keep_vertex(a, (int32_t)v) : 0;
  int total;
  b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (threadIdx.x == 0) a.bsum_v[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(TPB) clean_fcount_kernel(CleanArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  const int flag = t < a.F ? keep_face(a, t, &bad) : 0;
  if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 2), 1ull);
  int total;
  b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (threadIdx.x == 0) a.bsum_f[blockIdx.x] = (uint32_t)total;
}

// block 0: vertices, block 1: triangles
__global__ void __launch_bounds__(SCAN_TPB) clean_scan_kernel(CleanArgs a) {
  const bool v = blockIdx.x == 0;
  b3gs_scan_block_sums(v ? a.bsum_v : a.bsum_f, v ? a.nbv : a.nbf, a.totals + (v ? 0 : 1));
}

__global__ void __launch_bounds__(TPB) clean_vemit_kernel(CleanArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = v < a.V ? keep_vertex(a, (int32_t)v) : 0;
  int total;
  const int64_t id = (int64_t)a.bsum_v[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (v >= a.V) return;
  a.newid[v] = flag ? (int32_t)id : -1;
  if (!flag || id >= a.nverts) return;                            // (the outputs hold nverts rows)
#pragma unroll
  for (int x = 0; x < 3; x++) {
    a.out_vertices[3 * id + x] = a.vertices[3 * v + x];
    a.out_colours[3 * id + x] = a.colours[3 * v + x];
  }
}

__global__ void __launch_bounds__(TPB) clean_femit_kernel(CleanArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  const int flag = t < a.F ? keep_face(a, t, &bad) : 0;
  int total;
  const int64_t id = (int64_t)a.bsum_f[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  if (!flag || id >= a.ntris) return;                             // (the output holds ntris rows)
#pragma unroll
  for (int x = 0; x < 3; x++) a.out_faces[3 * id + x] = a.newid[a.faces[3 * t + x]];
}

struct CleanLayout {
  int32_t nbv, nbf;
  size_t newid, bsum_v, bsum_f, total;
};
static bool clean_layout(int64_t V, int64_t F, CleanLayout* l) {
  if (V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX) return false;
  l->nbv = (int32_t)blocks_of(V), l->nbf = (int32_t)blocks_of(F);
  size_t at = 256;                                                // the totals
  l->newid = at, at += b3gs_align256((size_t)(V ? V : 1) * sizeof(int32_t));
  l->bsum_v = at, at += b3gs_align256((size_t)(l->nbv ? l->nbv : 1) * sizeof(uint32_t));
  l->bsum_f = at, at += b3gs_align256((size_t)(l->nbf ? l->nbf : 1) * sizeof(uint32_t));
  l->total = at;
  return true;
}
static CleanArgs clean_args(int32_t V, int64_t F, const CleanLayout& l, void* workspace) {
  char* ws = static_cast<char*>(workspace);
  CleanArgs a = {};
  a.V = V, a.F = F, a.nbv = l.nbv, a.nbf = l.nbf;
  a.totals = reinterpret_cast<int64_t*>(ws);
  a.newid = reinterpret_cast<int32_t*>(ws + l.newid);
  a.bsum_v = reinterpret_cast<uint32_t*>(ws + l.bsum_v);
  a.bsum_f = reinterpret_cast<uint32_t*>(ws + l.bsum_f);
  return a;
}

// ---- points on the surface ---------------------------------------------------------------------------------------------
struct SampleArgs {
  int32_t V;
  int64_t F;
  int32_t nbf;
  const float* vertices;
  const int32_t* faces;
  float spacing;
  int64_t* totals;                  // [0] lattice points (exact), [1] triangles past the lattice limit, [2] triangles that
                                    // name no vertex, [3] the scan's own (wrapping) total
  uint32_t* nn;                     // [F] (n1 + 1) | (n2 + 1) << 16, minus one each; 0xFFFFFFFF: no lattice
  uint32_t* bsum;                   // [nbf]
  int64_t npoints;                  // emit: lattice rows of the output
  float* points;                    // emit: the first lattice row
};

__device__ __forceinline__ float edge_length(float x, float y, float z) {
  return sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
}
// lattice points of a triangle with A = n1 + 1, B = n2 + 1: the (i, j) with i B + j A < A B, without (0, 0).  Row i holds
// ceil(B (A - i) / A) of them; summed over i that is ((A-1)(B-1) + g - 1) / 2 + A + B - g with g = gcd(A, B).
__device__ __forceinline__ uint32_t lattice_count(uint32_t A, uint32_t B) {
  uint32_t g = A, r = B;
  while (r) { const uint32_t t = g % r; g = r; r = t; }
  return ((A - 1u) * (B - 1u) + g - 1u) / 2u + A + B - g - 1u;
}

__global__ void __launch_bounds__(TPB) sample_count_kernel(SampleArgs a) {
  __shared__ uint32_t wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  uint32_t cnt = 0u;
  if (t < a.F) {
    const int32_t f[3] = {a.faces[3 * t], a.faces[3 * t + 1], a.faces[3 * t + 2]};
    uint32_t code = 0xFFFFFFFFu;
    if (!face_ok(f, a.V)) {
      atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 2), 1ull);
    } else {
      const float* p0 = a.vertices + 3 * (size_t)f[0];
      const float* p1 = a.vertices + 3 * (size_t)f[1];
      const float* p2 = a.vertices + 3 * (size_t)f[2];
      const float l1 = edge_length(__fsub_rn(p1[0], p0[0]), __fsub_rn(p1[1], p0[1]), __fsub_rn(p1[2], p0[2]));
      const float l2 = edge_length(__fsub_rn(p2[0], p0[0]), __fsub_rn(p2[1], p0[1]), __fsub_rn(p2[2], p0[2]));
      const float n1 = floorf(__fdiv_rn(l1, a.spacing)), n2 = floorf(__fdiv_rn(l2, a.spacing));
      if (!(n1 < (float)MAX_LATTICE && n2 < (float)MAX_LATTICE)) {                  // (NaN and infinity land here too)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.totals + 1), 1ull);
      } else {
        const uint32_t A = (uint32_t)n1 + 1u, B = (uint32_t)n2 + 1u;
        code = (A - 1u) | ((B - 1u) << 16);
        cnt = lattice_count(A, B);
      }
    }
    a.nn[t] = code;
  }
  const unsigned long long wide = b3gs_wave_sum((unsigned long long)cnt);
  if ((threadIdx.x & 63) == 0 && wide) atomicAdd(reinterpret_cast<unsigned long long*>(a.totals), wide);
  uint32_t total;
  b3gs_block_exscan<TPB>(cnt, wave_n, &total);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_TPB) sample_scan_kernel(SampleArgs a) { b3gs_scan_block_sums(a.bsum, a.nbf, a.totals + 3); }

// Thread = triangle: the thread writes its whole lattice, so the time of the launch is that of the largest triangle.  At the
// intended spacing (a lattice of a few points per triangle) that is nothing; a single triangle near the 2^15 limit on both
// edges is legal and holds about 5 * 10^8 points, written by one lane over many seconds (limits).
__global__ void __launch_bounds__(TPB) sample_emit_kernel(SampleArgs a) {
  __shared__ uint32_t wave_n[TPB / B3GS_WAVE];
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const uint32_t code = t < a.F ? a.nn[t] : 0xFFFFFFFFu;
  const uint32_t A = (code & 0xFFFFu) + 1u, B = (code >> 16) + 1u;
  const uint32_t cnt = code == 0xFFFFFFFFu ? 0u : lattice_count(A, B);
  uint32_t total;
  int64_t at = (int64_t)a.bsum[blockIdx.x] + b3gs_block_exscan<TPB>(cnt, wave_n, &total);
  if (!cnt) return;
  const int32_t f0 = a.faces[3 * t], f1 = a.faces[3 * t + 1], f2 = a.faces[3 * t + 2];
  float p0[3], e1[3], e2[3];
#pragma unroll
  for (int x = 0; x < 3; x++) {
    p0[x] = a.vertices[3 * (size_t)f0 + x];
    e1[x] = __fsub_rn(a.vertices[3 * (size_t)f1 + x], p0[x]);
    e2[x] = __fsub_rn(a.vertices[3 * (size_t)f2 + x], p0[x]);
  }
  const float fa = (float)A, fb = (float)B;
  for (uint32_t i = 0; i < A; i++) {
    const uint32_t jn = (B * (A - i) + A - 1u) / A;              // the j with i B + j A < A B
    const float s = __fdiv_rn((float)i, fa);
    for (uint32_t j = i ? 0u : 1u; j < jn; j++) {
      if (at >= a.npoints) return;                                // (the output holds npoints lattice rows)
      const float w = __fdiv_rn((float)j, fb);
#pragma unroll
      for (int x = 0; x < 3; x++) a.points[3 * at + x] = __fadd_rn(__fadd_rn(p0[x], __fmul_rn(s, e1[x])), __fmul_rn(w, e2[x]));
      at++;
    }
  }
}

struct SampleLayout {
  int32_t nbf;
  size_t nn, bsum, total;
};
static bool sample_layout(int64_t F, SampleLayout* l) {
  if (F < 0 || F > INT32_MAX) return false;
  l->nbf = (int32_t)blocks_of(F);
  size_t at = 256;
  l->nn = at, at += b3gs_align256((size_t)(F ? F : 1) * sizeof(uint32_t));
  l->bsum = at, at += b3gs_align256((size_t)(l->nbf ? l->nbf : 1) * sizeof(uint32_t));
  l->total = at;
  return true;
}

// ---- nearest distances -------------------------------------------------------------------------------------------------
struct NGrid {                      // the head of the workspace, written by grid_params_kernel
  float o[3];                       // origin: floor(lower corner / h) * h, never above the lower corner
  float h;                          // cell edge
  int32_t dim[3];
  int32_t nshell;                   // the last shell a query may have to visit
};
struct NearWs {
  NGrid* grid;
  float* part;                      // [256][6] bounding box partials
  uint32_t* codes;                  // [Nb] cell id per point
  uint32_t* skey[2];
  uint32_t* sval[2];
  uint32_t* hist;
  float4* sorted;                   // [Nb] points in cell order
  uint2* cells;                     // [cap] {first, one past last} in `sorted`; {0, 0}: empty
};
// cells the table holds for Nb points: 8 per point, at least 4096, at most 2^24
static int64_t cell_capacity(int64_t Nb) {
  const int64_t c = 8 * Nb;
  return c < 4096 ? 4096 : (c > GRID_MAX_CELLS ? GRID_MAX_CELLS : c);
}
static size_t near_carve(char* base, int64_t Nb, NearWs* w) {
  char* cur = base;
  const size_t n = (size_t)(Nb > 0 ? Nb : 1);
  NearWs t;
  t.grid = b3gs_carve<NGrid>(cur, 1);
  t.part = b3gs_carve<float>(cur, 6 * 256);
  t.codes = b3gs_carve<uint32_t>(cur, n);
  for (int k = 0; k < 2; k++) t.skey[k] = b3gs_carve<uint32_t>(cur, n);
  for (int k = 0; k < 2; k++) t.sval[k] = b3gs_carve<uint32_t>(cur, n);
  t.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)n));
  t.sorted = b3gs_carve<float4>(cur, n);
  t.cells = b3gs_carve<uint2>(cur, (size_t)cell_capacity(Nb));
  if (w) *w = t;
  return (size_t)(cur - base);
}

__global__ void __launch_bounds__(TPB) near_bbox_kernel(int32_t n, const float* __restrict__ pts, float* __restrict__ part) {
  __shared__ float red[TPB / 64][6];
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB)
#pragma unroll
    for (int a = 0; a < 3; a++) { const float v = pts[3 * i + a]; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v); }
  const float v = b3gs_block_bbox<TPB>(lo, hi, red);
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = v;
}

// the cell coordinate of x along one axis, before clamping: one function for points and queries, monotone in x
__device__ __forceinline__ float cell_coord(float x, float o, float h) { return floorf(__fdiv_rn(__fsub_rn(x, o), h)); }

// The edge: the larger of the density edge (8 cells per point over the axes the box extends along), max_dist / 16 (a query
// visits at most 17 shells) and extent / 1000; then widened by a quarter at a time until the table holds the grid.
__global__ void __launch_bounds__(64) near_params_kernel(const float* __restrict__ part, int nparts, int32_t n, float max_dist,
                                                         int64_t cap, NGrid* g) {
  __shared__ float bb[6];
  if (threadIdx.x < 6) {
    float v = part[threadIdx.x];
    for (int k = 1; k < nparts; k++) v = threadIdx.x < 3 ? fminf(v, part[k * 6 + threadIdx.x]) : fmaxf(v, part[k * 6 + threadIdx.x]);
    bb[threadIdx.x] = v;
  }
  __syncthreads();
  if (threadIdx.x) return;
  float vol = 1.0f, emax = 0.0f;
  int k = 0;
  for (int a = 0; a < 3; a++) {
    const float ext = bb[3 + a] - bb[a];
    emax = fmaxf(emax, ext);
    if (ext > 0.0f) vol *= ext, k++;
  }
  const float per = vol / (8.0f * (float)n);
  float h = k == 3 ? cbrtf(per) : (k == 2 ? sqrtf(per) : (k == 1 ? per : 0.0f));
  h = fmaxf(fmaxf(h, max_dist * 0.0625f), emax * 0.001f);
  int32_t dim[3] = {1, 1, 1};
  float o[3] = {0.f, 0.f, 0.f};
  for (int it = 0; it < 64; it++) {
    int64_t cells = 1;
    bool fits = true;
    for (int a = 0; a < 3; a++) {
      o[a] = floorf(bb[a] / h) * h;
      if (!(o[a] <= bb[a])) o[a] = bb[a];                          // (the product rounded up: no point may lie below the origin)
      const float top = cell_coord(bb[3 + a], o[a], h);
      fits = fits && top >= 0.0f && top < (float)GRID_MAX_DIM;
      dim[a] = fits ? (int32_t)top + 1 : 1;
      cells *= dim[a];
    }
    if (fits && cells <= cap) break;
    h *= 1.25f;
    if (it == 63) dim[0] = dim[1] = dim[2] = 1;                   // (not finite: one cell, every index stays inside the table)
  }
  for (int a = 0; a < 3; a++) g->o[a] = o[a], g->dim[a] = dim[a];
  g->h = h;
  const int32_t md = max(dim[0], max(dim[1], dim[2]));
  const float reach = ceilf(max_dist / h) + 1.0f;                 // shells further out lie beyond max_dist
  g->nshell = reach < (float)md ? (int32_t)reach : md;
}

__device__ __forceinline__ int32_t clamp_cell(float c, int32_t lo, int32_t hi) { return (int32_t)fminf(fmaxf(c, (float)lo), (float)hi); }

__global__ void __launch_bounds__(TPB) near_cell_kernel(int32_t n, const float* __restrict__ pts, const NGrid* __restrict__ gp,
                                                        uint32_t* __restrict__ codes) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const NGrid g = *gp;
  int32_t c[3];
#pragma unroll
  for (int a = 0; a < 3; a++) c[a] = clamp_cell(cell_coord(pts[3 * i + a], g.o[a], g.h), 0, g.dim[a] - 1);
  codes[i] = (uint32_t)((c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0]);
}

__global__ void __launch_bounds__(TPB) near_build_kernel(int32_t n, const float* __restrict__ pts, const uint32_t* __restrict__ skey,
                                                         const uint32_t* __restrict__ sval, int64_t cap, float4* __restrict__ sorted,
                                                         uint2* __restrict__ cells) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = skey[i], src = sval[i];
  if (src < (uint32_t)n) sorted[i] = make_float4(pts[3 * (size_t)src], pts[3 * (size_t)src + 1], pts[3 * (size_t)src + 2], 0.0f);
  if (key >= (uint64_t)cap) return;
  if (i == 0 || skey[i - 1] != key) cells[key].x = (uint32_t)i;
  if (i == n - 1 || skey[i + 1] != key) cells[key].y = (uint32_t)(i + 1);
}

// Thread = query.  Shell s is the set of cells at Chebyshev distance s from the query's cell (the query's own coordinate is
// clamped to [-1, dim], which only brings it nearer to the grid).  The cell coordinate is a monotone function of x, the same
// for points and queries, and differs from (x - o) / h by at most 2^-23 of its value, i.e. 2^-12 of a cell over 1024 cells;
// so a point in shell s >= 2 is farther than (s - 1 - 2^-11) h from the query along one axis.  The bound used is
// ((s - 1) - 2^-8) h scaled by 0.9999 (eight times that slack, and room for the roundings of the bound and of d2
// themselves): the walk stops at the first shell whose bound, squared, exceeds the best squared distance so far or
// max_dist^2 (scaled UP by 1.0002), and every later shell is farther still.  Shells 0 and 1 are always visited.
__global__ void __launch_bounds__(TPB) near_query_kernel(int64_t na, const float* __restrict__ a, const NGrid* __restrict__ gp,
                                                         const uint2* __restrict__ cells, const float4* __restrict__ sorted,
                                                         float max_dist, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= na) return;
  const NGrid g = *gp;
  const float qx = a[3 * i], qy = a[3 * i + 1], qz = a[3 * i + 2];
  const int32_t nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
  const int32_t cx = clamp_cell(cell_coord(qx, g.o[0], g.h), -1, nx), cy = clamp_cell(cell_coord(qy, g.o[1], g.h), -1, ny),
                cz = clamp_cell(cell_coord(qz, g.o[2], g.h), -1, nz);
  const float md2 = max_dist * max_dist * 1.0002f;
  float best = INFINITY;
  auto scan = [&](int32_t x, int32_t y, int32_t z) {
    const uint2 r = cells[((size_t)z * ny + y) * nx + x];
    for (uint32_t j = r.x; j < r.y; j++) {
      const float4 p = sorted[j];
      const float dx = __fsub_rn(qx, p.x), dy = __fsub_rn(qy, p.y), dz = __fsub_rn(qz, p.z);
      best = fminf(best, __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    }
  };
  for (int32_t s = 0; s <= g.nshell; s++) {
    if (s >= 2) {
      const float lb = ((float)(s - 1) - 0.00390625f) * g.h * 0.9999f;
      if (lb * lb > fminf(best, md2)) break;
    }
    const int32_t z0 = max(cz - s, 0), z1 = min(cz + s, nz - 1), y0 = max(cy - s, 0), y1 = min(cy + s, ny - 1);
    const int32_t x0 = max(cx - s, 0), x1 = min(cx + s, nx - 1);
    for (int32_t z = z0; z <= z1; z++)
      for (int32_t y = y0; y <= y1; y++) {
        if (z - cz == s || cz - z == s || y - cy == s || cy - y == s) {
          for (int32_t x = x0; x <= x1; x++) scan(x, y, z);
        } else {
          if (cx - s >= 0 && cx - s < nx) scan(cx - s, y, z);
          if (s > 0 && cx + s >= 0 && cx + s < nx) scan(cx + s, y, z);
        }
      }
  }
  out[i] = fminf(max_dist, sqrt_rn(best));
}

// The same walk, keeping the point as well: sidx[j] is the index in b of sorted[j].  Among equal d2 the smallest index wins,
// whatever the order of the cells and of the points inside one; the strict bound test above never cuts off an equal d2.
__global__ void __launch_bounds__(TPB) near_query_index_kernel(int64_t na, const float* __restrict__ a, const NGrid* __restrict__ gp,
                                                               const uint2* __restrict__ cells, const float4* __restrict__ sorted,
                                                               const uint32_t* __restrict__ sidx, float max_dist, float* __restrict__ out,
                                                               int32_t* __restrict__ index) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= na) return;
  const NGrid g = *gp;
  const float qx = a[3 * i], qy = a[3 * i + 1], qz = a[3 * i + 2];
  const int32_t nx = g.dim[0], ny = g.dim[1], nz = g.dim[2];
  const int32_t cx = clamp_cell(cell_coord(qx, g.o[0], g.h), -1, nx), cy = clamp_cell(cell_coord(qy, g.o[1], g.h), -1, ny),
                cz = clamp_cell(cell_coord(qz, g.o[2], g.h), -1, nz);
  const float md2 = max_dist * max_dist * 1.0002f;
  float best = INFINITY;
  uint32_t bidx = 0xFFFFFFFFu;
  auto scan = [&](int32_t x, int32_t y, int32_t z) {
    const uint2 r = cells[((size_t)z * ny + y) * nx + x];
    for (uint32_t j = r.x; j < r.y; j++) {
      const float4 p = sorted[j];
      const float dx = __fsub_rn(qx, p.x), dy = __fsub_rn(qy, p.y), dz = __fsub_rn(qz, p.z);
      const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
      const uint32_t src = sidx[j];
      if (d2 < best || (d2 == best && src < bidx)) best = d2, bidx = src;
    }
  };
  for (int32_t s = 0; s <= g.nshell; s++) {
    if (s >= 2) {
      const float lb = ((float)(s - 1) - 0.00390625f) * g.h * 0.9999f;
      if (lb * lb > fminf(best, md2)) break;
    }
    const int32_t z0 = max(cz - s, 0), z1 = min(cz + s, nz - 1), y0 = max(cy - s, 0), y1 = min(cy + s, ny - 1);
    const int32_t x0 = max(cx - s, 0), x1 = min(cx + s, nx - 1);
    for (int32_t z = z0; z <= z1; z++)
      for (int32_t y = y0; y <= y1; y++) {
        if (z - cz == s || cz - z == s || y - cy == s || cy - y == s) {
          for (int32_t x = x0; x <= x1; x++) scan(x, y, z);
        } else {
          if (cx - s >= 0 && cx - s < nx) scan(cx - s, y, z);
          if (s > 0 && cx + s >= 0 && cx + s < nx) scan(cx + s, y, z);
        }
      }
  }
  const float d = sqrt_rn(best);
  out[i] = fminf(max_dist, d);
  index[i] = (bidx != 0xFFFFFFFFu && d <= max_dist) ? (int32_t)bidx : -1;
}

// ---- the score of one direction ----------------------------------------------------------------------------------------
constexpr int SCORE_Q = 3;            // sum of the distances, points counted, points nearer than tau

static int score_blocks(int64_t n) {
  const int64_t b = (n + 8 * TPB - 1) / (8 * TPB);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

__global__ void __launch_bounds__(TPB) score_partial_kernel(int64_t n, const float* __restrict__ dist, const uint8_t* __restrict__ mask,
                                                            float tau, int nb, double* __restrict__ part) {
  double q[SCORE_Q] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)nb * TPB) {
    if (mask && !mask[i]) continue;
    const float d = dist[i];
    q[0] += (double)d;
    q[1] += 1.0;
    if (d < tau) q[2] += 1.0;
  }
  __shared__ double red[TPB / 64][SCORE_Q];
  b3gs_block_sum_f64<TPB>(q, red, part + (size_t)blockIdx.x * SCORE_Q);
}

// one wave: fixed assignment of partials to lanes, fixed tree
__global__ void __launch_bounds__(64) score_fold_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  for (int k = 0; k < SCORE_Q; k++) {
    const double s = b3gs_wave_fold_f64(part + k, nb, SCORE_Q);
    if (threadIdx.x == 0) out[k] = s;
  }
}

static bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int b3gs_mesh_components(int32_t V, int64_t F, const int32_t* faces, int32_t* labels, int32_t* tri_count, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_components";
  if (V < 0 || F < 0 || F > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V, 0 <= F <= 2^31 - 1");
  if ((V > 0 && (!labels || !tri_count)) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (V == 0) return B3GS_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, labels, tri_count);
  if (F > 0) hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_of(3 * F)), dim3(TPB), 0, s, V, F, faces, labels);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, labels);
  if (F > 0) hipLaunchKernelGGL(cc_count_kernel, dim3(blocks_of(F)), dim3(TPB), 0, s, V, F, faces, (const int32_t*)labels, tri_count);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_mesh_clean_workspace_bytes(int64_t V, int64_t F) {
  CleanLayout l;
  return clean_layout(V, F, &l) ? l.total : 0;
}

extern "C" int b3gs_mesh_clean_count(int32_t V, int64_t F, const int32_t* faces, const int32_t* labels, const int32_t* tri_count,
                                     const int32_t* threshold, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_clean_count";
  CleanLayout l;
  if (!clean_layout(V, F, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (!threshold || (V > 0 && (!labels || !tri_count)) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  CleanArgs a = clean_args(V, F, l, workspace);
  a.faces = faces, a.labels = labels, a.tri_count = tri_count, a.threshold = threshold;
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(workspace, 0, 256, s);
  if (V > 0) hipLaunchKernelGGL(clean_vcount_kernel, dim3((unsigned)l.nbv), dim3(TPB), 0, s, a);
  if (F > 0) hipLaunchKernelGGL(clean_fcount_kernel, dim3((unsigned)l.nbf), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(clean_scan_kernel, dim3(2), dim3(SCAN_TPB), 0, s, a);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_clean_emit(int32_t V, int64_t F, const float* vertices, const uint8_t* colours, const int32_t* faces,
                                    const int32_t* labels, const int32_t* tri_count, const int32_t* threshold, void* workspace,
                                    int64_t nverts, int64_t ntris, float* out_vertices, uint8_t* out_colours, int32_t* out_faces,
                                    b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_clean_emit";
  CleanLayout l;
  if (!clean_layout(V, F, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (nverts < 0 || ntris < 0 || nverts > V || ntris > F) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= nverts <= V, 0 <= ntris <= F");
  if (!threshold || (V > 0 && (!labels || !tri_count || !vertices || !colours)) || (F > 0 && !faces) ||
      (nverts > 0 && (!out_vertices || !out_colours)) || (ntris > 0 && !out_faces))
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (nverts == 0 && ntris == 0) return B3GS_OK;
  CleanArgs a = clean_args(V, F, l, workspace);
  a.faces = faces, a.labels = labels, a.tri_count = tri_count, a.threshold = threshold;
  a.nverts = nverts, a.ntris = ntris, a.vertices = vertices, a.colours = colours;
  a.out_vertices = out_vertices, a.out_colours = out_colours, a.out_faces = out_faces;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(clean_vemit_kernel, dim3((unsigned)l.nbv), dim3(TPB), 0, s, a);
  if (ntris > 0) hipLaunchKernelGGL(clean_femit_kernel, dim3((unsigned)l.nbf), dim3(TPB), 0, s, a);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_mesh_sample_workspace_bytes(int64_t F) {
  SampleLayout l;
  return sample_layout(F, &l) ? l.total : 0;
}

static int sample_args(const char* what, int32_t V, int64_t F, const float* vertices, const int32_t* faces, float spacing,
                       void* workspace, SampleArgs* a) {
  SampleLayout l;
  if (V < 0 || !sample_layout(F, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V, F <= 2^31 - 1");
  if (!(spacing > 0.0f) || !(spacing <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "the spacing is positive and finite");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if ((V > 0 && !vertices) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  char* ws = static_cast<char*>(workspace);
  *a = SampleArgs{};
  a->V = V, a->F = F, a->nbf = l.nbf, a->vertices = vertices, a->faces = faces, a->spacing = spacing;
  a->totals = reinterpret_cast<int64_t*>(ws);
  a->nn = reinterpret_cast<uint32_t*>(ws + l.nn);
  a->bsum = reinterpret_cast<uint32_t*>(ws + l.bsum);
  return B3GS_OK;
}

extern "C" int b3gs_mesh_sample_count(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float spacing, void* workspace,
                                      b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_sample_count";
  SampleArgs a;
  if (int rc = sample_args(what, V, F, vertices, faces, spacing, workspace, &a)) return rc;
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(workspace, 0, 256, s);
  if (F > 0) {
    hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)a.nbf), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(sample_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, a);
  }
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_sample_emit(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float spacing, void* workspace,
                                     int64_t npoints, float* points, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_sample_emit";
  SampleArgs a;
  if (int rc = sample_args(what, V, F, vertices, faces, spacing, workspace, &a)) return rc;
  if (npoints < 0 || (int64_t)V + npoints > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "more than 2^31 - 1 points: use a larger spacing");
  if ((int64_t)V + npoints > 0 && !points) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output");
  hipStream_t s = (hipStream_t)stream;
  if (V > 0 && hipMemcpyAsync(points, vertices, (size_t)V * 3 * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
    return b3gs_launch_status(what);
  if (npoints > 0 && F > 0) {
    a.npoints = npoints, a.points = points + 3 * (size_t)V;
    hipLaunchKernelGGL(sample_emit_kernel, dim3((unsigned)a.nbf), dim3(TPB), 0, s, a);
  }
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_nearest_workspace_bytes(int64_t Nb) {
  if (Nb < 1 || Nb > INT32_MAX) return 0;
  return near_carve(nullptr, Nb, nullptr);
}

extern "C" int b3gs_nearest_grid(int64_t Nb, const float* b, float max_dist, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_nearest_grid";
  if (Nb < 1 || Nb > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "the cloud searched holds 1 .. 2^31 - 1 points");
  if (!(max_dist > 0.0f) || !(max_dist <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "max_dist is positive and finite");
  if (!b) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  NearWs w;
  near_carve(static_cast<char*>(workspace), Nb, &w);
  const int32_t n = (int32_t)Nb;
  const int64_t cap = cell_capacity(Nb);
  const int nparts = (int)(blocks_of(n) < 256u ? blocks_of(n) : 256u);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(near_bbox_kernel, dim3(nparts), dim3(TPB), 0, s, n, b, w.part);
  hipLaunchKernelGGL(near_params_kernel, dim3(1), dim3(64), 0, s, (const float*)w.part, nparts, n, max_dist, cap, w.grid);
  hipLaunchKernelGGL(near_cell_kernel, dim3(blocks_of(n)), dim3(TPB), 0, s, n, b, (const NGrid*)w.grid, w.codes);
  b3gs_launch_sort_u32_index(w.codes, w.skey, w.sval, (uint32_t)n, w.hist, s);
  (void)hipMemsetAsync(w.cells, 0, (size_t)cap * sizeof(uint2), s);
  hipLaunchKernelGGL(near_build_kernel, dim3(blocks_of(n)), dim3(TPB), 0, s, n, b, (const uint32_t*)w.skey[0], (const uint32_t*)w.sval[0], cap,
                     w.sorted, w.cells);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_nearest_query(int64_t Na, const float* a, int64_t Nb, float max_dist, const void* workspace, float* out,
                                  b3gs_stream_t stream) {
  static const char* what = "b3gs_nearest_query";
  if (Na < 0 || Na > INT32_MAX || Nb < 1 || Nb > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= Na <= 2^31 - 1, 1 <= Nb <= 2^31 - 1");
  if (!(max_dist > 0.0f) || !(max_dist <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "max_dist is positive and finite");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (Na == 0) return B3GS_OK;
  if (!a || !out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  NearWs w;
  near_carve(static_cast<char*>(const_cast<void*>(workspace)), Nb, &w);
  hipLaunchKernelGGL(near_query_kernel, dim3(blocks_of(Na)), dim3(TPB), 0, (hipStream_t)stream, Na, a, (const NGrid*)w.grid,
                     (const uint2*)w.cells, (const float4*)w.sorted, max_dist, out);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_nearest_query_index(int64_t Na, const float* a, int64_t Nb, float max_dist, const void* workspace, float* out,
                                        int32_t* index, b3gs_stream_t stream) {
  static const char* what = "b3gs_nearest_query_index";
  if (Na < 0 || Na > INT32_MAX || Nb < 1 || Nb > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= Na <= 2^31 - 1, 1 <= Nb <= 2^31 - 1");
  if (!(max_dist > 0.0f) || !(max_dist <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "max_dist is positive and finite");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (Na == 0) return B3GS_OK;
  if (!a || !out || !index) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  NearWs w;
  near_carve(static_cast<char*>(const_cast<void*>(workspace)), Nb, &w);
  hipLaunchKernelGGL(near_query_index_kernel, dim3(blocks_of(Na)), dim3(TPB), 0, (hipStream_t)stream, Na, a, (const NGrid*)w.grid,
                     (const uint2*)w.cells, (const float4*)w.sorted, (const uint32_t*)w.sval[0], max_dist, out, index);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_cloud_score_workspace_bytes(int64_t N) {
  if (N < 1 || N > INT32_MAX) return 0;
  return b3gs_align256((size_t)score_blocks(N) * SCORE_Q * sizeof(double));
}

extern "C" int b3gs_cloud_score(int64_t N, const float* dist, const uint8_t* mask, float tau, double* out, void* workspace,
                                b3gs_stream_t stream) {
  static const char* what = "b3gs_cloud_score";
  if (N < 1 || N > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 2^31 - 1 distances");
  if (tau != tau) return b3gs_fail(B3GS_ERR_ARG, what, "tau is NaN");
  if (!dist || !out || !workspace) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  const int nb = score_blocks(N);
  double* part = static_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(score_partial_kernel, dim3(nb), dim3(TPB), 0, s, N, dist, mask, tau, nb, part);
  hipLaunchKernelGGL(score_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)part, nb, out);
  return b3gs_launch_status(what);
}
