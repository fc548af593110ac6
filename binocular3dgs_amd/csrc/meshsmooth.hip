// Smoothing an extracted mesh (entry points added to ABI 18; binocular3dgs_amd/mesh_tools.py): the vertex
// adjacency, the Taubin filter, area-weighted vertex normals and the shaded resolve of the mesh rasterizer.
// include/b3gs_raster.h states the arithmetic statement by statement; tests/meshsmooth_ref.py restates it.  Every step is integer
// work, a stable sort, an ordered scan, or fp64 / float32 statements of one operation each that ONE thread executes in one fixed
// order (the file is compiled with -ffp-contract=off): every output is one fixed result.  No floating-point atomic anywhere.
//   build   finite    thread = vertex: coordinates that are not finite are counted
//           pairs     thread = face: the six ordered pairs and the three incidence slots; bad and good faces counted
//           incidence the slots sorted stably by vertex: per vertex its faces in face-index order
//           2 sorts   the pairs by second, then by first (each stable, the orders composed): equal pairs are adjacent
//           heads     head flags of the sorted pairs -> block sums -> scan -> the distinct pairs: the neighbour indices
//           edges     the head of a run with first < second is an undirected edge, the run length its face count
//           offsets   thread = vertex: the lower bound of the vertex among the firsts of the distinct pairs
//   smooth  pack      [V, 3] -> float4 rows; one launch per step, thread = vertex, ping -> pong; unpack
//   normals thread = vertex: its faces in face-index order
//   shaded  resolve_kernel of meshraster.hip with the colour taken from the interpolated vertex normal
#include "b3gs_internal.h"
#include "mesh_tri.h"
#include <cfloat>

namespace {

constexpr int TPB = MESH_TPB;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;       // a pair or an incidence slot that takes no part (vertex indices stay below 2^31)

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// words of the totals (int64 each) at the head of the workspace; T_PAIRS (the distinct ordered pairs) is the library's own
enum { T_BAD_FACES = 0, T_NONFINITE, T_EDGES, T_BOUNDARY, T_NONMANIFOLD, T_PINNED, T_ISOLATED, T_GOOD_FACES, T_PAIRS, T_WORDS };

struct AdjWs {
  int64_t* totals;
  int32_t* nbr_off;                 // [V + 1] CSR offsets of the neighbour lists
  int32_t* nbr_idx;                 // [6 F]   the neighbours of vertex i, ascending, at nbr_off[i] .. nbr_off[i + 1]
  uint2* inc;                       // [V]     {first, one past last} incident face of every vertex in inc_face
  int32_t* inc_face;                // [3 F]   face indices, per vertex in face-index order
  uint8_t* pinned;                  // [V]     an end of an edge whose face count is not 2
  float4* pos[2];                   // [V]     ping / pong of the filter
  uint32_t* skey[2];                // [6 F]   sort ping / pong
  uint32_t* sval[2];
  uint32_t* hist;
  uint32_t* pa;                     // [6 F]   first of every ordered pair, in face order
  uint32_t* pb;                     // [6 F]   second
  uint32_t* ord;                    // [6 F]   the order after the sort by second
  uint32_t* gkey;                   // [6 F]   the keys of the second sort, gathered in that order
  uint32_t* sb;                     // [6 F]   the seconds in the final order (the firsts are skey[0])
  int32_t* dfirst;                  // [6 F]   first of distinct pair k
  uint32_t* bsum;                   // [blocks of 6 F] head flags
};

// base == nullptr: only the size and the offsets are wanted; the pointers are then carved from ADJ_NO_BASE
static char* const ADJ_NO_BASE = reinterpret_cast<char*>((uintptr_t)1 << 20);

// (tests/test_gpu_sort_u32_index.py reads gkey, skey[0] and sval[0] of the build's last sort back from this layout: keep them in step)
static size_t adj_carve(char* base, int64_t V, int64_t F, AdjWs* w) {
  if (!base) base = ADJ_NO_BASE;
  char* cur = base;
  const size_t v = (size_t)(V > 0 ? V : 1), f = (size_t)(F > 0 ? F : 1), n = 6 * f;
  AdjWs t;
  t.totals = b3gs_carve<int64_t>(cur, 32);                           // one 256-byte head
  t.nbr_off = b3gs_carve<int32_t>(cur, v + 1);
  t.nbr_idx = b3gs_carve<int32_t>(cur, n);
  t.inc = b3gs_carve<uint2>(cur, v);
  t.inc_face = b3gs_carve<int32_t>(cur, 3 * f);
  t.pinned = b3gs_carve<uint8_t>(cur, v);
  for (int k = 0; k < 2; k++) t.pos[k] = b3gs_carve<float4>(cur, v);
  for (int k = 0; k < 2; k++) t.skey[k] = b3gs_carve<uint32_t>(cur, n);
  for (int k = 0; k < 2; k++) t.sval[k] = b3gs_carve<uint32_t>(cur, n);
  t.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)n));
  t.pa = b3gs_carve<uint32_t>(cur, n);
  t.pb = b3gs_carve<uint32_t>(cur, n);
  t.ord = b3gs_carve<uint32_t>(cur, n);
  t.gkey = b3gs_carve<uint32_t>(cur, n);
  t.sb = b3gs_carve<uint32_t>(cur, n);
  t.dfirst = b3gs_carve<int32_t>(cur, n);
  t.bsum = b3gs_carve<uint32_t>(cur, blocks_of((int64_t)n));
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

// ---- build -------------------------------------------------------------------------------------------------------------
// What the calls add into or write only in part is zeroed by these two kernels, not by memset nodes: replayed from a captured
// graph a second time, a 256-byte hipMemsetAsync that another memset follows directly was seen to fill the head with a
// pattern that is not zero (tests/test_gpu_meshsmooth.py replays three times).
__global__ void __launch_bounds__(TPB) adj_clear_kernel(int32_t V, int64_t* __restrict__ head, uint2* __restrict__ inc, uint8_t* __restrict__ pinned) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i < 32) head[i] = 0;                                          // the 256-byte head: the totals
  if (i < V) inc[i] = make_uint2(0u, 0u), pinned[i] = 0;
}
__global__ void __launch_bounds__(B3GS_WAVE) adj_clear_word_kernel(int64_t* word) {
  if (threadIdx.x == 0) *word = 0;
}

__global__ void __launch_bounds__(TPB) adj_finite_kernel(int32_t V, const float* __restrict__ pts, int64_t* totals) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool bad = false;
  if (i < V) {
#pragma unroll
    for (int a = 0; a < 3; a++) bad = bad || !(fabsf(pts[3 * i + a]) <= FLT_MAX);      // (true for NaN and for either infinity)
  }
  count_flags(totals + T_NONFINITE, bad);
}

// pairs 6 t .. 6 t + 5: (a,b), (b,a), (b,c), (c,b), (c,a), (a,c), a pair with equal ends dropped; slot 3 t + x: corner x, unless an
// earlier corner of the face names the vertex already
__global__ void __launch_bounds__(TPB) adj_pairs_kernel(int32_t V, int64_t F, const int32_t* __restrict__ faces, uint32_t* __restrict__ pa,
                                                        uint32_t* __restrict__ pb, uint32_t* __restrict__ slots, int64_t* totals) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool bad = false, good = false;
  if (t < F) {
    const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    good = face_ok(f, V);
    bad = !good;
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const uint32_t x = (uint32_t)f[e], y = (uint32_t)f[e == 2 ? 0 : e + 1];
      const bool live = good && x != y;
      pa[6 * t + 2 * e] = live ? x : NO_KEY, pb[6 * t + 2 * e] = live ? y : NO_KEY;
      pa[6 * t + 2 * e + 1] = live ? y : NO_KEY, pb[6 * t + 2 * e + 1] = live ? x : NO_KEY;
    }
    uint32_t a = NO_KEY, b = NO_KEY, c = NO_KEY;
    if (good) {
      a = (uint32_t)f[0], b = (uint32_t)f[1], c = (uint32_t)f[2];
      if (c == a || c == b) c = NO_KEY;
      if (b == a) b = NO_KEY;
    }
    slots[3 * t] = a, slots[3 * t + 1] = b, slots[3 * t + 2] = c;
  }
  count_flags(totals + T_BAD_FACES, bad);
  count_flags(totals + T_GOOD_FACES, good);
}

__global__ void __launch_bounds__(TPB) adj_inc_kernel(int64_t n, int32_t V, const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                                      uint2* __restrict__ inc, int32_t* __restrict__ inc_face) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  inc_face[i] = (int32_t)(sval[i] / 3u);
  const uint32_t key = skey[i];
  if (key >= (uint32_t)V) return;                                   // (NO_KEY slots sort behind every vertex)
  if (i == 0 || skey[i - 1] != key) inc[key].x = (uint32_t)i;
  if (i == n - 1 || skey[i + 1] != key) inc[key].y = (uint32_t)(i + 1);
}

// order_out[i] = order_in[perm[i]] (order_in null: the identity), key_out[i] = key[order_out[i]]
__global__ void __launch_bounds__(TPB) adj_compose_kernel(int64_t n, const uint32_t* __restrict__ order_in, const uint32_t* __restrict__ perm,
                                                          const uint32_t* __restrict__ key, uint32_t* __restrict__ order_out,
                                                          uint32_t* __restrict__ key_out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  uint32_t p = perm[i];
  if (p >= (uint64_t)n) p = 0u;                                      // (a permutation of 0 .. n-1: never taken)
  uint32_t e = order_in ? order_in[p] : p;
  if (e >= (uint64_t)n) e = 0u;
  if (order_out) order_out[i] = e;
  key_out[i] = key[e];
}

__device__ __forceinline__ int head_flag(const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb, int64_t i, int64_t n) {
  return i < n && sa[i] != NO_KEY && (i == 0 || sa[i] != sa[i - 1] || sb[i] != sb[i - 1]);
}

__global__ void __launch_bounds__(TPB) adj_head_count_kernel(int64_t n, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb,
                                                             uint32_t* __restrict__ bsum) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int total;
  b3gs_block_rank<TPB, 1>(head_flag(sa, sb, i, n), wave_n, &total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(SCAN_TPB) adj_scan_kernel(uint32_t* bsum, int nb, int64_t* total) { b3gs_scan_block_sums(bsum, nb, total); }

// distinct pair k = the heads in front of sorted position i; the head of a run with first < second is an undirected edge and the
// run length the number of good faces that contain it (each names the ordered pair once)
__global__ void __launch_bounds__(TPB) adj_emit_kernel(int64_t n, const uint32_t* __restrict__ sa, const uint32_t* __restrict__ sb,
                                                       const uint32_t* __restrict__ bsum, int32_t* __restrict__ nbr_idx,
                                                       int32_t* __restrict__ dfirst, uint8_t* __restrict__ pinned, int64_t* totals) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int flag = head_flag(sa, sb, i, n);
  int total;
  const int64_t k = (int64_t)bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(flag, wave_n, &total);
  bool edge = false, boundary = false, nonmanifold = false;
  if (flag && k < n) {
    const uint32_t a = sa[i], b = sb[i];
    nbr_idx[k] = (int32_t)b;
    dfirst[k] = (int32_t)a;
    if (a < b) {
      int64_t j = i + 1;
      while (j < n && sa[j] == a && sb[j] == b) j++;
      const int64_t m = j - i;
      edge = true, boundary = m == 1, nonmanifold = m > 2;
      if (m != 2) pinned[a] = 1, pinned[b] = 1;                       // (the same byte from every writer; a < b < V: live pairs name vertices)
    }
  }
  count_flags(totals + T_EDGES, edge);
  count_flags(totals + T_BOUNDARY, boundary);
  count_flags(totals + T_NONMANIFOLD, nonmanifold);
}

// nbr_off[v] = the distinct pairs whose first is below v, v = 0 .. V
__global__ void __launch_bounds__(TPB) adj_offsets_kernel(int32_t V, int64_t n, const int32_t* __restrict__ dfirst, const int64_t* __restrict__ totals,
                                                          int32_t* __restrict__ nbr_off) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (v > V) return;
  int64_t lo = 0, hi = min(max(totals[T_PAIRS], (int64_t)0), n);
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)dfirst[mid] < v) lo = mid + 1; else hi = mid;
  }
  nbr_off[v] = (int32_t)lo;
}

__global__ void __launch_bounds__(TPB) adj_class_kernel(int32_t V, const int32_t* __restrict__ nbr_off, const uint8_t* __restrict__ pinned,
                                                        int64_t* totals) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const bool in = v < V;
  count_flags(totals + T_PINNED, in && pinned[v] != 0);
  count_flags(totals + T_ISOLATED, in && nbr_off[v + 1] == nbr_off[v]);
}

// ---- the filter --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) smooth_pack_kernel(int32_t V, const float* __restrict__ pts, float4* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i < V) pos[i] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], 0.0f);
}

__global__ void __launch_bounds__(TPB) smooth_unpack_kernel(int32_t V, const float4* __restrict__ pos, float* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const float4 p = pos[i];
  pts[3 * i] = p.x, pts[3 * i + 1] = p.y, pts[3 * i + 2] = p.z;
}

// One Jacobi step with factor k.  Thread = vertex; every fp64 statement is one operation, the neighbours in ascending order:
// tests/meshsmooth_ref.py walks the same statements.  A neighbour is one 16-byte load.
__global__ void __launch_bounds__(TPB) smooth_step_kernel(int32_t V, int32_t n, const float4* __restrict__ in, float4* __restrict__ out,
                                                          const int32_t* __restrict__ nbr_off, const int32_t* __restrict__ nbr_idx,
                                                          const uint8_t* __restrict__ pinned, double k, int32_t pin) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const float4 p = in[i];
  const int32_t j0 = nbr_off[i], j1 = min(nbr_off[i + 1], n);
  float4 q = p;
  if (j0 >= 0 && j1 > j0 && !(pin && pinned[i])) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int32_t j = j0; j < j1; j++) {
      const uint32_t v = (uint32_t)nbr_idx[j];
      if (v >= (uint32_t)V) continue;                               // (a list of this mesh names vertices: never taken)
      const float4 o = in[v];
      sx += (double)o.x, sy += (double)o.y, sz += (double)o.z;
    }
    const double deg = (double)(j1 - j0);
    const double mx = sx / deg, my = sy / deg, mz = sz / deg;
    const double dx = mx - (double)p.x, dy = my - (double)p.y, dz = mz - (double)p.z;
    const double tx = k * dx, ty = k * dy, tz = k * dz;
    q.x = (float)((double)p.x + tx), q.y = (float)((double)p.y + ty), q.z = (float)((double)p.z + tz);
  }
  out[i] = q;
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------
// Thread = vertex: the area-weighted sum of its faces' normals, in face-index order, then the unit vector.
__global__ void __launch_bounds__(TPB) vertex_normals_kernel(int32_t V, int64_t F, const float* __restrict__ pts, const int32_t* __restrict__ faces,
                                                             const uint2* __restrict__ inc, const int32_t* __restrict__ inc_face,
                                                             float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= V) return;
  const uint2 range = inc[i];
  double Nx = 0.0, Ny = 0.0, Nz = 0.0;
  for (uint32_t j = range.x; j < range.y && j < 3ull * (uint64_t)F; j++) {
    const size_t t = (size_t)(uint32_t)inc_face[j];
    if (t >= (size_t)F) continue;
    const int32_t f[3] = {faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]};
    if (!face_ok(f, V)) continue;                                   // (an incident face names vertices: never taken)
    const size_t i0 = (size_t)f[0], i1 = (size_t)f[1], i2 = (size_t)f[2];
    const double p0x = (double)pts[3 * i0], p0y = (double)pts[3 * i0 + 1], p0z = (double)pts[3 * i0 + 2];
    const double ux = (double)pts[3 * i1] - p0x, uy = (double)pts[3 * i1 + 1] - p0y, uz = (double)pts[3 * i1 + 2] - p0z;
    const double vx = (double)pts[3 * i2] - p0x, vy = (double)pts[3 * i2 + 1] - p0y, vz = (double)pts[3 * i2 + 2] - p0z;
    const double nx = uy * vz - uz * vy;
    const double ny = uz * vx - ux * vz;
    const double nz = ux * vy - uy * vx;
    Nx += nx, Ny += ny, Nz += nz;
  }
  const double l = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
  const bool unit = l > 0.0 && l <= DBL_MAX;
  normals[3 * i] = unit ? (float)(Nx / l) : 0.0f;
  normals[3 * i + 1] = unit ? (float)(Ny / l) : 0.0f;
  normals[3 * i + 2] = unit ? (float)(Nz / l) : 0.0f;
}

// ---- the shaded resolve ------------------------------------------------------------------------------------------------
struct ShadedArgs {
  int32_t n, W, H, V;
  int64_t F;
  int32_t mode;
  const float* normals;
  const int32_t* faces;
  const SVert* sv;
  const unsigned long long* vis;
  const float* bg;
  int32_t* triangle_id;
  float* depth;
  float* alpha;
  float* colour;
  int32_t* face_pixels;
  Cam cam[NV];
};

// resolve_kernel of meshraster.hip with the colour taken from the vertex normals, interpolated like the vertex colours
__global__ void __launch_bounds__(TPB) shaded_resolve_kernel(ShadedArgs a) {
  const int64_t pix = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int view = blockIdx.y;
  const int64_t plane = (int64_t)a.W * a.H;
  if (pix >= plane) return;
  const unsigned long long word = a.vis[(size_t)view * plane + pix];
  const uint32_t f = (uint32_t)word;
  int32_t id = -1;
  float z = 0.0f, al = 0.0f, col[3] = {0.0f, 0.0f, 0.0f};
  if (a.bg)
    for (int ch = 0; ch < 3; ch++) col[ch] = a.bg[ch];
  int32_t idx[3] = {0, 0, 0};
  if (word != ~0ull && f < (uint64_t)a.F) {
    idx[0] = a.faces[3 * (size_t)f], idx[1] = a.faces[3 * (size_t)f + 1], idx[2] = a.faces[3 * (size_t)f + 2];
    if (face_ok(idx, a.V)) id = (int32_t)f;
  }
  if (id >= 0) {
    const SVert* sv = a.sv + (size_t)view * a.V;
    Tri t;
    int winding;
    int64_t E[3];
    float w[3];
    tri_setup(sv[idx[0]], sv[idx[1]], sv[idx[2]], a.W, a.H, 0, &t, &winding);
    if (winding == 0) {
      id = -1;                                                    // (not a word this mesh and these cameras can leave)
    } else {
      tri_edges(t, (int32_t)(pix % a.W), (int32_t)(pix / a.W), E);
      z = tri_depth(t, E, w);
      al = 1.0f;
      if (a.face_pixels) atomicAdd(a.face_pixels + id, 1);
      if (a.colour) {
        const Cam& c = a.cam[view];
        float g[3], q[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const float n0 = a.normals[3 * (size_t)idx[0] + r], n1 = a.normals[3 * (size_t)idx[1] + r], n2 = a.normals[3 * (size_t)idx[2] + r];
          g[r] = __fmul_rn(__fadd_rn(__fadd_rn(__fmul_rn(w[0], n0), __fmul_rn(w[1], n1)), __fmul_rn(w[2], n2)), z);
        }
#pragma unroll
        for (int r = 0; r < 3; r++)
          q[r] = __fadd_rn(__fadd_rn(__fmul_rn(c.rot[3 * r], g[0]), __fmul_rn(c.rot[3 * r + 1], g[1])), __fmul_rn(c.rot[3 * r + 2], g[2]));
        const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(q[0], q[0]), __fmul_rn(q[1], q[1])), __fmul_rn(q[2], q[2])));   // (correctly rounded)
        const bool unit = len > 0.0f && len <= FLT_MAX;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          q[r] = unit ? __fdiv_rn(q[r], len) : 0.0f;
          if (winding > 0) q[r] = -q[r];                          // clockwise as seen: the face looks away
        }
        if (a.mode == B3GS_MESH_SHADE_SMOOTH) {
#pragma unroll
          for (int r = 0; r < 3; r++) col[r] = __fmul_rn(__fadd_rn(q[r], 1.0f), 0.5f);
        } else {                                                  // a grey headlight
          const float lit = fmaxf(-q[2], 0.0f);
          float v = __fmul_rn(0.85f, lit);
          v = __fadd_rn(v, 0.15f);
          col[0] = v, col[1] = v, col[2] = v;
        }
      }
    }
  }
  const size_t o = (size_t)view * plane + pix;
  if (a.triangle_id) a.triangle_id[o] = id;
  if (a.depth) a.depth[o] = z;
  if (a.alpha) a.alpha[o] = al;
  if (a.colour)
    for (int ch = 0; ch < 3; ch++) a.colour[((size_t)view * 3 + ch) * plane + pix] = col[ch];
}

static bool sizes_ok(int64_t V, int64_t F) { return V >= 0 && F >= 0 && V <= INT32_MAX && F <= INT32_MAX / 6; }

static int check_common(const char* what, int32_t V, int64_t F, const void* workspace) {
  if (!sizes_ok(V, F)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V <= 2^31 - 1, 0 <= 6 F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  return B3GS_OK;
}

// the vertices of this call: word 1 of the totals
static void count_nonfinite(int32_t V, const float* vertices, const AdjWs& w, hipStream_t s) {
  hipLaunchKernelGGL(adj_clear_word_kernel, dim3(1), dim3(B3GS_WAVE), 0, s, w.totals + T_NONFINITE);
  if (V > 0) hipLaunchKernelGGL(adj_finite_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, vertices, w.totals);
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_mesh_adjacency_workspace_bytes(int64_t V, int64_t F) {
  if (!sizes_ok(V, F)) return 0;
  return adj_carve(nullptr, V, F, nullptr);
}

extern "C" int b3gs_mesh_adjacency_layout(int64_t V, int64_t F, size_t* offsets) {
  static const char* what = "b3gs_mesh_adjacency_layout";
  if (!sizes_ok(V, F)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V <= 2^31 - 1, 0 <= 6 F <= 2^31 - 1");
  if (!offsets) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  AdjWs w;
  adj_carve(nullptr, V, F, &w);
  const void* part[5] = {w.nbr_off, w.nbr_idx, w.inc, w.inc_face, w.pinned};
  for (int k = 0; k < 5; k++) offsets[k] = (size_t)(static_cast<const char*>(part[k]) - ADJ_NO_BASE);
  return B3GS_OK;
}

extern "C" int b3gs_mesh_adjacency_build(int32_t V, int64_t F, const float* vertices, const int32_t* faces, void* workspace,
                                         b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_adjacency_build";
  if (int rc = check_common(what, V, F, workspace)) return rc;
  if ((V > 0 && !vertices) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  AdjWs w;
  adj_carve(static_cast<char*>(workspace), V, F, &w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adj_clear_kernel, dim3(blocks_of(V > 32 ? V : 32)), dim3(TPB), 0, s, V, w.totals, w.inc, w.pinned);
  if (V > 0) hipLaunchKernelGGL(adj_finite_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, vertices, w.totals);
  const int64_t n = 6 * F, n3 = 3 * F;
  if (F > 0) {
    const unsigned nbf = blocks_of(F), nbn = blocks_of(n);
    // the slots go to skey[0]: the first pass of the sort reads them there and writes skey[1], the second one replaces them
    hipLaunchKernelGGL(adj_pairs_kernel, dim3(nbf), dim3(TPB), 0, s, V, F, faces, w.pa, w.pb, w.skey[0], w.totals);
    b3gs_launch_sort_u32_index(w.skey[0], w.skey, w.sval, (uint32_t)n3, w.hist, s);
    hipLaunchKernelGGL(adj_inc_kernel, dim3(blocks_of(n3)), dim3(TPB), 0, s, n3, V, (const uint32_t*)w.skey[0], (const uint32_t*)w.sval[0], w.inc,
                       w.inc_face);
    // stable sorts by second, then by first: the last one decides, ties keep the order of the sort before
    b3gs_launch_sort_u32_index(w.pb, w.skey, w.sval, (uint32_t)n, w.hist, s);
    hipLaunchKernelGGL(adj_compose_kernel, dim3(nbn), dim3(TPB), 0, s, n, (const uint32_t*)nullptr, (const uint32_t*)w.sval[0],
                       (const uint32_t*)w.pa, w.ord, w.gkey);
    b3gs_launch_sort_u32_index(w.gkey, w.skey, w.sval, (uint32_t)n, w.hist, s);
    hipLaunchKernelGGL(adj_compose_kernel, dim3(nbn), dim3(TPB), 0, s, n, (const uint32_t*)w.ord, (const uint32_t*)w.sval[0],
                       (const uint32_t*)w.pb, (uint32_t*)nullptr, w.sb);
    hipLaunchKernelGGL(adj_head_count_kernel, dim3(nbn), dim3(TPB), 0, s, n, (const uint32_t*)w.skey[0], (const uint32_t*)w.sb, w.bsum);
    hipLaunchKernelGGL(adj_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, w.bsum, (int)nbn, w.totals + T_PAIRS);
    hipLaunchKernelGGL(adj_emit_kernel, dim3(nbn), dim3(TPB), 0, s, n, (const uint32_t*)w.skey[0], (const uint32_t*)w.sb, (const uint32_t*)w.bsum,
                       w.nbr_idx, w.dfirst, w.pinned, w.totals);
  }
  hipLaunchKernelGGL(adj_offsets_kernel, dim3(blocks_of((int64_t)V + 1)), dim3(TPB), 0, s, V, n, (const int32_t*)w.dfirst,
                     (const int64_t*)w.totals, w.nbr_off);
  if (V > 0)
    hipLaunchKernelGGL(adj_class_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, (const int32_t*)w.nbr_off, (const uint8_t*)w.pinned, w.totals);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_smooth(int32_t V, int64_t F, const float* vertices, void* workspace, int32_t iterations, double lambda, double mu,
                                int32_t pin_boundary, float* out_vertices, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_smooth";
  if (int rc = check_common(what, V, F, workspace)) return rc;
  if (iterations < 0 || iterations > (1 << 20)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= iterations <= 2^20");
  if (!(lambda > 0.0 && lambda <= 1.0)) return b3gs_fail(B3GS_ERR_ARG, what, "0 < lambda <= 1");
  if (!(mu <= 0.0) || (mu != 0.0 && !(mu < -lambda)) || !(mu >= -DBL_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "mu = 0, or mu < -lambda and finite");
  if (V > 0 && (!vertices || !out_vertices)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  AdjWs w;
  adj_carve(static_cast<char*>(workspace), V, F, &w);
  hipStream_t s = (hipStream_t)stream;
  count_nonfinite(V, vertices, w, s);
  if (V == 0) return b3gs_launch_status(what);
  const unsigned nbv = blocks_of(V);
  const int32_t n = (int32_t)(6 * F);
  hipLaunchKernelGGL(smooth_pack_kernel, dim3(nbv), dim3(TPB), 0, s, V, vertices, w.pos[0]);
  int cur = 0;
  for (int32_t r = 0; r < iterations; r++)
    for (int half = 0; half < 2; half++) {
      if (half == 1 && mu == 0.0) continue;                          // a plain Laplacian filter
      hipLaunchKernelGGL(smooth_step_kernel, dim3(nbv), dim3(TPB), 0, s, V, n, (const float4*)w.pos[cur], w.pos[cur ^ 1],
                         (const int32_t*)w.nbr_off, (const int32_t*)w.nbr_idx, (const uint8_t*)w.pinned, half ? mu : lambda,
                         (int32_t)(pin_boundary != 0));
      cur ^= 1;
    }
  hipLaunchKernelGGL(smooth_unpack_kernel, dim3(nbv), dim3(TPB), 0, s, V, (const float4*)w.pos[cur], out_vertices);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_vertex_normals(int32_t V, int64_t F, const float* vertices, const int32_t* faces, void* workspace, float* normals,
                                        b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_vertex_normals";
  if (int rc = check_common(what, V, F, workspace)) return rc;
  if ((V > 0 && (!vertices || !normals)) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  AdjWs w;
  adj_carve(static_cast<char*>(workspace), V, F, &w);
  hipStream_t s = (hipStream_t)stream;
  count_nonfinite(V, vertices, w, s);
  if (V > 0)
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_of(V)), dim3(TPB), 0, s, V, F, vertices, faces, (const uint2*)w.inc,
                       (const int32_t*)w.inc_face, normals);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_resolve_shaded_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                              const float* normals, const int32_t* faces, const void* workspace, const float* bg, int32_t mode,
                                              int32_t* triangle_id, float* depth, float* alpha, float* colour, int32_t* face_pixels,
                                              b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_resolve_shaded_batch";
  Layout l;
  if (!layout(nviews, V, F, W, H, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views, 1 <= W, H <= 16384, 0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (mode != B3GS_MESH_SHADE_SMOOTH && mode != B3GS_MESH_SHADE_LIT) return b3gs_fail(B3GS_ERR_ARG, what, "unknown mode");
  if (!cameras || (V > 0 && !normals) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  const char* ws = static_cast<const char*>(workspace);
  ShadedArgs a = {};
  a.n = nviews, a.W = W, a.H = H, a.V = V, a.F = F, a.mode = mode;
  a.normals = normals, a.faces = faces, a.bg = bg;
  a.sv = reinterpret_cast<const SVert*>(ws + l.sv);
  a.vis = reinterpret_cast<const unsigned long long*>(ws + l.vis);
  a.triangle_id = triangle_id, a.depth = depth, a.alpha = alpha, a.colour = colour, a.face_pixels = face_pixels;
  load_cams(nviews, cameras, a.cam);
  hipLaunchKernelGGL(shaded_resolve_kernel, dim3(blocks_of((int64_t)W * H), (unsigned)nviews), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}
