// Rendering an extracted mesh (entry points added to ABI 18; binocular3dgs_amd/mesh_render.py).
// include/b3gs_raster.h states the arithmetic; tests/meshraster_ref.py restates it.  Membership of a pixel in a triangle is
// 64-bit integer work, depth is single correctly rounded operations, and the visibility buffer is a minimum over a set of
// packed (depth bits, triangle index) words: one fixed output whatever the schedule and whichever path took a triangle.
//   transform   thread = (view, vertex): camera-space z and the snapped screen position, once, into the workspace
//   setup       thread = (view, triangle): reject / cull / clamped box -> the triangle's path.  A box of at most small_box
//               pixels is walked by the lane at once; a larger one is flagged, and the block sums of the two flags are left for
//               the ordered scan (b3gs_internal.h)
//   scan, emit  the flagged triangles of a view, in triangle order, into the wave list and the workgroup list
//   wave        one wave per entry of the wave list: the box in 8 x 8 pixel blocks, lane = pixel, a block is skipped when an
//               edge function is negative at the corner of the block where it is largest
//   group       one workgroup per entry of the workgroup list: its waves share the 8 x 8 blocks of the box
//   resolve     thread = (view, pixel): the winner decoded, its barycentrics recomputed from the same integers
// The last two walk their lists with a fixed grid (the list lengths are device words): nothing reads the device.
#include "b3gs_internal.h"
#include "mesh_tri.h"
#include <cfloat>

namespace {

constexpr int TPB = MESH_TPB;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int GROUP_TPB = 1024;                 // the workgroup path: 16 waves per triangle
constexpr int32_t GUARD = 1 << 22;              // |X|, |Y| of a snapped vertex stay below this
constexpr int WAVE_GRID = 2048, GROUP_GRID = 256;

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

struct RasterArgs {
  int32_t n, W, H, V;
  int64_t F;
  int32_t nbf, cull, small_box, wave_box;
  const float* vertices;
  const int32_t* faces;
  SVert* sv;                                    // [n][V]
  unsigned long long* vis;                      // [n][H * W]
  uint8_t* cls;                                 // [n][F] 0: done or nothing to do, 1: wave list, 2: workgroup list
  uint32_t* bsum;                               // [n][2][nbf]
  int32_t* totals;                              // [n][2] entries of the two lists
  uint32_t* list;                               // [n][2][F]
  int32_t* counts;                              // [9]
  Cam cam[NV];
};

// Pixel (i, j) of the view whose buffer is `vis`: the packed minimum.  The word only ever decreases, so a plain read that
// already shows a smaller one settles the matter without the atomic.
__device__ __forceinline__ void tri_pixel(const Tri& t, int32_t i, int32_t j, int32_t W, unsigned long long* vis) {
  int64_t E[3];
  if (!tri_edges(t, i, j, E)) return;
  float w[3];
  const float z = tri_depth(t, E, w);
  const unsigned long long word = ((unsigned long long)__float_as_uint(z) << 32) | t.id;
  unsigned long long* p = vis + (size_t)j * W + i;
  if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= word) return;
  atomicMin(p, word);
}
// The 8 x 8 pixel blocks first, first + step, .. of the box, lane = pixel of the block.
__device__ __forceinline__ void tri_blocks(const Tri& t, int32_t first, int32_t step, int lane, int32_t W, unsigned long long* vis) {
  const int32_t nbx = (t.x1 - t.x0) / 8 + 1, nby = (t.y1 - t.y0) / 8 + 1;
  const int64_t nblk = (int64_t)nbx * nby;
  for (int64_t b = first; b < nblk; b += step) {
    const int32_t bx = t.x0 + 8 * (int32_t)(b % nbx), by = t.y0 + 8 * (int32_t)(b / nbx);
    bool out = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {               // the largest value of E_k over the block, at one of its corners
      const int64_t top = t.e0[k] + t.ex[k] * bx + t.ey[k] * by + max(t.ex[k] * 7, (int64_t)0) + max(t.ey[k] * 7, (int64_t)0);
      out = out || top < t.bias[k];
    }
    if (out) continue;
    const int32_t i = bx + (lane & 7), j = by + (lane >> 3);
    if (i <= t.x1 && j <= t.y1) tri_pixel(t, i, j, W, vis);
  }
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) transform_kernel(RasterArgs a) {
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int view = blockIdx.y;
  if (v >= a.V) return;
  const Cam& c = a.cam[view];
  const float x = a.vertices[3 * v], y = a.vertices[3 * v + 1], z = a.vertices[3 * v + 2];
  float p[3];
#pragma unroll
  for (int r = 0; r < 3; r++)
    p[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.rot[3 * r], x), __fmul_rn(c.rot[3 * r + 1], y)), __fmul_rn(c.rot[3 * r + 2], z)), c.trans[r]);
  const float cx = __fsub_rn(__fmul_rn(0.5f, (float)a.W), 0.5f), cy = __fsub_rn(__fmul_rn(0.5f, (float)a.H), 0.5f);
  const float sx = __fadd_rn(__fmul_rn(c.fx, __fdiv_rn(p[0], p[2])), cx), sy = __fadd_rn(__fmul_rn(c.fy, __fdiv_rn(p[1], p[2])), cy);
  const float rx = rintf(__fmul_rn(sx, 256.0f)), ry = rintf(__fmul_rn(sy, 256.0f));
  SVert s;
  s.ok = p[2] > B3GS_NEAR && p[2] <= FLT_MAX && fabsf(rx) < (float)GUARD && fabsf(ry) < (float)GUARD;      // (NaN: rejected)
  s.X = s.ok ? (int32_t)rx : 0, s.Y = s.ok ? (int32_t)ry : 0;
  s.pz = p[2];
  a.sv[(size_t)view * a.V + v] = s;
}

__global__ void __launch_bounds__(TPB) setup_kernel(RasterArgs a) {
  __shared__ int wave_n[2][TPB / B3GS_WAVE];
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int view = blockIdx.y;
  int cls = 0;
  if (f < a.F) {
    const int32_t idx[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
    bool rejected = true;
    if (!face_ok(idx, a.V)) {
      if (view == 0) atomicAdd(a.counts + NV, 1);
    } else {
      const SVert* sv = a.sv + (size_t)view * a.V;
      const SVert s0 = sv[idx[0]], s1 = sv[idx[1]], s2 = sv[idx[2]];
      rejected = !(s0.ok && s1.ok && s2.ok);
      Tri t;
      int winding;
      if (!rejected && tri_setup(s0, s1, s2, a.W, a.H, a.cull, &t, &winding)) {
        t.id = (uint32_t)f;
        const int64_t box = (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1);
        if (box <= a.small_box) {
          unsigned long long* vis = a.vis + (size_t)view * a.W * a.H;
          for (int32_t j = t.y0; j <= t.y1; j++)
            for (int32_t i = t.x0; i <= t.x1; i++) tri_pixel(t, i, j, a.W, vis);
        } else {
          cls = box <= a.wave_box ? 1 : 2;
        }
      }
    }
    if (rejected) atomicAdd(a.counts + view, 1);
    a.cls[(size_t)view * a.F + f] = (uint8_t)cls;
  }
  int total[2];
  b3gs_block_rank<TPB, 1>(cls == 1, wave_n[0], &total[0]);
  b3gs_block_rank<TPB, 1>(cls == 2, wave_n[1], &total[1]);
  if (threadIdx.x < 2) a.bsum[((size_t)view * 2 + threadIdx.x) * a.nbf + blockIdx.x] = (uint32_t)total[threadIdx.x];
}

// block (list, view)
__global__ void __launch_bounds__(SCAN_TPB) scan_kernel(RasterArgs a) {
  const size_t k = (size_t)blockIdx.y * 2 + blockIdx.x;
  b3gs_scan_block_sums(a.bsum + k * a.nbf, a.nbf, a.totals + k);
}

__global__ void __launch_bounds__(TPB) emit_kernel(RasterArgs a) {
  __shared__ int wave_n[2][TPB / B3GS_WAVE];
  const int64_t f = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int view = blockIdx.y;
  const int cls = f < a.F ? a.cls[(size_t)view * a.F + f] : 0;
  int total, rank[2];
  rank[0] = b3gs_block_rank<TPB, 1>(cls == 1, wave_n[0], &total);
  rank[1] = b3gs_block_rank<TPB, 1>(cls == 2, wave_n[1], &total);
  if (!cls) return;
  const size_t k = (size_t)view * 2 + (cls - 1);
  const int64_t at = (int64_t)a.bsum[k * a.nbf + blockIdx.x] + rank[cls - 1];
  if (at < a.F) a.list[k * a.F + at] = (uint32_t)f;
}

// entry e of list `which` of the view -> the triangle, set up again from the workspace (the flags of setup_kernel say that
// it is there and covers something)
__device__ __forceinline__ bool list_tri(const RasterArgs& a, int view, int which, int64_t e, Tri* t) {
  const uint32_t f = a.list[((size_t)view * 2 + which) * a.F + e];
  if (f >= (uint64_t)a.F) return false;
  const int32_t idx[3] = {a.faces[3 * (size_t)f], a.faces[3 * (size_t)f + 1], a.faces[3 * (size_t)f + 2]};
  if (!face_ok(idx, a.V)) return false;
  const SVert* sv = a.sv + (size_t)view * a.V;
  const SVert s0 = sv[idx[0]], s1 = sv[idx[1]], s2 = sv[idx[2]];
  int winding;
  if (!(s0.ok && s1.ok && s2.ok) || !tri_setup(s0, s1, s2, a.W, a.H, a.cull, t, &winding)) return false;
  t->id = f;
  return true;
}

__global__ void __launch_bounds__(TPB) wave_kernel(RasterArgs a) {
  const int view = blockIdx.y, lane = threadIdx.x & (B3GS_WAVE - 1);
  const int64_t count = min((int64_t)a.totals[view * 2], a.F);
  const int64_t nwaves = (int64_t)gridDim.x * (TPB / B3GS_WAVE);
  unsigned long long* vis = a.vis + (size_t)view * a.W * a.H;
  for (int64_t e = (int64_t)blockIdx.x * (TPB / B3GS_WAVE) + threadIdx.x / B3GS_WAVE; e < count; e += nwaves) {
    Tri t;
    if (list_tri(a, view, 0, e, &t)) tri_blocks(t, 0, 1, lane, a.W, vis);
  }
}

__global__ void __launch_bounds__(GROUP_TPB) group_kernel(RasterArgs a) {
  const int view = blockIdx.y, lane = threadIdx.x & (B3GS_WAVE - 1);
  const int64_t count = min((int64_t)a.totals[view * 2 + 1], a.F);
  unsigned long long* vis = a.vis + (size_t)view * a.W * a.H;
  for (int64_t e = blockIdx.x; e < count; e += gridDim.x) {
    Tri t;
    if (list_tri(a, view, 1, e, &t)) tri_blocks(t, threadIdx.x / B3GS_WAVE, GROUP_TPB / B3GS_WAVE, lane, a.W, vis);
  }
}

struct ResolveArgs {
  int32_t n, W, H, V;
  int64_t F;
  int32_t shading;
  const float* vertices;
  const uint8_t* colours;
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

__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }   // (correctly rounded: see meshtools.hip)

__global__ void __launch_bounds__(TPB) resolve_kernel(ResolveArgs a) {
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
      if (a.colour && a.shading == B3GS_MESH_SHADE_COLOUR) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const float c0 = (float)a.colours[3 * (size_t)idx[0] + ch], c1 = (float)a.colours[3 * (size_t)idx[1] + ch],
                      c2 = (float)a.colours[3 * (size_t)idx[2] + ch];
          const float s = __fadd_rn(__fadd_rn(__fmul_rn(w[0], c0), __fmul_rn(w[1], c1)), __fmul_rn(w[2], c2));
          col[ch] = __fdiv_rn(__fmul_rn(s, z), 255.0f);
        }
      } else if (a.colour) {
        const Cam& c = a.cam[view];
        float p[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const float* q = a.vertices + 3 * (size_t)idx[k];
#pragma unroll
          for (int r = 0; r < 3; r++)
            p[k][r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.rot[3 * r], q[0]), __fmul_rn(c.rot[3 * r + 1], q[1])), __fmul_rn(c.rot[3 * r + 2], q[2])),
                                c.trans[r]);
        }
        float u[3], v[3], nrm[3];
#pragma unroll
        for (int r = 0; r < 3; r++) u[r] = __fsub_rn(p[1][r], p[0][r]), v[r] = __fsub_rn(p[2][r], p[0][r]);
        nrm[0] = __fsub_rn(__fmul_rn(u[1], v[2]), __fmul_rn(u[2], v[1]));
        nrm[1] = __fsub_rn(__fmul_rn(u[2], v[0]), __fmul_rn(u[0], v[2]));
        nrm[2] = __fsub_rn(__fmul_rn(u[0], v[1]), __fmul_rn(u[1], v[0]));
        const float len = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(nrm[0], nrm[0]), __fmul_rn(nrm[1], nrm[1])), __fmul_rn(nrm[2], nrm[2])));
        const bool unit = len > 0.0f && len <= FLT_MAX;
#pragma unroll
        for (int r = 0; r < 3; r++) {
          float q = unit ? __fdiv_rn(nrm[r], len) : 0.0f;
          if (winding > 0) q = -q;                                // clockwise as seen: the normal points away
          col[r] = __fmul_rn(__fadd_rn(q, 1.0f), 0.5f);
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

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_mesh_raster_workspace_bytes(int32_t nviews, int64_t V, int64_t F, int32_t W, int32_t H) {
  Layout l;
  return layout(nviews, V, F, W, H, &l) ? l.total : 0;
}

extern "C" int b3gs_mesh_raster_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F, const float* vertices,
                                      const int32_t* faces, int32_t cull_backface, int32_t small_box, int32_t wave_box, void* workspace,
                                      int32_t* counts, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_raster_batch";
  Layout l;
  if (!layout(nviews, V, F, W, H, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views, 1 <= W, H <= 16384, 0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (!cameras || !counts || (V > 0 && !vertices) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  char* ws = static_cast<char*>(workspace);
  RasterArgs a = {};
  a.n = nviews, a.W = W, a.H = H, a.V = V, a.F = F, a.nbf = l.nbf, a.cull = cull_backface != 0;
  a.small_box = small_box < 0 ? B3GS_MESH_SMALL_BOX : small_box;
  a.wave_box = wave_box < 0 ? B3GS_MESH_WAVE_BOX : wave_box;
  a.vertices = vertices, a.faces = faces, a.counts = counts;
  a.totals = reinterpret_cast<int32_t*>(ws);
  a.sv = reinterpret_cast<SVert*>(ws + l.sv);
  a.vis = reinterpret_cast<unsigned long long*>(ws + l.vis);
  a.cls = reinterpret_cast<uint8_t*>(ws + l.cls);
  a.bsum = reinterpret_cast<uint32_t*>(ws + l.bsum);
  a.list = reinterpret_cast<uint32_t*>(ws + l.list);
  load_cams(nviews, cameras, a.cam);
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(ws, 0, 256, s);
  (void)hipMemsetAsync(counts, 0, (NV + 1) * sizeof(int32_t), s);
  (void)hipMemsetAsync(a.vis, 0xFF, (size_t)nviews * W * H * sizeof(unsigned long long), s);
  if (V > 0 && F > 0) {
    const unsigned nv = (unsigned)nviews;
    hipLaunchKernelGGL(transform_kernel, dim3(blocks_of(V), nv), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)l.nbf, nv), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(scan_kernel, dim3(2, nv), dim3(SCAN_TPB), 0, s, a);
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)l.nbf, nv), dim3(TPB), 0, s, a);
    const int64_t wave_blocks = (F + TPB / B3GS_WAVE - 1) / (TPB / B3GS_WAVE);
    hipLaunchKernelGGL(wave_kernel, dim3((unsigned)(wave_blocks < WAVE_GRID ? wave_blocks : WAVE_GRID), nv), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(group_kernel, dim3((unsigned)(F < GROUP_GRID ? F : GROUP_GRID), nv), dim3(GROUP_TPB), 0, s, a);
  } else if (F > 0) {                                             // no vertex: every face names none
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)l.nbf, (unsigned)nviews), dim3(TPB), 0, s, a);
  }
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_resolve_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F, const float* vertices,
                                       const uint8_t* colours, const int32_t* faces, const void* workspace, const float* bg, int32_t shading,
                                       int32_t* triangle_id, float* depth, float* alpha, float* colour, int32_t* face_pixels,
                                       b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_resolve_batch";
  Layout l;
  if (!layout(nviews, V, F, W, H, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views, 1 <= W, H <= 16384, 0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (shading != B3GS_MESH_SHADE_COLOUR && shading != B3GS_MESH_SHADE_NORMAL) return b3gs_fail(B3GS_ERR_ARG, what, "unknown shading");
  if (!cameras || (V > 0 && !vertices) || (F > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (colour && shading == B3GS_MESH_SHADE_COLOUR && V > 0 && !colours) return b3gs_fail(B3GS_ERR_ARG, what, "colour shading needs the vertex colours");
  const char* ws = static_cast<const char*>(workspace);
  ResolveArgs a = {};
  a.n = nviews, a.W = W, a.H = H, a.V = V, a.F = F, a.shading = shading;
  a.vertices = vertices, a.colours = colours, a.faces = faces, a.bg = bg;
  a.sv = reinterpret_cast<const SVert*>(ws + l.sv);
  a.vis = reinterpret_cast<const unsigned long long*>(ws + l.vis);
  a.triangle_id = triangle_id, a.depth = depth, a.alpha = alpha, a.colour = colour, a.face_pixels = face_pixels;
  load_cams(nviews, cameras, a.cam);
  hipLaunchKernelGGL(resolve_kernel, dim3(blocks_of((int64_t)W * H), (unsigned)nviews), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}
