// Texturing an extracted mesh (entry points added to ABI 18; binocular3dgs_amd/mesh_texture.py).
// include/b3gs_raster.h states the arithmetic; tests/texture_ref.py restates it.  Every triangle owns a right-angled patch of
// the atlas (texture_layout.h); a texel is a point of its triangle's plane.
//   accumulate  thread = texel: the point, the views that see it (the rasterizer's resolved triangle id and depth at the
//               nearest pixel), the images sampled bilinearly, summed in view order into the texel's own four floats
//   finalize    thread = texel: the weighted mean as uint8, or the interpolated vertex colours where no view saw the texel
//   resolve     thread = (view, pixel): the rasterizer's resolve with the colour fetched from the atlas
// No float atomics and no sum across threads: one fixed output whatever the launch geometry.  Nothing reads the device.
#include "b3gs_internal.h"
#include "mesh_tri.h"
#include "texture_layout.h"
#include <cfloat>
#include <cstdio>

namespace {

constexpr int TPB = MESH_TPB;
static_assert(B3GS_TEX_MIN_CELL == B3GS_TEXTURE_MIN_CELL && B3GS_TEX_MAX_CELL == B3GS_TEXTURE_MAX_CELL && B3GS_TEX_MAX_SIDE == B3GS_MAX_ATLAS_SIDE,
              "texture_layout.h restates the limits of include/b3gs_raster.h");

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

__device__ __forceinline__ float sqrt_rn(float x) { return sqrtf(x); }   // (correctly rounded: see meshtools.hip)
__device__ __forceinline__ float dot3(const float* a, const float* b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(a[0], b[0]), __fmul_rn(a[1], b[1])), __fmul_rn(a[2], b[2]));
}
// statement 2: the barycentrics of the texel with the local indices (i, j)
__device__ __forceinline__ void texel_bary(int32_t n, int32_t i, int32_t j, float* b) {
  const float leg = (float)(n - 2);
  b[1] = __fdiv_rn((float)i, leg), b[2] = __fdiv_rn((float)j, leg);
  b[0] = __fsub_rn(__fsub_rn(1.0f, b[1]), b[2]);
}
// statement 7: the four neighbours of (x, y), 0 <= x <= w - 1, 0 <= y <= h - 1, of a plane of w x h values
struct Bilinear {
  int64_t o00, o01, o10, o11;
  float fx, fy, gx, gy;
};
__device__ __forceinline__ Bilinear bilinear_at(float x, float y, int32_t w, int32_t h) {
  const float xf = floorf(x), yf = floorf(y);
  const int32_t x0 = (int32_t)xf, y0 = (int32_t)yf, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
  Bilinear s;
  s.fx = __fsub_rn(x, xf), s.fy = __fsub_rn(y, yf), s.gx = __fsub_rn(1.0f, s.fx), s.gy = __fsub_rn(1.0f, s.fy);
  s.o00 = (int64_t)y0 * w + x0, s.o01 = (int64_t)y0 * w + x1, s.o10 = (int64_t)y1 * w + x0, s.o11 = (int64_t)y1 * w + x1;
  return s;
}
__device__ __forceinline__ float bilinear_mix(const Bilinear& s, float v00, float v01, float v10, float v11) {
  const float top = __fadd_rn(__fmul_rn(s.gx, v00), __fmul_rn(s.fx, v01)), bot = __fadd_rn(__fmul_rn(s.gx, v10), __fmul_rn(s.fx, v11));
  return __fadd_rn(__fmul_rn(s.gy, top), __fmul_rn(s.fy, bot));
}
// statement 8: a value in 0 .. 1 -> uint8 (NaN -> 0)
__device__ __forceinline__ uint8_t to_byte(float r) { return (uint8_t)rintf(__fmul_rn(255.0f, fminf(fmaxf(r, 0.0f), 1.0f))); }

struct AccumArgs {
  TexAtlas atlas;
  int32_t n, W, H, V, two_sided;
  float slack;
  const float* vertices;
  const int32_t* faces;
  const int32_t* triangle_id;                   // [n][H][W]
  const float* depth;                           // [n][1][H][W]
  const float* images;                          // [n][3][H][W]
  float4* accum;                                // [Ht][Wt]
  int32_t* bad;                                 // [1]
  Cam cam[NV];
  float centre[NV][3];
};

__global__ void __launch_bounds__(TPB) texture_accumulate_kernel(AccumArgs a) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (t >= (int64_t)a.atlas.Wt * a.atlas.Ht) return;
  int32_t li, lj;
  const int64_t f = tex_owner(a.atlas, (int32_t)(t % a.atlas.Wt), (int32_t)(t / a.atlas.Wt), &li, &lj);
  if (f < 0) return;
  const int32_t idx[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
  if (!face_ok(idx, a.V)) {
    if (li == 0 && lj == 0) atomicAdd(a.bad, 1);                  // the texel of corner 0: once per triangle
    return;
  }
  float b[3], vx[3][3], q[3], e1[3], e2[3], nrm[3];
  texel_bary(a.atlas.n, li, lj, b);
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int r = 0; r < 3; r++) vx[k][r] = a.vertices[3 * (size_t)idx[k] + r];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    q[r] = __fadd_rn(__fadd_rn(__fmul_rn(b[0], vx[0][r]), __fmul_rn(b[1], vx[1][r])), __fmul_rn(b[2], vx[2][r]));
    e1[r] = __fsub_rn(vx[1][r], vx[0][r]), e2[r] = __fsub_rn(vx[2][r], vx[0][r]);
  }
  nrm[0] = __fsub_rn(__fmul_rn(e1[1], e2[2]), __fmul_rn(e1[2], e2[1]));
  nrm[1] = __fsub_rn(__fmul_rn(e1[2], e2[0]), __fmul_rn(e1[0], e2[2]));
  nrm[2] = __fsub_rn(__fmul_rn(e1[0], e2[1]), __fmul_rn(e1[1], e2[0]));
  const float len = sqrt_rn(dot3(nrm, nrm));
  if (!(len > 0.0f && len <= FLT_MAX)) return;                    // no area, or a vertex that is not finite: weight 0
#pragma unroll
  for (int r = 0; r < 3; r++) nrm[r] = __fdiv_rn(nrm[r], len);
  const float cx = __fsub_rn(__fmul_rn(0.5f, (float)a.W), 0.5f), cy = __fsub_rn(__fmul_rn(0.5f, (float)a.H), 0.5f);
  const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
  const int64_t plane = (int64_t)a.W * a.H;
  float4 acc = a.accum[t];
  for (int v = 0; v < a.n; v++) {
    const Cam& c = a.cam[v];
    float p[3];
#pragma unroll
    for (int r = 0; r < 3; r++)
      p[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.rot[3 * r], q[0]), __fmul_rn(c.rot[3 * r + 1], q[1])), __fmul_rn(c.rot[3 * r + 2], q[2])), c.trans[r]);
    const float sx = __fadd_rn(__fmul_rn(c.fx, __fdiv_rn(p[0], p[2])), cx), sy = __fadd_rn(__fmul_rn(c.fy, __fdiv_rn(p[1], p[2])), cy);
    if (!(p[2] > B3GS_NEAR && p[2] <= FLT_MAX && sx >= 0.0f && sx <= xmax && sy >= 0.0f && sy <= ymax)) continue;    // (NaN: skipped)
    const int64_t pix = (int64_t)rintf(sy) * a.W + (int64_t)rintf(sx);
    const int32_t tid = a.triangle_id[v * plane + pix];
    if (!(tid < 0 || tid == f || p[2] <= __fadd_rn(a.depth[v * plane + pix], a.slack))) continue;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; r++) d[r] = __fsub_rn(a.centre[v][r], q[r]);
    const float dl = sqrt_rn(dot3(d, d));
    if (!(dl > 0.0f && dl <= FLT_MAX)) continue;
    float cosine = __fdiv_rn(dot3(nrm, d), dl);
    if (a.two_sided) cosine = fabsf(cosine);
    if (!(cosine > 0.0f)) continue;
    const float w = __fmul_rn(cosine, cosine);
    const Bilinear s = bilinear_at(sx, sy, a.W, a.H);
    const float* img = a.images + (size_t)v * 3 * plane;
    float col[3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float* pl = img + ch * plane;
      col[ch] = bilinear_mix(s, pl[s.o00], pl[s.o01], pl[s.o10], pl[s.o11]);
    }
    acc.x = __fadd_rn(acc.x, __fmul_rn(w, col[0])), acc.y = __fadd_rn(acc.y, __fmul_rn(w, col[1]));
    acc.z = __fadd_rn(acc.z, __fmul_rn(w, col[2])), acc.w = __fadd_rn(acc.w, w);
  }
  a.accum[t] = acc;
}

struct FinalArgs {
  TexAtlas atlas;
  int32_t V;
  const uint8_t* colours;
  const int32_t* faces;
  const float4* accum;
  uint8_t* texture;                             // [Ht][Wt][3]
  int32_t* coverage;                            // [2]
};

__global__ void __launch_bounds__(TPB) texture_finalize_kernel(FinalArgs a) {
  const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const bool live = t < (int64_t)a.atlas.Wt * a.atlas.Ht;
  int32_t li = 0, lj = 0, seen = 0;
  const int64_t f = live ? tex_owner(a.atlas, (int32_t)(t % a.atlas.Wt), (int32_t)(t / a.atlas.Wt), &li, &lj) : -1;
  uint8_t out[3] = {0, 0, 0};
  if (f >= 0) {
    const float4 acc = a.accum[t];
    if (acc.w > 0.0f) {
      seen = 1;
      out[0] = to_byte(__fdiv_rn(acc.x, acc.w)), out[1] = to_byte(__fdiv_rn(acc.y, acc.w)), out[2] = to_byte(__fdiv_rn(acc.z, acc.w));
    } else if (a.colours) {
      const int32_t idx[3] = {a.faces[3 * f], a.faces[3 * f + 1], a.faces[3 * f + 2]};
      if (face_ok(idx, a.V)) {
        float b[3];
        texel_bary(a.atlas.n, li, lj, b);
#pragma unroll
        for (int k = 0; k < 3; k++) b[k] = fmaxf(b[k], 0.0f);
        const float sum = __fadd_rn(__fadd_rn(b[0], b[1]), b[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) b[k] = __fdiv_rn(b[k], sum);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
          const float c0 = (float)a.colours[3 * (size_t)idx[0] + ch], c1 = (float)a.colours[3 * (size_t)idx[1] + ch],
                      c2 = (float)a.colours[3 * (size_t)idx[2] + ch];
          out[ch] = to_byte(__fdiv_rn(__fadd_rn(__fadd_rn(__fmul_rn(b[0], c0), __fmul_rn(b[1], c1)), __fmul_rn(b[2], c2)), 255.0f));
        }
      }
    }
  }
  if (live)
    for (int ch = 0; ch < 3; ch++) a.texture[3 * t + ch] = out[ch];
  const int nseen = b3gs_wave_sum(seen), nowned = b3gs_wave_sum(f >= 0 ? 1 : 0);      // every lane of the wave is here
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0 && nowned) {
    if (nseen) atomicAdd(a.coverage, nseen);
    atomicAdd(a.coverage + 1, nowned);
  }
}

struct TexResolveArgs {
  TexAtlas atlas;
  int32_t n, W, H, V;
  int64_t F;
  const int32_t* faces;
  const SVert* sv;
  const unsigned long long* vis;
  const float* bg;
  const uint8_t* texture;
  int32_t* triangle_id;
  float* depth;
  float* alpha;
  float* colour;
  int32_t* face_pixels;
};

// resolve_kernel of meshraster.hip with the colour taken from the atlas
__global__ void __launch_bounds__(TPB) texture_resolve_kernel(TexResolveArgs a) {
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
        float cu[3], cv[3];
        tex_corners(a.atlas, id, cu, cv);
        float u = __fmul_rn(dot3(w, cu), z), v = __fmul_rn(dot3(w, cv), z);
        u = fminf(fmaxf(u, 0.0f), (float)(a.atlas.Wt - 1)), v = fminf(fmaxf(v, 0.0f), (float)(a.atlas.Ht - 1));      // (NaN -> 0)
        const Bilinear s = bilinear_at(u, v, a.atlas.Wt, a.atlas.Ht);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
          col[ch] = __fdiv_rn(bilinear_mix(s, (float)a.texture[3 * s.o00 + ch], (float)a.texture[3 * s.o01 + ch],
                                           (float)a.texture[3 * s.o10 + ch], (float)a.texture[3 * s.o11 + ch]), 255.0f);
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

// -> NULL when (F, cell, Wt, Ht) is an atlas, else what is wrong with it
static const char* atlas_of(int64_t F, int32_t cell, int32_t Wt, int32_t Ht, TexAtlas* a) {
  static thread_local char msg[160];
  const int32_t want = tex_atlas_height(F, cell, Wt);
  if (!want) {
    snprintf(msg, sizeof msg, "no atlas: 1 <= F <= 2^31 - 1, 4 <= cell <= 256, cell + 1 <= Wt and Wt, Ht <= 16384; the largest cell that fits this width is %d",
             (int)tex_largest_cell(F, Wt));
    return msg;
  }
  if (want != Ht) return "Ht is not the height of this atlas (b3gs_mesh_texture_atlas_height)";
  a->n = cell, a->Wt = Wt, a->Ht = Ht, a->cpr = Wt / (cell + 1), a->F = F;
  return nullptr;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int32_t b3gs_mesh_texture_atlas_height(int64_t F, int32_t cell, int32_t Wt) { return tex_atlas_height(F, cell, Wt); }

extern "C" int b3gs_mesh_texture_accumulate_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                                  const float* vertices, const int32_t* faces, int32_t cell, int32_t Wt, int32_t Ht,
                                                  const int32_t* triangle_id, const float* depth, const float* images, float slack,
                                                  int32_t two_sided, float* accum, int32_t* bad_faces, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_texture_accumulate_batch";
  Layout l;
  if (!layout(nviews, V, F, W, H, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views, 1 <= W, H <= 16384, 0 <= V, F <= 2^31 - 1");
  AccumArgs a = {};
  if (const char* bad = atlas_of(F, cell, Wt, Ht, &a.atlas)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  if (!(slack >= 0.0f && slack <= FLT_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "slack >= 0 and finite");
  if (!cameras || !triangle_id || !depth || !images || !accum || !bad_faces || (V > 0 && !vertices) || !faces)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if ((uintptr_t)accum & 15) return b3gs_fail(B3GS_ERR_ARG, what, "accum is 16-byte aligned");
  a.n = nviews, a.W = W, a.H = H, a.V = V, a.two_sided = two_sided != 0, a.slack = slack;
  a.vertices = vertices, a.faces = faces, a.triangle_id = triangle_id, a.depth = depth, a.images = images;
  a.accum = reinterpret_cast<float4*>(accum), a.bad = bad_faces;
  load_cams(nviews, cameras, a.cam);
  for (int v = 0; v < nviews; v++) {                              // statement 5: the camera centre - R^T t
    const Cam& c = a.cam[v];
    for (int r = 0; r < 3; r++) a.centre[v][r] = -((c.rot[r] * c.trans[0] + c.rot[3 + r] * c.trans[1]) + c.rot[6 + r] * c.trans[2]);
  }
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(bad_faces, 0, sizeof(int32_t), s);
  hipLaunchKernelGGL(texture_accumulate_kernel, dim3(blocks_of((int64_t)Wt * Ht)), dim3(TPB), 0, s, a);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_texture_finalize(int32_t V, int64_t F, const uint8_t* colours, const int32_t* faces, int32_t cell, int32_t Wt,
                                          int32_t Ht, const float* accum, uint8_t* texture, int32_t* coverage, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_texture_finalize";
  FinalArgs a = {};
  if (V < 0) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= V <= 2^31 - 1");
  if (const char* bad = atlas_of(F, cell, Wt, Ht, &a.atlas)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  if (!faces || !accum || !texture || !coverage) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if ((uintptr_t)accum & 15) return b3gs_fail(B3GS_ERR_ARG, what, "accum is 16-byte aligned");
  a.V = V, a.colours = colours, a.faces = faces, a.accum = reinterpret_cast<const float4*>(accum), a.texture = texture, a.coverage = coverage;
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(coverage, 0, 2 * sizeof(int32_t), s);
  hipLaunchKernelGGL(texture_finalize_kernel, dim3(blocks_of((int64_t)Wt * Ht)), dim3(TPB), 0, s, a);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_resolve_textured_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                                const float* vertices, const int32_t* faces, const void* workspace, const float* bg,
                                                const uint8_t* texture, int32_t cell, int32_t Wt, int32_t Ht, int32_t* triangle_id,
                                                float* depth, float* alpha, float* colour, int32_t* face_pixels, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_resolve_textured_batch";
  Layout l;
  if (!layout(nviews, V, F, W, H, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views, 1 <= W, H <= 16384, 0 <= V, F <= 2^31 - 1");
  if (!aligned256(workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  TexResolveArgs a = {};
  if (const char* bad = atlas_of(F, cell, Wt, Ht, &a.atlas)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  if (!cameras || (V > 0 && !vertices) || !faces || !texture) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  const char* ws = static_cast<const char*>(workspace);
  a.n = nviews, a.W = W, a.H = H, a.V = V, a.F = F, a.faces = faces, a.bg = bg, a.texture = texture;
  a.sv = reinterpret_cast<const SVert*>(ws + l.sv);
  a.vis = reinterpret_cast<const unsigned long long*>(ws + l.vis);
  a.triangle_id = triangle_id, a.depth = depth, a.alpha = alpha, a.colour = colour, a.face_pixels = face_pixels;
  hipLaunchKernelGGL(texture_resolve_kernel, dim3(blocks_of((int64_t)W * H), (unsigned)nviews), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}
