// What the mesh rasterizer (meshraster.hip) and the texture calls (texture.hip) share: a view's camera, a vertex on the screen,
// a triangle's edge functions and depth, and the layout of the workspace b3gs_mesh_raster_batch fills.  include/b3gs_raster.h,
// section "rendering an extracted mesh", states the arithmetic; every function here is one of its statements.
#pragma once
#include "b3gs_internal.h"

namespace {

constexpr int MESH_TPB = 256;
constexpr int NV = B3GS_MAX_MESH_VIEWS;

struct Cam {
  float rot[9], trans[3], fx, fy;
};
struct SVert {                                  // one (view, vertex): 16 bytes
  int32_t X, Y;                                 // screen position in 1/256 pixel
  float pz;                                     // camera-space z
  int32_t ok;                                   // 0: the vertex rejects every triangle that names it
};

// ---- one triangle on the screen ----------------------------------------------------------------------------------------
// E_k(i, j) = e0[k] + ex[k] i + ey[k] j is the edge function opposite vertex k at the centre of pixel (i, j), oriented so
// that the doubled area A is positive; the pixel is inside when every E_k >= bias[k] (0 on a top or left edge, 1 elsewhere).
struct Tri {
  int64_t A, e0[3], ex[3], ey[3];
  int32_t bias[3];
  float iz[3];
  int32_t x0, y0, x1, y1;                       // clamped box, inclusive; empty when x1 < x0 or y1 < y0
  uint32_t id;
};

__device__ __forceinline__ bool face_ok(const int32_t* f, int32_t V) {
  return (uint32_t)f[0] < (uint32_t)V && (uint32_t)f[1] < (uint32_t)V && (uint32_t)f[2] < (uint32_t)V;
}

// -> 0: the triangle covers nothing (zero area, culled, box outside the image); 1: t is filled.  winding: the sign of the
// doubled area as given (+1: clockwise as seen, the normal points away).
__device__ __forceinline__ int tri_setup(const SVert& a, const SVert& b, const SVert& c, int32_t W, int32_t H, int cull, Tri* t,
                                         int* winding) {
  const int64_t X[3] = {a.X, b.X, c.X}, Y[3] = {a.Y, b.Y, c.Y};
  const int64_t area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
  *winding = area > 0 ? 1 : (area < 0 ? -1 : 0);
  if (area == 0 || (cull && area > 0)) return 0;
  const int64_t s = area > 0 ? 1 : -1;
  t->A = s * area;
#pragma unroll
  for (int k = 0; k < 3; k++) {                 // the edge from vertex k + 1 to vertex k + 2
    const int p = k == 2 ? 0 : k + 1, q = p == 2 ? 0 : p + 1;
    const int64_t dx = s * (X[q] - X[p]), dy = s * (Y[q] - Y[p]);
    t->e0[k] = dy * X[p] - dx * Y[p];
    t->ex[k] = -256 * dy;
    t->ey[k] = 256 * dx;
    t->bias[k] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
  }
  const int64_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
  const int64_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
  t->x0 = (int32_t)max((xmin + 255) >> 8, (int64_t)0), t->x1 = (int32_t)min(xmax >> 8, (int64_t)W - 1);
  t->y0 = (int32_t)max((ymin + 255) >> 8, (int64_t)0), t->y1 = (int32_t)min(ymax >> 8, (int64_t)H - 1);
  t->iz[0] = __fdiv_rn(1.0f, a.pz), t->iz[1] = __fdiv_rn(1.0f, b.pz), t->iz[2] = __fdiv_rn(1.0f, c.pz);
  return t->x1 >= t->x0 && t->y1 >= t->y0;
}

__device__ __forceinline__ bool tri_edges(const Tri& t, int32_t i, int32_t j, int64_t* E) {
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    E[k] = t.e0[k] + t.ex[k] * i + t.ey[k] * j;
    in = in && E[k] >= t.bias[k];
  }
  return in;
}
// the barycentric weights and the perspective-correct z of a covered pixel
__device__ __forceinline__ float tri_depth(const Tri& t, const int64_t* E, float* w) {
  const double A = (double)t.A;
#pragma unroll
  for (int k = 0; k < 3; k++) w[k] = __fmul_rn((float)((double)E[k] / A), t.iz[k]);
  const float iz = __fadd_rn(__fadd_rn(w[0], w[1]), w[2]);
  return __fdiv_rn(1.0f, iz);
}
// ---- the workspace of b3gs_mesh_raster_batch, which both resolves read ------------------------------------------------------
struct Layout {
  int32_t nbf;
  size_t sv, vis, cls, bsum, list, total;
};
static bool layout(int32_t n, int64_t V, int64_t F, int32_t W, int32_t H, Layout* l) {
  if (n < 1 || n > NV || V < 0 || F < 0 || V > INT32_MAX || F > INT32_MAX || W < 1 || H < 1 || W > B3GS_MAX_MESH_IMAGE || H > B3GS_MAX_MESH_IMAGE)
    return false;
  const size_t v = (size_t)(V ? V : 1), f = (size_t)(F ? F : 1);
  l->nbf = (int32_t)((F + MESH_TPB - 1) / MESH_TPB);                   // the triangle blocks of setup_kernel
  size_t at = 256;                                                // the list lengths
  l->sv = at, at += b3gs_align256((size_t)n * v * sizeof(SVert));
  l->vis = at, at += b3gs_align256((size_t)n * W * H * sizeof(unsigned long long));
  l->cls = at, at += b3gs_align256((size_t)n * f);
  l->bsum = at, at += b3gs_align256((size_t)n * 2 * (l->nbf ? l->nbf : 1) * sizeof(uint32_t));
  l->list = at, at += b3gs_align256((size_t)n * 2 * f * sizeof(uint32_t));
  l->total = at;
  return true;
}
static void load_cams(int32_t n, const float* cameras, Cam* cam) {
  for (int v = 0; v < n; v++) {
    const float* row = cameras + 14 * v;
    for (int q = 0; q < 9; q++) cam[v].rot[q] = row[q];
    for (int q = 0; q < 3; q++) cam[v].trans[q] = row[9 + q];
    cam[v].fx = row[12], cam[v].fy = row[13];
  }
}
static bool aligned256(const void* p) { return p && !((uintptr_t)p & 255); }

}  // namespace
