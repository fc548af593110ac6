// Normal priors (added to ABI 18; binocular3dgs_amd/normal_prior.py): the normal of the rendered
// depth map by central differences of the back-projected points, its cosine + L1 loss against a target normal plane with the
// gradient in depth AND alpha, the forward alone, and the bilinear resize that brings a prior of any size to the training size.
// include/b3gs_raster.h states every rule; tests/normal_prior_ref.py restates them in numpy float64.
//   forward   grid (image blocks, views), thread = pixel: the four axis neighbours' points, n, validity, the three loss sums
//             through the fixed tree of depthprior.hip, and the UNSCALED tangent adjoints g_tx, g_ty of its own centre as six
//             fp64 planes of the workspace.  The LAST workgroup of a view to arrive folds the block sums with one wave in a fixed
//             order, writes `parts` and 1 / N, and resets the counter (depthprior.hip::last_arrival).
//   gather    thread = pixel: four neighbours' adjoints from the workspace, 1 / N from device memory, its own two words.
//             (why the adjoints are stored and not recomputed from an LDS tile.)
// fp64 throughout, only + - * / sqrt (the Makefile compiles with -ffp-contract=off); no floating-point atomic, no scratch, no
// host read.
#include "b3gs_internal.h"

#include <cmath>

namespace {

constexpr int TPB = 256;
constexpr int NQ = 3;                 // count, 1 - n.t, |n - t|_1
constexpr int HEAD = 32;              // doubles: [0] the arrival counter (its low word), [H_INV] 1 / N
constexpr int H_INV = 8;
constexpr int NADJ = 6;               // g_tx, g_ty

struct Geo {
  int32_t W, H, npix;
  float alpha_min;
  double tfx, tfy;
  const float* depth;
  const float* alpha;
  const uint8_t* mask;
};
struct View {
  Geo g;
  int32_t nb;
  double wc, wl;
  const float* target;
  float* gd;
  float* ga;
  float* normals;
  uint8_t* valid;
  double* parts;
  double* ws;
};
struct Batch {
  int32_t n;
  View v[B3GS_NORMAL_PRIOR_MAX_VIEWS];
};
struct NView {
  Geo g;
  float* normals;
  uint8_t* valid;
};
struct NBatch {
  int32_t n;
  NView v[B3GS_NORMAL_PRIOR_MAX_VIEWS];
};

static inline int nblocks(int64_t n) { return (int)((n + TPB - 1) / TPB); }
__host__ __device__ static inline size_t part_doubles(int nb) { return ((size_t)NQ * nb + 31) / 32 * 32; }
static inline bool aligned256(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }
static inline bool size_ok(int32_t W, int32_t H) { return W >= 1 && H >= 1 && (int64_t)W * H <= (1 << 24); }

__device__ __forceinline__ void st(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
}

__device__ __forceinline__ double ray(int i, int n, double t) { return ((2.0 * ((double)i + 0.5)) / (double)n - 1.0) * t; }
// p of a usable pixel INSIDE the image; false: not usable
__device__ __forceinline__ bool point(const Geo& g, int x, int y, double (&p)[3]) {
  const int idx = y * g.W + x;
  const float a = g.alpha[idx];
  if (!(a >= g.alpha_min)) return false;
  const double z = (double)g.depth[idx] / (double)a;
  p[0] = z * ray(x, g.W, g.tfx), p[1] = z * ray(y, g.H, g.tfy), p[2] = z;
  return true;
}
__device__ __forceinline__ void cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1], c[1] = a[2] * b[0] - a[0] * b[2], c[2] = a[0] * b[1] - a[1] * b[0];
}
// n, s and the tangents of a valid pixel; false: not valid (every neighbour that is read lies inside the image)
__device__ __forceinline__ bool normal_at(const Geo& g, int x, int y, double (&n)[3], double (&tx)[3], double (&ty)[3], double* s) {
  if (x < 1 || y < 1 || x > g.W - 2 || y > g.H - 2) return false;
  const int idx = y * g.W + x;
  if (g.mask && g.mask[idx] == 0) return false;
  if (!(g.alpha[idx] >= g.alpha_min)) return false;
  double l[3], r[3], u[3], d[3], c[3];
  if (!point(g, x - 1, y, l) || !point(g, x + 1, y, r) || !point(g, x, y - 1, u) || !point(g, x, y + 1, d)) return false;
#pragma unroll
  for (int k = 0; k < 3; k++) tx[k] = r[k] - l[k], ty[k] = d[k] - u[k];
  cross(ty, tx, c);
  const double cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  if (!(cc > 0.0) || !(cc < HUGE_VAL)) return false;
  *s = sqrt(cc);
#pragma unroll
  for (int k = 0; k < 3; k++) n[k] = c[k] / *s;
  return true;
}
// (depthprior.hip::last_arrival: one counter per view, gridDim.x arrivals each)
__device__ __forceinline__ bool last_arrival(uint32_t* ticket, uint32_t* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *flag = t == gridDim.x - 1u;
  }
  __syncthreads();
  return *flag != 0u;
}

__global__ void __launch_bounds__(TPB) normal_prior_forward_kernel(Batch b) {
  __shared__ double red[TPB / B3GS_WAVE][NQ];
  __shared__ uint32_t last;
  const View& v = b.v[blockIdx.y];
  const Geo& g = v.g;
  const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
  double* part = v.ws + HEAD;
  double* adj = part + part_doubles(v.nb);
  if (blk < v.nb) {                                                  // (uniform per workgroup)
    double q[NQ] = {0.0, 0.0, 0.0};
    const int idx = blk * TPB + tid;
    if (idx < g.npix) {
      const int x = idx % g.W, y = idx / g.W;
      double n[3] = {0.0, 0.0, 0.0}, tx[3], ty[3], s, gtx[3] = {0.0, 0.0, 0.0}, gty[3] = {0.0, 0.0, 0.0};
      const bool ok = normal_at(g, x, y, n, tx, ty, &s);
      if (ok) {
        double t[3], h[3], e[3];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = (double)v.target[(size_t)k * g.npix + idx];
        const double dot = (n[0] * t[0] + n[1] * t[1]) + n[2] * t[2];
        double df[3];
#pragma unroll
        for (int k = 0; k < 3; k++) df[k] = n[k] - t[k];
        q[0] = 1.0, q[1] = 1.0 - dot, q[2] = (fabs(df[0]) + fabs(df[1])) + fabs(df[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const double sg = df[k] > 0.0 ? 1.0 : df[k] < 0.0 ? -1.0 : 0.0;
          h[k] = v.wl * sg - v.wc * t[k];
        }
        const double d = (n[0] * h[0] + n[1] * h[1]) + n[2] * h[2];
#pragma unroll
        for (int k = 0; k < 3; k++) e[k] = (h[k] - n[k] * d) / s;
        cross(tx, e, gty);
        cross(e, ty, gtx);
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        adj[(size_t)k * g.npix + idx] = gtx[k];
        adj[(size_t)(3 + k) * g.npix + idx] = gty[k];
      }
      if (v.normals) {
#pragma unroll
        for (int k = 0; k < 3; k++) v.normals[(size_t)k * g.npix + idx] = (float)n[k];
      }
      if (v.valid) v.valid[idx] = ok ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < NQ; k++) {
      const double s = b3gs_wave_sum(q[k]);
      if ((tid & (B3GS_WAVE - 1)) == 0) red[tid / B3GS_WAVE][k] = s;
    }
    __syncthreads();
    if (tid < NQ) st(part + (size_t)blk * NQ + tid, (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]));
  }
  uint32_t* ticket = reinterpret_cast<uint32_t*>(v.ws);
  if (!last_arrival(ticket, &last)) return;
  if (tid >= B3GS_WAVE) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double s[NQ] = {0.0, 0.0, 0.0};
  for (int bb = tid; bb < v.nb; bb += B3GS_WAVE) {
    double w[NQ];
#pragma unroll
    for (int k = 0; k < NQ; k++) w[k] = ld(part + (size_t)bb * NQ + k);
#pragma unroll
    for (int k = 0; k < NQ; k++) s[k] += w[k];
  }
#pragma unroll
  for (int k = 0; k < NQ; k++) s[k] = b3gs_wave_sum(s[k]);
  if (tid) return;
  const double N = s[0];
  double ct = 0.0, lt = 0.0, L = 0.0, inv = 0.0, mean = 0.0;
  if (N > 0.0) {
    ct = s[1] / N, lt = s[2] / N;
    L = v.wc * ct + v.wl * lt;
    inv = 1.0 / N, mean = 1.0 - ct;
  }
  v.ws[H_INV] = inv;
  v.parts[0] = L, v.parts[1] = ct, v.parts[2] = lt, v.parts[3] = N, v.parts[4] = mean, v.parts[5] = 0.0;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TPB) normal_prior_gather_kernel(Batch b) {
  const View& v = b.v[blockIdx.y];
  const Geo& g = v.g;
  const int idx = (int)(blockIdx.x * TPB + threadIdx.x);
  if (idx >= g.npix) return;
  const float a = g.alpha[idx];
  if (!(a >= g.alpha_min)) {
    v.gd[idx] = 0.0f, v.ga[idx] = 0.0f;
    return;
  }
  const int x = idx % g.W, y = idx / g.W;
  const double* adj = v.ws + HEAD + part_doubles(v.nb);
  const double inv = v.ws[H_INV];
  double gp[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double* gtx = adj + (size_t)k * g.npix;
    const double* gty = adj + (size_t)(3 + k) * g.npix;
    const double A = x >= 1 ? gtx[idx - 1] : 0.0, B = x <= g.W - 2 ? gtx[idx + 1] : 0.0;
    const double C = y >= 1 ? gty[idx - g.W] : 0.0, D = y <= g.H - 2 ? gty[idx + g.W] : 0.0;
    gp[k] = ((A - B) + C) - D;
  }
  const double z = (double)g.depth[idx] / (double)a;
  const double gz = ((gp[0] * ray(x, g.W, g.tfx) + gp[1] * ray(y, g.H, g.tfy)) + gp[2]) * inv;
  v.gd[idx] = (float)(gz / (double)a);
  v.ga[idx] = (float)((0.0 - gz * z) / (double)a);
}

__global__ void __launch_bounds__(TPB) depth_normals_kernel(NBatch b) {
  const NView& v = b.v[blockIdx.y];
  const Geo& g = v.g;
  const int idx = (int)(blockIdx.x * TPB + threadIdx.x);
  if (idx >= g.npix) return;
  double n[3] = {0.0, 0.0, 0.0}, tx[3], ty[3], s;
  const bool ok = normal_at(g, idx % g.W, idx / g.W, n, tx, ty, &s);
#pragma unroll
  for (int k = 0; k < 3; k++) v.normals[(size_t)k * g.npix + idx] = (float)n[k];
  v.valid[idx] = ok ? 1 : 0;
}

// ---- resize ----------------------------------------------------------------------------------------------------------------
struct RView {
  int32_t Wsrc, Hsrc, W, H, npix, nsrc;
  float sx, sy;
  const float* src;
  const uint8_t* src_mask;
  float* normals;
  uint8_t* mask;
};
struct RBatch {
  int32_t n;
  RView v[B3GS_NORMAL_PRIOR_MAX_VIEWS];
};

__global__ void __launch_bounds__(TPB) normal_resize_kernel(RBatch b) {
  const RView& v = b.v[blockIdx.y];
  const int idx = (int)(blockIdx.x * TPB + threadIdx.x);
  if (idx >= v.npix) return;
  const int x = idx % v.W, y = idx / v.W;
  const float sx = fmaf((float)x + 0.5f, v.sx, -0.5f), sy = fmaf((float)y + 0.5f, v.sy, -0.5f);
  const float bx = floorf(sx), by = floorf(sy);
  const float fx = sx - bx, fy = sy - by;
  const int xa = min(max((int)bx, 0), v.Wsrc - 1), xb = min(max((int)bx + 1, 0), v.Wsrc - 1);
  const int ya = min(max((int)by, 0), v.Hsrc - 1), yb = min(max((int)by + 1, 0), v.Hsrc - 1);
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float w[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
  const int at[4] = {ya * v.Wsrc + xa, ya * v.Wsrc + xb, yb * v.Wsrc + xa, yb * v.Wsrc + xb};
  float p[4][3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    p[k][0] = p[k][1] = p[k][2] = 0.0f;
    if (w[k] != 0.0f) {
      const float s0 = v.src[at[k]], s1 = v.src[(size_t)v.nsrc + at[k]], s2 = v.src[2 * (size_t)v.nsrc + at[k]];
      const bool good = isfinite(s0) && isfinite(s1) && isfinite(s2) && (!v.src_mask || v.src_mask[at[k]] != 0);
      ok = ok && good;
      if (good) p[k][0] = s0, p[k][1] = s1, p[k][2] = s2;
    }
  }
  double val[3];
#pragma unroll
  for (int c = 0; c < 3; c++) val[c] = (double)fmaf(w[3], p[3][c], fmaf(w[2], p[2][c], fmaf(w[1], p[1][c], w[0] * p[0][c])));
  const double l = (val[0] * val[0] + val[1] * val[1]) + val[2] * val[2];
  ok = ok && l >= 0.25;
  const double s = sqrt(l);
#pragma unroll
  for (int c = 0; c < 3; c++) v.normals[(size_t)c * v.npix + idx] = ok ? (float)(val[c] / s) : 0.0f;
  v.mask[idx] = ok ? 1 : 0;
}

static const char* geo_error(int32_t W, int32_t H, const float* depth, const float* alpha, float alpha_min, double tfx, double tfy) {
  if (!size_ok(W, H)) return "1 <= W, H and W H <= 2^24";
  if (!depth || !alpha) return "NULL pointer";
  if (!(alpha_min > 0.0f)) return "alpha_min > 0 (and not NaN)";
  if (!(tfx > 0.0) || !(tfy > 0.0) || !(tfx < HUGE_VAL) || !(tfy < HUGE_VAL)) return "tanfovx, tanfovy > 0 and finite";
  return nullptr;
}
static Geo geo_of(int32_t W, int32_t H, const float* depth, const float* alpha, const uint8_t* mask, float alpha_min, double tfx, double tfy) {
  Geo g;
  g.W = W, g.H = H, g.npix = W * H, g.alpha_min = alpha_min, g.tfx = tfx, g.tfy = tfy;
  g.depth = depth, g.alpha = alpha, g.mask = mask;
  return g;
}

}  // namespace

extern "C" size_t b3gs_normal_prior_workspace_bytes(int32_t W, int32_t H) {
  if (!size_ok(W, H)) return 0;
  const int64_t npix = (int64_t)W * H;
  return b3gs_align256(sizeof(double) * (HEAD + part_doubles(nblocks(npix)) + (size_t)NADJ * (size_t)npix));
}

extern "C" int b3gs_normal_prior_loss_batch(int32_t n_views, const B3gsNormalPriorIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_normal_prior_loss_batch";
  if (n_views < 1 || n_views > B3GS_NORMAL_PRIOR_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_views <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  Batch b = {};
  b.n = n_views;
  int gridx = 0;
  for (int k = 0; k < n_views; k++) {
    const B3gsNormalPriorIO& s = io[k];
    if (const char* bad = geo_error(s.W, s.H, s.depth, s.alpha, s.alpha_min, s.tanfovx, s.tanfovy)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (s.w_cos != s.w_cos || s.w_l1 != s.w_l1) return b3gs_fail(B3GS_ERR_ARG, what, "a weight is NaN");
    if (!s.target || !s.dL_ddepth || !s.dL_dalpha || !s.parts) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    if (!aligned256(s.workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
    View& v = b.v[k];
    v.g = geo_of(s.W, s.H, s.depth, s.alpha, s.mask, s.alpha_min, s.tanfovx, s.tanfovy);
    v.nb = nblocks(v.g.npix);
    v.wc = s.w_cos, v.wl = s.w_l1;
    v.target = s.target, v.gd = s.dL_ddepth, v.ga = s.dL_dalpha, v.normals = s.normals, v.valid = s.valid;
    v.parts = s.parts, v.ws = static_cast<double*>(s.workspace);
    gridx = v.nb > gridx ? v.nb : gridx;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(normal_prior_forward_kernel, dim3(gridx, n_views), dim3(TPB), 0, s, b);
  hipLaunchKernelGGL(normal_prior_gather_kernel, dim3(gridx, n_views), dim3(TPB), 0, s, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_depth_normals_batch(int32_t n_views, const B3gsDepthNormalsIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_depth_normals_batch";
  if (n_views < 1 || n_views > B3GS_NORMAL_PRIOR_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_views <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  NBatch b = {};
  b.n = n_views;
  int gridx = 0;
  for (int k = 0; k < n_views; k++) {
    const B3gsDepthNormalsIO& s = io[k];
    if (const char* bad = geo_error(s.W, s.H, s.depth, s.alpha, s.alpha_min, s.tanfovx, s.tanfovy)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (!s.normals || !s.valid) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    b.v[k].g = geo_of(s.W, s.H, s.depth, s.alpha, s.mask, s.alpha_min, s.tanfovx, s.tanfovy);
    b.v[k].normals = s.normals, b.v[k].valid = s.valid;
    gridx = nblocks(b.v[k].g.npix) > gridx ? nblocks(b.v[k].g.npix) : gridx;
  }
  hipLaunchKernelGGL(depth_normals_kernel, dim3(gridx, n_views), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_resize_normals_batch(int32_t n_views, const B3gsNormalResizeIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_resize_normals_batch";
  if (n_views < 1 || n_views > B3GS_NORMAL_PRIOR_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_views <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  RBatch b = {};
  b.n = n_views;
  int gridx = 0;
  for (int k = 0; k < n_views; k++) {
    const B3gsNormalResizeIO& s = io[k];
    if (!size_ok(s.W, s.H) || !size_ok(s.Wsrc, s.Hsrc)) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= W, H, W H <= 2^24 for the source and the output");
    if (!s.src || !s.normals || !s.mask) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    RView& v = b.v[k];
    v.Wsrc = s.Wsrc, v.Hsrc = s.Hsrc, v.W = s.W, v.H = s.H, v.npix = s.W * s.H, v.nsrc = s.Wsrc * s.Hsrc;
    v.sx = (float)s.Wsrc / (float)s.W, v.sy = (float)s.Hsrc / (float)s.H;
    v.src = s.src, v.src_mask = s.src_mask, v.normals = s.normals, v.mask = s.mask;
    gridx = nblocks(v.npix) > gridx ? nblocks(v.npix) : gridx;
  }
  hipLaunchKernelGGL(normal_resize_kernel, dim3(gridx, n_views), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}
