// Depth priors (added to ABI 18; binocular3dgs_amd/depth_prior.py): the scale- and shift-invariant
// Pearson loss between the rendered depth and a prior plane -- over the whole image and over the patches of a movable grid --
// with its gradient, and the bilinear resize that brings a prior of any size to the training size.
// include/b3gs_raster.h states every rule; tests/depth_prior_ref.py restates them in numpy float64.
//   sums      grid (image blocks + patches, views).  An image block: thread = pixel, six fp64 quantities, the fixed tree of
//             b3gs_block_sum_f64.  A patch: thread t walks the patch's pixels t, t + 256, .. in row-major patch order, the same
//             tree, and thread 0 derives the patch's means, centred sums and rho.  The LAST workgroup of a view to arrive (the
//             arrival counter of poisson.hip: release / acquire at agent scope, nobody waits) folds the image partials and the
//             patch terms with one wave in a fixed order, writes `parts` and resets the counter.
//   gradient  thread = pixel: reads the image row and its patch's row, writes its own word.
//   resize    thread = output pixel, float32 fma in the stated order.
// fp64 throughout the loss, only + - * / sqrt (the Makefile compiles with -ffp-contract=off); no floating-point atomic, no
// scratch, no host read.  The kernels are bandwidth-trivial next to the rasterizer: the point is one fixed operation order.
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int NQ = 6;
constexpr int HEAD = 32;              // doubles: [0] the arrival counter (its low word), [H_ROW ..] the image's row, [H_COUNT]
constexpr int ROW = 16;               // doubles of a patch row (and of the image's row in the head)
constexpr int H_ROW = 8, H_COUNT = 24;
enum { S_N = 0, S_X, S_Y, S_XX, S_YY, S_XY, D_FLAG, D_MX, D_MY, D_CXX, D_DEN, D_RHO, D_TERM, D_CXY, D_CYY };

struct View {
  int32_t W, H, npix, nbg, gx, npatch, patch, mode, min_valid;
  float alpha_min;
  double wg, wl;
  const float* depth;
  const float* alpha;
  const float* prior;
  const uint8_t* mask;
  const int32_t* off;
  float* grad;
  double* parts;
  double* ws;
};
struct Batch {
  int32_t n;
  View v[B3GS_DEPTH_PRIOR_MAX_VIEWS];
};

static inline int nblocks(int64_t n) { return (int)((n + TPB - 1) / TPB); }
__host__ __device__ static inline size_t part_doubles(int nbg) { return ((size_t)NQ * nbg + 31) / 32 * 32; }
static inline bool aligned256(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

__device__ __forceinline__ void st(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
}

// (x, y, t') of a used pixel; false: not used
__device__ __forceinline__ bool pixel(const View& v, int idx, double* x, double* y, double* t) {
  if (v.mask[idx] == 0 || !(v.alpha[idx] >= v.alpha_min)) return false;
  const double d = (double)v.depth[idx];
  if (v.mode == B3GS_DEPTH_PRIOR_DISPARITY) {
    const double r = 1.0 / (d + 1e-5);
    *x = r, *t = 0.0 - r * r;
  } else {
    *x = d, *t = 1.0;
  }
  *y = (double)v.prior[idx];
  return true;
}
__device__ __forceinline__ void add_pixel(const View& v, int idx, double (&q)[NQ]) {
  double x, y, t;
  if (!pixel(v, idx, &x, &y, &t)) return;
  q[S_N] += 1.0, q[S_X] += x, q[S_Y] += y, q[S_XX] += x * x, q[S_YY] += y * y, q[S_XY] += x * y;
}
__device__ __forceinline__ void offsets(const View& v, int* ox, int* oy) {
  int a = 0, b = 0;
  if (v.off) a = v.off[0], b = v.off[1];
  *ox = min(max(a, 0), v.patch - 1), *oy = min(max(b, 0), v.patch - 1);
}
// the derived entries of a row from its six sums (a skipped set: all zero)
__device__ __forceinline__ void derive(const double (&s)[NQ], int min_valid, double (&d)[ROW]) {
#pragma unroll
  for (int k = 0; k < ROW; k++) d[k] = k < NQ ? s[k] : 0.0;
  const double n = s[S_N];
  if (!(n >= (double)min_valid)) return;
  const double cxx = s[S_XX] - (s[S_X] * s[S_X]) / n, cyy = s[S_YY] - (s[S_Y] * s[S_Y]) / n, cxy = s[S_XY] - (s[S_X] * s[S_Y]) / n;
  if (!(cxx > 0.0) || !(cyy > 0.0)) return;
  const double den = sqrt(cxx * cyy), rho = cxy / den;
  d[D_FLAG] = 1.0, d[D_MX] = s[S_X] / n, d[D_MY] = s[S_Y] / n, d[D_CXX] = cxx, d[D_DEN] = den, d[D_RHO] = rho, d[D_TERM] = 1.0 - rho;
  d[D_CXY] = cxy, d[D_CYY] = cyy;
}
__device__ __forceinline__ double gradient_of(const double* row, double x, double y, double t) {
  const double u = (y - row[D_MY]) / row[D_DEN], w = (row[D_RHO] * (x - row[D_MX])) / row[D_CXX];
  return (0.0 - (u - w)) * t;
}
// every thread of every workgroup of the launch calls this once: true in every thread of the workgroup of ITS VIEW that arrives
// last (poisson.hip::last_arrival, one counter per view: gridDim.x arrivals each)
__device__ __forceinline__ bool last_arrival(uint32_t* ticket, uint32_t* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *flag = t == gridDim.x - 1u;
  }
  __syncthreads();
  return *flag != 0u;
}

__global__ void __launch_bounds__(TPB) depth_prior_sums_kernel(Batch b) {
  __shared__ double red[TPB / B3GS_WAVE][NQ];
  __shared__ uint32_t last;
  const View& v = b.v[blockIdx.y];
  const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
  double* gpart = v.ws + HEAD;
  double* prow = gpart + part_doubles(v.nbg);
  if (blk < v.nbg + v.npatch) {                                      // (uniform per workgroup)
    double q[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool image = blk < v.nbg;
    if (image) {
      const int idx = blk * TPB + tid;
      if (idx < v.npix) add_pixel(v, idx, q);
    } else {
      const int pid = blk - v.nbg, p = v.patch, pp = p * p;
      int ox, oy;
      offsets(v, &ox, &oy);
      const int x0 = (pid % v.gx) * p - ox, y0 = (pid / v.gx) * p - oy;
      for (int k = tid; k < pp; k += TPB) {
        const int x = x0 + k % p, y = y0 + k / p;
        if (x >= 0 && x < v.W && y >= 0 && y < v.H) add_pixel(v, y * v.W + x, q);
      }
    }
#pragma unroll
    for (int k = 0; k < NQ; k++) {
      const double s = b3gs_wave_sum(q[k]);
      if ((tid & (B3GS_WAVE - 1)) == 0) red[tid / B3GS_WAVE][k] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double s[NQ];
#pragma unroll
      for (int k = 0; k < NQ; k++) s[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
      if (image) {
#pragma unroll
        for (int k = 0; k < NQ; k++) st(gpart + (size_t)blk * NQ + k, s[k]);
      } else {
        double d[ROW];
        derive(s, v.min_valid, d);
        double* row = prow + (size_t)(blk - v.nbg) * ROW;
#pragma unroll
        for (int k = 0; k < ROW; k++) st(row + k, d[k]);
      }
    }
  }
  uint32_t* ticket = reinterpret_cast<uint32_t*>(v.ws);
  if (!last_arrival(ticket, &last)) return;
  if (tid >= B3GS_WAVE) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double s[NQ] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int bb = tid; bb < v.nbg; bb += B3GS_WAVE) {                  // (the six loads of a partial in flight together)
    double w[NQ];
#pragma unroll
    for (int k = 0; k < NQ; k++) w[k] = ld(gpart + (size_t)bb * NQ + k);
#pragma unroll
    for (int k = 0; k < NQ; k++) s[k] += w[k];
  }
#pragma unroll
  for (int k = 0; k < NQ; k++) s[k] = b3gs_wave_sum(s[k]);
  double tsum = 0.0, csum = 0.0;
  for (int pid = tid; pid < v.npatch; pid += B3GS_WAVE) {
    tsum += ld(prow + (size_t)pid * ROW + D_TERM);
    csum += ld(prow + (size_t)pid * ROW + D_FLAG);
  }
  tsum = b3gs_wave_sum(tsum), csum = b3gs_wave_sum(csum);
  if (tid) return;
  double d[ROW];
  derive(s, v.min_valid, d);
  const double mean = csum > 0.0 ? tsum / csum : 0.0;
  double a = 0.0, off = 0.0;
  if (d[D_FLAG] != 0.0) {
    a = d[D_CXY] / d[D_CYY];
    off = d[D_MX] - a * d[D_MY];
  }
#pragma unroll
  for (int k = 0; k < ROW; k++) v.ws[H_ROW + k] = d[k];
  v.ws[H_COUNT] = csum;
  v.parts[0] = v.wg * d[D_TERM] + v.wl * mean;
  v.parts[1] = d[D_TERM], v.parts[2] = mean, v.parts[3] = s[S_N], v.parts[4] = csum, v.parts[5] = d[D_RHO], v.parts[6] = a, v.parts[7] = off;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TPB) depth_prior_grad_kernel(Batch b) {
  const View& v = b.v[blockIdx.y];
  const int idx = (int)(blockIdx.x * TPB + threadIdx.x);
  if (idx >= v.npix) return;
  double x, y, t;
  if (!pixel(v, idx, &x, &y, &t)) {
    v.grad[idx] = 0.0f;
    return;
  }
  const double* head = v.ws + H_ROW;
  const double count = v.ws[H_COUNT];
  double gg = 0.0, gp = 0.0;
  if (head[D_FLAG] != 0.0) gg = gradient_of(head, x, y, t);
  if (v.npatch > 0 && count > 0.0) {
    int ox, oy;
    offsets(v, &ox, &oy);
    const int i = (idx % v.W + ox) / v.patch, j = (idx / v.W + oy) / v.patch;
    const double* row = v.ws + HEAD + part_doubles(v.nbg) + (size_t)(j * v.gx + i) * ROW;
    if (row[D_FLAG] != 0.0) gp = gradient_of(row, x, y, t);
  }
  const double lg = v.wg * gg;
  const double lp = count > 0.0 ? (v.wl * gp) / count : 0.0;
  v.grad[idx] = (float)(lg + lp);
}

// ---- resize ----------------------------------------------------------------------------------------------------------------
struct RView {
  int32_t Wsrc, Hsrc, W, H, npix;
  float sx, sy;
  const float* src;
  const uint8_t* src_mask;
  float* prior;
  uint8_t* mask;
};
struct RBatch {
  int32_t n;
  RView v[B3GS_DEPTH_PRIOR_MAX_VIEWS];
};

__global__ void __launch_bounds__(TPB) depth_resize_kernel(RBatch b) {
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
  float p[4];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    p[k] = 0.0f;
    if (w[k] != 0.0f) {
      const float s = v.src[at[k]];
      const bool valid = isfinite(s) && s > 0.0f && (!v.src_mask || v.src_mask[at[k]] != 0);
      ok = ok && valid;
      p[k] = valid ? s : 0.0f;
    }
  }
  const float val = fmaf(w[3], p[3], fmaf(w[2], p[2], fmaf(w[1], p[1], w[0] * p[0])));
  v.prior[idx] = ok ? val : 0.0f;
  v.mask[idx] = ok ? 1 : 0;
}

}  // namespace

extern "C" size_t b3gs_depth_prior_workspace_bytes(int32_t W, int32_t H, int32_t patch) {
  if (W < 1 || H < 1 || (int64_t)W * H > (1 << 24) || !(patch == 0 || (patch >= 8 && patch <= 256))) return 0;
  const int nbg = nblocks((int64_t)W * H);
  const size_t np = patch ? (size_t)((W + patch - 1) / patch + 1) * (size_t)((H + patch - 1) / patch + 1) : 0;
  return b3gs_align256(sizeof(double) * (HEAD + part_doubles(nbg) + (size_t)ROW * np));
}

extern "C" int b3gs_depth_prior_loss_batch(int32_t n_views, const B3gsDepthPriorIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_depth_prior_loss_batch";
  if (n_views < 1 || n_views > B3GS_DEPTH_PRIOR_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_views <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  Batch b = {};
  b.n = n_views;
  int gridx = 0;
  for (int k = 0; k < n_views; k++) {
    const B3gsDepthPriorIO& s = io[k];
    if (!b3gs_depth_prior_workspace_bytes(s.W, s.H, s.patch)) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= W, H, W H <= 2^24; patch is 0 or 8 .. 256");
    if (s.mode != B3GS_DEPTH_PRIOR_DEPTH && s.mode != B3GS_DEPTH_PRIOR_DISPARITY) return b3gs_fail(B3GS_ERR_ARG, what, "mode is B3GS_DEPTH_PRIOR_DEPTH or B3GS_DEPTH_PRIOR_DISPARITY");
    if (s.min_valid < 2) return b3gs_fail(B3GS_ERR_ARG, what, "min_valid >= 2");
    if (s.alpha_min != s.alpha_min || s.w_global != s.w_global || s.w_local != s.w_local) return b3gs_fail(B3GS_ERR_ARG, what, "alpha_min or a weight is NaN");
    if (!s.depth || !s.alpha || !s.prior || !s.mask || !s.dL_ddepth || !s.parts) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    if (!aligned256(s.workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
    View& v = b.v[k];
    v.W = s.W, v.H = s.H, v.npix = s.W * s.H, v.nbg = nblocks(v.npix);
    v.patch = s.patch;
    v.gx = s.patch ? (s.W + s.patch - 1) / s.patch + 1 : 0;
    v.npatch = s.patch ? v.gx * ((s.H + s.patch - 1) / s.patch + 1) : 0;
    v.mode = s.mode, v.min_valid = s.min_valid, v.alpha_min = s.alpha_min;
    v.wg = s.w_global, v.wl = s.patch ? s.w_local : 0.0;
    v.depth = s.depth, v.alpha = s.alpha, v.prior = s.prior, v.mask = s.mask, v.off = s.offset_dev;
    v.grad = s.dL_ddepth, v.parts = s.parts, v.ws = static_cast<double*>(s.workspace);
    if (v.nbg + v.npatch > gridx) gridx = v.nbg + v.npatch;
  }
  int gridg = 0;
  for (int k = 0; k < n_views; k++) gridg = b.v[k].nbg > gridg ? b.v[k].nbg : gridg;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(depth_prior_sums_kernel, dim3(gridx, n_views), dim3(TPB), 0, s, b);
  hipLaunchKernelGGL(depth_prior_grad_kernel, dim3(gridg, n_views), dim3(TPB), 0, s, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_resize_depth_batch(int32_t n_views, const B3gsDepthResizeIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_resize_depth_batch";
  if (n_views < 1 || n_views > B3GS_DEPTH_PRIOR_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_views <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  RBatch b = {};
  b.n = n_views;
  int gridx = 0;
  for (int k = 0; k < n_views; k++) {
    const B3gsDepthResizeIO& s = io[k];
    if (s.W < 1 || s.H < 1 || s.Wsrc < 1 || s.Hsrc < 1 || (int64_t)s.W * s.H > (1 << 24) || (int64_t)s.Wsrc * s.Hsrc > (1 << 24))
      return b3gs_fail(B3GS_ERR_ARG, what, "1 <= W, H, W H <= 2^24 for the source and the output");
    if (!s.src || !s.prior || !s.mask) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    RView& v = b.v[k];
    v.Wsrc = s.Wsrc, v.Hsrc = s.Hsrc, v.W = s.W, v.H = s.H, v.npix = s.W * s.H;
    v.sx = (float)s.Wsrc / (float)s.W, v.sy = (float)s.Hsrc / (float)s.H;
    v.src = s.src, v.src_mask = s.src_mask, v.prior = s.prior, v.mask = s.mask;
    gridx = nblocks(v.npix) > gridx ? nblocks(v.npix) : gridx;
  }
  hipLaunchKernelGGL(depth_resize_kernel, dim3(gridx, n_views), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}
