// Per-image exposure compensation (added to ABI 18; binocular3dgs_amd/exposure.py): the 3x4 affine
// colour transform of upstream 3DGS applied to a render before the loss, its backward with the 12 gradient sums of the matrix,
// the closed-form fit of the best transform between a render and a photo (colour-corrected PSNR), and a row-sparse Adam for
// the table of matrices.  include/b3gs_raster.h states every rule; tests/exposure_ref.py restates them in numpy float64.
//   apply     thread = pixel: out_c = ((t_c + a_c0 r) + a_c1 g) + a_c2 b in fp64, one rounding.  The matrix is 12 floats, or
//             row *row_dev of a table: read on the device, so a graph replay changes the view.
//   backward  thread = pixel: g_in, and the 12 products g_out_c x_k as one partial per 256-pixel block (the fixed tree of
//             depthprior.hip).  The LAST workgroup of a plane to arrive (one counter per plane, release / acquire at agent
//             scope, nobody waits) reports to its GROUP -- the planes that share a matrix --, and the last plane of the group
//             folds every plane's partials in block order and adds the planes in plane order: one G per matrix.
//   fit       the same scheme over 22 sums; the last workgroup solves the three 4x4 systems by one Cholesky factorisation.
//   adam      one launch of 12 lanes on the row the word names.
// fp64 throughout, only + - * / sqrt (the Makefile compiles with -ffp-contract=off); no floating-point atomic, no scratch, no
// host read, no allocation.  The counters reset themselves.
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int NG = 12;                // sums of the backward
constexpr int NF = 22;                // sums of the fit: the 10 unique entries of S, then the 12 of B
constexpr int HEAD = 32;              // doubles: the plane's counter (word 0) and its group's (word 1, used in the leader's)
constexpr int SLOT = 24;              // doubles of a block's partial (NG or NF used)

struct Plane {
  int32_t W, H, npix, nb, V, leader, members;
  const float* in;
  const float* g_out;
  float* out;
  const float* A;
  const int32_t* row;
  double* G;
  double* ws;
};
struct Batch {
  int32_t n;
  Plane v[B3GS_EXPOSURE_MAX_PLANES];
};
struct FitPlane {
  int32_t W, H, npix, nb;
  const float* render;
  const float* gt;
  const uint8_t* mask;
  float* A;
  double* sums;
  int32_t* flag;
  double* ws;
};
struct FitBatch {
  int32_t n;
  FitPlane v[B3GS_EXPOSURE_MAX_PLANES];
};

static inline int nblocks(int64_t n) { return (int)((n + TPB - 1) / TPB); }
static inline bool aligned256(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 255u) == 0; }

__device__ __forceinline__ void st(double* p, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT));
}
// the 12 floats of a plane's matrix (a row word outside the table is clamped into it)
__device__ __forceinline__ const float* matrix_of(const Plane& v) {
  if (!v.row) return v.A;
  const int r = min(max(*v.row, 0), v.V - 1);
  return v.A + (size_t)NG * r;
}
// every thread of the workgroup calls this once: true in every thread of the workgroup that is arrival number `expected` of
// `ticket` (depthprior.hip::last_arrival with the count as an argument)
__device__ __forceinline__ bool last_arrival(uint32_t* ticket, uint32_t expected, uint32_t* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *flag = t == expected - 1u;
  }
  __syncthreads();
  return *flag != 0u;
}
// the block's partial of NQ sums: the tree of depthprior.hip, stored by thread 0 past the L1
template <int NQ>
__device__ __forceinline__ void store_partial(const double (&q)[NQ], double (*red)[NQ], double* slot) {
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < NQ; k++) {
    const double s = b3gs_wave_sum(q[k]);
    if ((tid & (B3GS_WAVE - 1)) == 0) red[tid / B3GS_WAVE][k] = s;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < NQ; k++) st(slot + k, (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]));
  }
}
// ONE wave: lane l adds the partials l, l + 64, .. in order to +0, then the butterfly; every lane gets the NQ sums
template <int NQ>
__device__ __forceinline__ void fold(const double* part, int nb, double (&s)[NQ]) {
  const int lane = (int)threadIdx.x;
#pragma unroll
  for (int k = 0; k < NQ; k++) s[k] = 0.0;
  for (int b = lane; b < nb; b += B3GS_WAVE) {
    double w[NQ];
#pragma unroll
    for (int k = 0; k < NQ; k++) w[k] = ld(part + (size_t)b * SLOT + k);
#pragma unroll
    for (int k = 0; k < NQ; k++) s[k] += w[k];
  }
#pragma unroll
  for (int k = 0; k < NQ; k++) s[k] = b3gs_wave_sum(s[k]);
}

__global__ void __launch_bounds__(TPB) exposure_apply_kernel(Batch b) {
  const Plane& v = b.v[blockIdx.y];
  const int idx = (int)(blockIdx.x * TPB + threadIdx.x);
  if (idx >= v.npix) return;
  const float* a = matrix_of(v);
  const size_t n = (size_t)v.npix;
  const double r = (double)v.in[idx], g = (double)v.in[n + idx], bl = (double)v.in[2 * n + idx];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double s = (((double)a[4 * c + 3] + (double)a[4 * c] * r) + (double)a[4 * c + 1] * g) + (double)a[4 * c + 2] * bl;
    v.out[c * n + idx] = (float)s;
  }
}

__global__ void __launch_bounds__(TPB) exposure_backward_kernel(Batch b) {
  __shared__ double red[TPB / B3GS_WAVE][NG];
  __shared__ uint32_t last;
  const Plane& v = b.v[blockIdx.y];
  const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
  uint32_t* ticket = reinterpret_cast<uint32_t*>(v.ws);
  if (blk < v.nb) {                                                   // (uniform per workgroup)
    const float* a = matrix_of(v);
    const size_t n = (size_t)v.npix;
    const int idx = blk * TPB + tid;
    double q[NG];
#pragma unroll
    for (int k = 0; k < NG; k++) q[k] = 0.0;
    if (idx < v.npix) {
      const double x[3] = {(double)v.in[idx], (double)v.in[n + idx], (double)v.in[2 * n + idx]};
      const double g[3] = {(double)v.g_out[idx], (double)v.g_out[n + idx], (double)v.g_out[2 * n + idx]};
#pragma unroll
      for (int k = 0; k < 3; k++)
        v.out[k * n + idx] = (float)(((double)a[k] * g[0] + (double)a[4 + k] * g[1]) + (double)a[8 + k] * g[2]);
#pragma unroll
      for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[4 * c + k] = g[c] * x[k];
        q[4 * c + 3] = g[c];
      }
    }
    store_partial<NG>(q, red, v.ws + HEAD + (size_t)blk * SLOT);
  }
  if (!last_arrival(ticket, gridDim.x, &last)) return;
  // the last workgroup of this plane: the plane is done; is its group?
  const Plane& lead = b.v[v.leader];
  uint32_t* gticket = reinterpret_cast<uint32_t*>(lead.ws) + 1;
  if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!last_arrival(gticket, (uint32_t)lead.members, &last)) return;
  if (tid >= B3GS_WAVE) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double total[NG];
#pragma unroll
  for (int k = 0; k < NG; k++) total[k] = 0.0;
  for (int m = v.leader; m < b.n; m++) {                              // the members in plane order
    const Plane& p = b.v[m];
    if (p.leader != v.leader) continue;
    double s[NG];
    fold<NG>(p.ws + HEAD, p.nb, s);
#pragma unroll
    for (int k = 0; k < NG; k++) total[k] += s[k];
  }
  if (tid) return;
  float* g32 = reinterpret_cast<float*>(lead.G + NG);
#pragma unroll
  for (int k = 0; k < NG; k++) {
    lead.G[k] = total[k];
    g32[k] = (float)total[k];
  }
  __hip_atomic_store(gticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- fit -------------------------------------------------------------------------------------------------------------------
// S a_c = b_c, c = 0, 1, 2, by one Cholesky factorisation S = L L^T in the order the header states; false: degenerate
__device__ __forceinline__ bool solve(const double (&f)[NF], double (&A)[NG]) {
  // S[i][j], i <= j, in the order rr rg rb r gg gb g bb b n
  const int at[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
  const double n = f[9];
  if (!(n >= 16.0)) return false;
  const double trace = ((f[0] + f[4]) + f[7]) + f[9];
  const double thr = trace * 9.094947017729282379150390625e-13;       // 2^-40
  double L[4][4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double d = f[at[j][j]];
#pragma unroll
    for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k];
    if (!(d > thr)) return false;
    L[j][j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i < 4; i++) {
      double s = f[at[i][j]];
#pragma unroll
      for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double y[4], a[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      double s = f[10 + 4 * c + i];
#pragma unroll
      for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 3; i >= 0; i--) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < 4; k++) s = s - L[k][i] * a[k];
      a[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) A[4 * c + i] = a[i];
  }
  return true;
}

__global__ void __launch_bounds__(TPB) exposure_fit_kernel(FitBatch b) {
  __shared__ double red[TPB / B3GS_WAVE][NF];
  __shared__ uint32_t last;
  const FitPlane& v = b.v[blockIdx.y];
  const int blk = (int)blockIdx.x, tid = (int)threadIdx.x;
  uint32_t* ticket = reinterpret_cast<uint32_t*>(v.ws);
  if (blk < v.nb) {
    const size_t n = (size_t)v.npix;
    const int idx = blk * TPB + tid;
    double q[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) q[k] = 0.0;
    if (idx < v.npix && (!v.mask || v.mask[idx] != 0)) {
      const double x[4] = {(double)v.render[idx], (double)v.render[n + idx], (double)v.render[2 * n + idx], 1.0};
      const double y[3] = {(double)v.gt[idx], (double)v.gt[n + idx], (double)v.gt[2 * n + idx]};
      int at = 0;
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = i; j < 4; j++) q[at++] = x[i] * x[j];
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) q[10 + 4 * c + i] = x[i] * y[c];
    }
    store_partial<NF>(q, red, v.ws + HEAD + (size_t)blk * SLOT);
  }
  if (!last_arrival(ticket, gridDim.x, &last)) return;
  if (tid >= B3GS_WAVE) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double f[NF];
  fold<NF>(v.ws + HEAD, v.nb, f);
  if (tid) return;
  double A[NG] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  double sol[NG];
  const bool ok = solve(f, sol);
  v.sums[0] = f[9];
#pragma unroll
  for (int k = 0; k < NF; k++) v.sums[1 + k] = f[k];
#pragma unroll
  for (int k = 0; k < NG; k++) v.A[k] = (float)(ok ? sol[k] : A[k]);
  *v.flag = ok ? 0 : 1;
  __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- row-sparse Adam -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(B3GS_WAVE) exposure_adam_kernel(int32_t V, float* table, float* exp_avg, float* exp_avg_sq, int32_t* steps,
                                                                  double* prods, const int32_t* row_dev, const double* grad,
                                                                  const float* lr_dev, double beta1, double beta2, double eps,
                                                                  const int32_t* skip_if_nonzero) {
  // a step rendered from truncated tile lists is dropped here, on the device (optim.hip: adam_kernel, bump_step)
  if (skip_if_nonzero && *skip_if_nonzero != 0) return;
  const int row = *row_dev;
  if (row < 0 || row >= V) return;
  const int k = (int)threadIdx.x;
  const double p1 = prods[2 * row] * beta1, p2 = prods[2 * row + 1] * beta2;
  const int32_t step = steps[row];
  __syncthreads();                                                    // (every lane has read the row's products)
  if (k == 0) {
    prods[2 * row] = p1, prods[2 * row + 1] = p2;
    steps[row] = step + 1;
  }
  if (k >= NG) return;
  const size_t at = (size_t)NG * row + k;
  const double g = grad[k], lr = (double)*lr_dev;
  const double m = beta1 * (double)exp_avg[at] + (1.0 - beta1) * g;
  const double s = beta2 * (double)exp_avg_sq[at] + ((1.0 - beta2) * g) * g;
  const double mhat = m / (1.0 - p1);
  const double den = sqrt(s) / sqrt(1.0 - p2) + eps;
  exp_avg[at] = (float)m;
  exp_avg_sq[at] = (float)s;
  table[at] = (float)((double)table[at] - (lr * mhat) / den);
}

int fill(const char* what, int32_t n, const B3gsExposurePlane* io, bool backward, Batch* out, int* gridx) {
  if (n < 1 || n > B3GS_EXPOSURE_MAX_PLANES) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_planes <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  Batch& b = *out;
  b.n = n;
  *gridx = 0;
  for (int k = 0; k < n; k++) {
    const B3gsExposurePlane& s = io[k];
    if (!b3gs_exposure_workspace_bytes(s.W, s.H)) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= W, H, W H <= 2^24");
    if (!s.in || !s.out || !s.A) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    if (s.row_dev && s.V < 1) return b3gs_fail(B3GS_ERR_ARG, what, "a table has V >= 1 rows");
    Plane& v = b.v[k];
    v.W = s.W, v.H = s.H, v.npix = s.W * s.H, v.nb = nblocks(v.npix), v.V = s.V;
    v.in = s.in, v.g_out = s.g_out, v.out = s.out, v.A = s.A, v.row = s.row_dev, v.G = s.G, v.ws = static_cast<double*>(s.workspace);
    v.leader = k, v.members = 0;
    if (backward) {
      if (!s.g_out || !s.G) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
      if (!aligned256(s.workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
      for (int m = 0; m < k; m++) {
        const bool same = io[m].A == s.A && io[m].row_dev == s.row_dev;
        if (same && v.leader == k) v.leader = b.v[m].leader;
        if (same != (io[m].G == s.G)) return b3gs_fail(B3GS_ERR_ARG, what, "planes name the same G exactly when they share a matrix");
        if (io[m].workspace == s.workspace) return b3gs_fail(B3GS_ERR_ARG, what, "every plane has a workspace of its own");
      }
      b.v[v.leader].members++;
    }
    if (v.nb > *gridx) *gridx = v.nb;
  }
  return B3GS_OK;
}

}  // namespace

extern "C" size_t b3gs_exposure_workspace_bytes(int32_t W, int32_t H) {
  if (W < 1 || H < 1 || (int64_t)W * H > (1 << 24)) return 0;
  return b3gs_align256(sizeof(double) * (HEAD + (size_t)SLOT * nblocks((int64_t)W * H)));
}

extern "C" int b3gs_exposure_apply(int32_t n_planes, const B3gsExposurePlane* io, b3gs_stream_t stream) {
  const char* what = "b3gs_exposure_apply";
  Batch b = {};
  int gridx = 0;
  const int rc = fill(what, n_planes, io, false, &b, &gridx);
  if (rc != B3GS_OK) return rc;
  hipLaunchKernelGGL(exposure_apply_kernel, dim3(gridx, n_planes), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_exposure_backward(int32_t n_planes, const B3gsExposurePlane* io, b3gs_stream_t stream) {
  const char* what = "b3gs_exposure_backward";
  Batch b = {};
  int gridx = 0;
  const int rc = fill(what, n_planes, io, true, &b, &gridx);
  if (rc != B3GS_OK) return rc;
  hipLaunchKernelGGL(exposure_backward_kernel, dim3(gridx, n_planes), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_exposure_fit(int32_t n_planes, const B3gsExposureFitIO* io, b3gs_stream_t stream) {
  const char* what = "b3gs_exposure_fit";
  if (n_planes < 1 || n_planes > B3GS_EXPOSURE_MAX_PLANES) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= n_planes <= 8");
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  FitBatch b = {};
  b.n = n_planes;
  int gridx = 0;
  for (int k = 0; k < n_planes; k++) {
    const B3gsExposureFitIO& s = io[k];
    if (!b3gs_exposure_workspace_bytes(s.W, s.H)) return b3gs_fail(B3GS_ERR_ARG, what, "1 <= W, H, W H <= 2^24");
    if (!s.render || !s.gt || !s.A || !s.sums || !s.flag) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    if (!aligned256(s.workspace)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer, or a workspace that is not 256-byte aligned");
    for (int m = 0; m < k; m++)
      if (io[m].workspace == s.workspace) return b3gs_fail(B3GS_ERR_ARG, what, "every plane has a workspace of its own");
    FitPlane& v = b.v[k];
    v.W = s.W, v.H = s.H, v.npix = s.W * s.H, v.nb = nblocks(v.npix);
    v.render = s.render, v.gt = s.gt, v.mask = s.mask, v.A = s.A, v.sums = s.sums, v.flag = s.flag, v.ws = static_cast<double*>(s.workspace);
    if (v.nb > gridx) gridx = v.nb;
  }
  hipLaunchKernelGGL(exposure_fit_kernel, dim3(gridx, n_planes), dim3(TPB), 0, (hipStream_t)stream, b);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_exposure_adam(int32_t V, float* table, float* exp_avg, float* exp_avg_sq, int32_t* steps, double* prods,
                                  const int32_t* row_dev, const double* grad, const float* lr_dev, double beta1, double beta2,
                                  double eps, const int32_t* skip_if_nonzero, b3gs_stream_t stream) {
  const char* what = "b3gs_exposure_adam";
  if (V < 1) return b3gs_fail(B3GS_ERR_ARG, what, "V >= 1");
  if (!table || !exp_avg || !exp_avg_sq || !steps || !prods || !row_dev || !grad || !lr_dev) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= beta < 1, eps >= 0");
  hipLaunchKernelGGL(exposure_adam_kernel, dim3(1), dim3(B3GS_WAVE), 0, (hipStream_t)stream, V, table, exp_avg, exp_avg_sq, steps, prods,
                     row_dev, grad, lr_dev, beta1, beta2, eps, skip_if_nonzero);
  return b3gs_launch_status(what);
}
