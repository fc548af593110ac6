// The camera pose gradient as a reduction of the per-Gaussian gradients (added to ABI 18; binocular3dgs_amd/pose.py,
// INTEGRATION.md section 24).  include/b3gs_raster.h states the arithmetic; tests/pose_ref.py restates it in numpy float64.
//
// A render from a moved camera is the render of the inversely moved scene from the fixed camera, so dL/d(pose) is linear in
// the gradients the backward already produced.  For a world-frame twist (omega, t) of the SCENE about the pivot c:
//   dL/dt       = sum_i g_mu_i
//   dL/domega_k = sum_i [ ((mu_i - c) x g_mu_i)_k + 1/2 <g_q_i, e_k (x) q_i> + sum_l sum_c g_f_i[l,:,c]^T G_l^k f_i[l,:,c] ]
// with e_k (x) q the Hamilton product in (w, x, y, z) order on the raw quaternion and G_l^k = d/dtheta D_l(exp(theta e_k)) at 0,
// D_l the band rotation of edit.sh_rotation_matrices (Y_l(d)^T D_l = Y_l(R^T d)^T) in the basis of preprocess.hip.
//
// The generators, by hand: R^T d = d - theta e_k x d + O(theta^2), so Y_l(d)^T G_l^k = -((e_k x d) . grad) Y_l(d)^T: column m of
// G_l^k holds the coordinates, in the band's own basis, of the polynomial -((e_k x d) . grad) Y_l,m.  The operators are
//   x: z d/dy - y d/dz      y: x d/dz - z d/dx      z: y d/dx - x d/dy
// and e.g. for band 1 = C1 (-y, z, -x) about z: (y d/dx - x d/dy)(-y) = x = -Y_1,2 / C1 ... so G[2][0] = -1, and (..)(-x) = -y =
// Y_1,0 / C1, so G[0][2] = +1.  Every G is antisymmetric; the entries above the diagonal, G[j][m] with j < m (all others are 0 or
// their negatives), are
//   band 1 (3x3)   x: [0][1] = 1                      y: [1][2] = 1                       z: [0][2] = 1
//   band 2 (5x5)   x: [0][3] = 1, [1][2] = r3,        y: [0][1] = -1, [2][3] = r3,        z: [0][4] = 2, [1][3] = 1
//                     [1][4] = 1                         [3][4] = 1
//   band 3 (7x7)   x: [0][5] = r6/2, [1][4] = r10/2,  y: [0][1] = -r6/2, [1][2] = -r10/2, z: [0][6] = 3, [1][5] = 2, [2][4] = 1
//                     [1][6] = r6/2, [2][3] = r6,        [3][4] = r6, [4][5] = r10/2,
//                     [2][5] = r10/2                     [5][6] = r6/2
// with r3 = sqrt 3, r6 = sqrt 6, r10 = sqrt 10.  D is a homomorphism (Y(d)^T D(R1 R2) = Y(R2^T R1^T d)^T = Y(R1^T d)^T D(R2) =
// Y(d)^T D(R1) D(R2)), so the generators close as so(3) does: [G^x, G^y] = G^z and cyclic, in every band.
// With an antisymmetric G, g^T G f = sum_{j<m} G[j][m] (g_j f_m - g_m f_j): 1 / 8 / 13 terms per axis triple and channel.
//
// Layout.  Workgroup = 256 consecutive Gaussians, grid.y = the view.  Workgroup g of nb takes the chunks g, g + nb, .. of 256
// rows; nb = clamp(ceil(P / 1024), 1, 1024): four chunks per workgroup until 1024 workgroups (four per CU) are in flight.
// xyz / rotation and their gradients are 12- and 16-byte rows a wave reads as one contiguous run.  features_rest and its
// gradient are 36 / 96 / 180-byte rows: read by thread = Gaussian the 64 lanes of a load sit in 64 rows.  So the chunk's rows --
// ONE contiguous block of 256 K floats -- go through LDS as in edit.hip (lane i loads word i; row stride K | 1 words, odd: 32
// lanes on 32 banks): first the parameters, which the thread keeps in registers, then -- in the SAME LDS block -- the
// gradients (46 KB per workgroup at K = 45, where two blocks would allow one workgroup per CU).  The staging loads go out in
// batches of 9 / 12 / 15 per thread before their LDS stores (one load in flight per thread ran at 1.1 TB/s, the batches at
// 2.8 TB/s, 1M Gaussians, one view; K = 45 then takes 249 VGPRs: two workgroups per CU).  A skipped row is not loaded either.  fp64 throughout (-ffp-contract=off: no fused multiply-add), six sums per thread, b3gs_block_sum_f64 per
// workgroup, one wave per view folds the partials (b3gs_wave_fold_f64): no atomics, the same bits on every call.
#include "b3gs_internal.h"
#include <cfloat>

namespace {

constexpr int TPB = 256;
constexpr int NQ = 6;                 // tau_x tau_y tau_z f_x f_y f_z
constexpr int MAX_NB = 1024;
constexpr double R3 = 1.7320508075688772, R6 = 2.4494897427831779, R6H = 1.2247448713915890, R10H = 1.5811388300841898;

static int pose_blocks(int64_t P) {
  const int64_t b = (P + 4 * TPB - 1) / (4 * TPB);
  return (int)(b < 1 ? 1 : (b > MAX_NB ? MAX_NB : b));
}

struct PoseArgs {
  int32_t P, nb;
  const float *xyz, *rotation, *rest;
  const float* gx[B3GS_MAX_POSE_VIEWS];
  const float* gr[B3GS_MAX_POSE_VIEWS];
  const float* gf[B3GS_MAX_POSE_VIEWS];
  const uint8_t* skip[B3GS_MAX_POSE_VIEWS];
  double c[3];
  double* part;                       // [nviews][nb][NQ]
};

// s_k = s_k + a (g_j f_m - g_m f_j): one entry G[j][m] = a above the diagonal and its mirror
#define B3GS_POSE_TERM(s, a, j, m) s = s + (a) * (g[j] * f[m] - g[m] * f[j])

// one band (N = 3, 5, 7 coefficients) of one row: channel 0, 1, 2 in turn, per channel the statements below in order.
// frow: the parameters (registers), grow: the gradients (LDS); both [N][3] as features_rest keeps them
template <int N>
__device__ __forceinline__ void band_terms(const float* frow, const float* grow, double& sx, double& sy, double& sz) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double f[N], g[N];
#pragma unroll
    for (int k = 0; k < N; k++) f[k] = (double)frow[3 * k + c], g[k] = (double)grow[3 * k + c];
    if constexpr (N == 3) {
      B3GS_POSE_TERM(sx, 1.0, 0, 1);
      B3GS_POSE_TERM(sy, 1.0, 1, 2);
      B3GS_POSE_TERM(sz, 1.0, 0, 2);
    } else if constexpr (N == 5) {
      B3GS_POSE_TERM(sx, 1.0, 0, 3);
      B3GS_POSE_TERM(sx, R3, 1, 2);
      B3GS_POSE_TERM(sx, 1.0, 1, 4);
      B3GS_POSE_TERM(sy, -1.0, 0, 1);
      B3GS_POSE_TERM(sy, R3, 2, 3);
      B3GS_POSE_TERM(sy, 1.0, 3, 4);
      B3GS_POSE_TERM(sz, 2.0, 0, 4);
      B3GS_POSE_TERM(sz, 1.0, 1, 3);
    } else {
      B3GS_POSE_TERM(sx, R6H, 0, 5);
      B3GS_POSE_TERM(sx, R10H, 1, 4);
      B3GS_POSE_TERM(sx, R6H, 1, 6);
      B3GS_POSE_TERM(sx, R6, 2, 3);
      B3GS_POSE_TERM(sx, R10H, 2, 5);
      B3GS_POSE_TERM(sy, -R6H, 0, 1);
      B3GS_POSE_TERM(sy, -R10H, 1, 2);
      B3GS_POSE_TERM(sy, R6, 3, 4);
      B3GS_POSE_TERM(sy, R10H, 4, 5);
      B3GS_POSE_TERM(sy, R6H, 5, 6);
      B3GS_POSE_TERM(sz, 3.0, 0, 6);
      B3GS_POSE_TERM(sz, 2.0, 1, 5);
      B3GS_POSE_TERM(sz, 1.0, 2, 4);
    }
  }
}
#undef B3GS_POSE_TERM

// the chunk's rows [nrows][K] at src -> rows[r * KP + k], coalesced; a row with dead[r] != 0 is not read
// (K words per thread in batches of U: the U loads of a batch are issued before the first of their LDS stores, so that a thread
// has U loads in flight, not one)
template <int K>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int nrows, const uint8_t* dead, float* rows) {
  constexpr int KP = K | 1;
  constexpr int U = K == 9 ? 9 : (K == 24 ? 12 : 15);
  static_assert(K % U == 0, "K words per thread in whole batches");
  const int nwords = nrows * K;
  for (int k0 = 0; k0 < K; k0 += U) {
    float v[U];
    int at[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int w = (k0 + u) * TPB + threadIdx.x;
      const int r = w / K;
      at[u] = (w < nwords && !dead[r]) ? r * KP + (w - r * K) : -1;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (at[u] >= 0) v[u] = src[(k0 + u) * TPB + threadIdx.x];
#pragma unroll
    for (int u = 0; u < U; u++)
      if (at[u] >= 0) rows[at[u]] = v[u];
  }
}

// K: floats of one features_rest row (0, 9, 24, 45 for sh_degree 0..3)
template <int K>
__global__ void __launch_bounds__(TPB) pose_partial_kernel(PoseArgs a) {
  constexpr int KP = K | 1;
  const int v = blockIdx.y;
  const float* __restrict__ gx = a.gx[v];
  const float* __restrict__ gr = a.gr[v];
  const float* __restrict__ gf = a.gf[v];
  const uint8_t* __restrict__ skip = a.skip[v];
  __shared__ float rows[K > 0 ? TPB * KP : 1];
  __shared__ uint8_t dead[TPB];
  double q[NQ];
#pragma unroll
  for (int k = 0; k < NQ; k++) q[k] = 0.0;
  const int64_t P = a.P;
  const int64_t nchunks = (P + TPB - 1) / TPB;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += a.nb) {       // (uniform per workgroup: every thread meets every barrier)
    const int64_t g0 = ch * TPB;
    const int64_t i = g0 + threadIdx.x;
    const bool live = i < P && !(skip && skip[i]);
    float f[K > 0 ? K : 1];
    if constexpr (K > 0) {
      const int64_t left = P - g0;
      const int nrows = (int)(left < TPB ? left : TPB);
      dead[threadIdx.x] = live ? 0 : 1;
      __syncthreads();                                            // (and: the last chunk's reads of `rows` are over)
      stage_rows<K>(a.rest + (size_t)g0 * K, nrows, dead, rows);
      __syncthreads();
      if (live) {
#pragma unroll
        for (int k = 0; k < K; k++) f[k] = rows[threadIdx.x * KP + k];
      }
      __syncthreads();
      stage_rows<K>(gf + (size_t)g0 * K, nrows, dead, rows);
      __syncthreads();
    }
    if (!live) continue;
    const double gmx = (double)gx[3 * i], gmy = (double)gx[3 * i + 1], gmz = (double)gx[3 * i + 2];
    const double dx = (double)a.xyz[3 * i] - a.c[0], dy = (double)a.xyz[3 * i + 1] - a.c[1], dz = (double)a.xyz[3 * i + 2] - a.c[2];
    const double qw = (double)a.rotation[4 * i], qx = (double)a.rotation[4 * i + 1], qy = (double)a.rotation[4 * i + 2],
                 qz = (double)a.rotation[4 * i + 3];
    const double gw = (double)gr[4 * i], gqx = (double)gr[4 * i + 1], gqy = (double)gr[4 * i + 2], gqz = (double)gr[4 * i + 3];
    const double cx = dy * gmz - dz * gmy, cy = dz * gmx - dx * gmz, cz = dx * gmy - dy * gmx;
    // <g_q, e_k (x) q>: e_x (x) q = (-x, w, -z, y), e_y (x) q = (-y, z, w, -x), e_z (x) q = (-z, -y, x, w)
    const double hx = ((gqx * qw - gw * qx) + gqz * qy) - gqy * qz;
    const double hy = ((gqy * qw - gw * qy) + gqx * qz) - gqz * qx;
    const double hz = ((gqz * qw - gw * qz) + gqy * qx) - gqx * qy;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if constexpr (K > 0) {
      const float* grow = rows + threadIdx.x * KP;
      band_terms<3>(f, grow, sx, sy, sz);
      if constexpr (K >= 24) band_terms<5>(f + 9, grow + 9, sx, sy, sz);
      if constexpr (K >= 45) band_terms<7>(f + 24, grow + 24, sx, sy, sz);
    }
    q[0] += (cx + 0.5 * hx) + sx;
    q[1] += (cy + 0.5 * hy) + sy;
    q[2] += (cz + 0.5 * hz) + sz;
    q[3] += gmx;
    q[4] += gmy;
    q[5] += gmz;
  }
  __shared__ double red[TPB / 64][NQ];
  b3gs_block_sum_f64<TPB>(q, red, a.part + ((size_t)v * a.nb + blockIdx.x) * NQ);
}

// one wave per view: fixed assignment of partials to lanes, fixed tree (nb = 0: zeros)
__global__ void __launch_bounds__(64) pose_fold_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  const double* p = part + (size_t)blockIdx.x * nb * NQ;
  for (int k = 0; k < NQ; k++) {
    const double s = b3gs_wave_fold_f64(p + k, nb, NQ);
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * NQ + k] = s;
  }
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_pose_gradient_workspace_bytes(int32_t P, int32_t nviews) {
  if (P < 1 || nviews < 1 || nviews > B3GS_MAX_POSE_VIEWS) return 0;
  return b3gs_align256((size_t)nviews * pose_blocks(P) * NQ * sizeof(double));
}

extern "C" int b3gs_pose_gradient(int32_t P, int32_t sh_degree, int32_t nviews, const float* xyz, const float* rotation,
                                  const float* features_rest, const float* const* grad_xyz, const float* const* grad_rotation,
                                  const float* const* grad_features_rest, const uint8_t* const* skip, const double* pivot, double* out,
                                  void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_pose_gradient";
  if (P < 0) return b3gs_fail(B3GS_ERR_ARG, what, "P >= 0");
  if (sh_degree < 0 || sh_degree > 3) return b3gs_fail(B3GS_ERR_ARG, what, "sh_degree is 0 .. 3");
  if (nviews < 1 || nviews > B3GS_MAX_POSE_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views");
  if (!pivot || !out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  for (int k = 0; k < 3; k++)
    if (!(pivot[k] >= -DBL_MAX && pivot[k] <= DBL_MAX)) return b3gs_fail(B3GS_ERR_ARG, what, "the pivot is finite");
  PoseArgs a = {};
  a.P = P, a.nb = P > 0 ? pose_blocks(P) : 0;
  if (P > 0) {
    if (!xyz || !rotation || !grad_xyz || !grad_rotation || !workspace || (sh_degree > 0 && (!features_rest || !grad_features_rest)))
      return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    for (int v = 0; v < nviews; v++) {
      if (!grad_xyz[v] || !grad_rotation[v] || (sh_degree > 0 && !grad_features_rest[v])) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
      a.gx[v] = grad_xyz[v], a.gr[v] = grad_rotation[v];
      a.gf[v] = sh_degree > 0 ? grad_features_rest[v] : nullptr;
      a.skip[v] = skip ? skip[v] : nullptr;
    }
  }
  a.xyz = xyz, a.rotation = rotation, a.rest = sh_degree > 0 ? features_rest : nullptr;
  for (int k = 0; k < 3; k++) a.c[k] = pivot[k];
  a.part = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  if (P > 0) {
    const dim3 grid(a.nb, nviews), block(TPB);
    switch (sh_degree) {
      case 0: hipLaunchKernelGGL(pose_partial_kernel<0>, grid, block, 0, st, a); break;
      case 1: hipLaunchKernelGGL(pose_partial_kernel<9>, grid, block, 0, st, a); break;
      case 2: hipLaunchKernelGGL(pose_partial_kernel<24>, grid, block, 0, st, a); break;
      default: hipLaunchKernelGGL(pose_partial_kernel<45>, grid, block, 0, st, a); break;
    }
  }
  hipLaunchKernelGGL(pose_fold_kernel, dim3(nviews), dim3(64), 0, st, (const double*)a.part, a.nb, out);
  return b3gs_launch_status(what);
}
