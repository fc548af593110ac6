// Editing a trained model (added to ABI 18; binocular3dgs_amd/edit.py).
// include/b3gs_raster.h states the arithmetic; tests/edit_ref.py restates it in numpy float64.  Everything below is fp64 in one
// fixed operation order with ONE rounding to float32 at the store (the library is built with -ffp-contract=off: a product and
// the sum that takes it are two roundings, as in numpy), a float32 compare, or integer work: every output is one fixed result.
//   transform   points: thread = point.  Gaussians: workgroup = 256 consecutive Gaussians.  xyz / rotation / scaling are 12- and
//               16-byte rows a wave reads as one contiguous run.  features_rest is a 36 / 96 / 180-byte row per Gaussian: read
//               by thread = Gaussian, the 64 lanes of one load sit in 64 different rows.  So the workgroup's rows -- ONE contiguous
//               block of 256 K floats -- are staged through LDS: lane i loads word i of the block (256 contiguous bytes per wave
//               instruction), thread = Gaussian then reads its row from LDS (row stride K | 1 words: 9, 25 or 45, odd, so the
//               32 lanes of a ds_read_b32 group sit on 32 banks), rotates it in
//               fp64 with the matrices in the kernel arguments (uniform: scalar loads), writes the row back to LDS, and the
//               block is stored as it was loaded.  A workgroup reads all of its rows before it writes one and owns them: in place
//               is allowed.  No atomics, no reduction.
//   select      thread = Gaussian; the enabled tests are uniform branches, a disabled test reads nothing
//   sums        grid-stride partials of 18 doubles per workgroup (b3gs_block_sum_f64), folded in index order by one wave
#include "b3gs_internal.h"
#include <cfloat>

namespace {

constexpr int TPB = 256;
constexpr int SUMS_Q = 18;            // n, sum a (3), sum b (3), sum |a|^2, sum b a^T (9), sum |b|^2
constexpr int CAM_WORDS = 19;         // 3x4 world-to-view, fx fy cx cy W H near

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

struct Xf { B3gsSimilarity s; };      // by value in the kernel arguments (808 bytes)

__device__ __forceinline__ void xf_point(const B3gsSimilarity& T, double x, double y, double z, float* o) {
#pragma unroll
  for (int i = 0; i < 3; i++) o[i] = (float)(T.s * ((T.R[3 * i] * x + T.R[3 * i + 1] * y) + T.R[3 * i + 2] * z) + T.t[i]);
}

__global__ void __launch_bounds__(TPB) transform_points_kernel(int64_t n, const float* in, Xf xf, float* out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
  float o[3];
  xf_point(xf.s, x, y, z, o);
  out[3 * i] = o[0], out[3 * i + 1] = o[1], out[3 * i + 2] = o[2];
}

// one band of one colour channel: o[m] = sum_k D[m][k] f[k], k ascending, from the first product
template <int N>
__device__ __forceinline__ void rotate_band(const double* D, float* row) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    double f[N], o[N];
#pragma unroll
    for (int k = 0; k < N; k++) f[k] = (double)row[3 * k + c];
#pragma unroll
    for (int m = 0; m < N; m++) {
      double acc = D[m * N] * f[0];
#pragma unroll
      for (int k = 1; k < N; k++) acc = acc + D[m * N + k] * f[k];
      o[m] = acc;
    }
#pragma unroll
    for (int m = 0; m < N; m++) row[3 * m + c] = (float)o[m];
  }
}

// K: floats of one features_rest row (0, 9, 24, 45 for sh_degree 0..3)
template <int K>
__global__ void __launch_bounds__(TPB) transform_gaussians_kernel(int32_t P, const float* xyz, const float* rotation, const float* scaling,
                                                                  const float* rest, Xf xf, float* out_xyz, float* out_rotation,
                                                                  float* out_scaling, float* out_rest) {
  const B3gsSimilarity& T = xf.s;
  const int64_t g0 = (int64_t)blockIdx.x * TPB;
  const int64_t i = g0 + threadIdx.x;
  const bool live = i < P;
  if (live) {
    float o[3];
    xf_point(T, (double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], o);
    const double rw = rotation[4 * i], rx = rotation[4 * i + 1], ry = rotation[4 * i + 2], rz = rotation[4 * i + 3];
    const double qw = T.q[0], qx = T.q[1], qy = T.q[2], qz = T.q[3];
    const float w4[4] = {(float)(((qw * rw - qx * rx) - qy * ry) - qz * rz), (float)(((qw * rx + qx * rw) + qy * rz) - qz * ry),
                         (float)(((qw * ry - qx * rz) + qy * rw) + qz * rx), (float)(((qw * rz + qx * ry) - qy * rx) + qz * rw)};
    float sc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) sc[k] = (float)((double)scaling[3 * i + k] + T.ln_s);
#pragma unroll
    for (int k = 0; k < 3; k++) out_xyz[3 * i + k] = o[k], out_scaling[3 * i + k] = sc[k];
#pragma unroll
    for (int k = 0; k < 4; k++) out_rotation[4 * i + k] = w4[k];
  }
  if constexpr (K > 0) {
    constexpr int KP = K | 1;                               // the LDS row stride: odd
    __shared__ float rows[TPB * KP];
    const int64_t left = (int64_t)P - g0;
    const int nrows = (int)(left < TPB ? left : TPB);       // >= 1: the grid holds ceil(P / TPB) workgroups
    const int nwords = nrows * K;
    const float* src = rest + (size_t)g0 * K;
    for (int w = threadIdx.x; w < nwords; w += TPB) rows[(w / K) * KP + w % K] = src[w];
    __syncthreads();
    if (live) {
      float* row = rows + threadIdx.x * KP;
      rotate_band<3>(T.D1, row);
      if constexpr (K >= 24) rotate_band<5>(T.D2, row + 9);
      if constexpr (K >= 45) rotate_band<7>(T.D3, row + 24);
    }
    __syncthreads();
    float* dst = out_rest + (size_t)g0 * K;
    for (int w = threadIdx.x; w < nwords; w += TPB) dst[w] = rows[(w / K) * KP + w % K];
  }
}

// ---- selection ---------------------------------------------------------------------------------------------------------
struct SelectArgs {
  int32_t P, flags, nviews, min_views, mask_h, mask_w;
  const float *xyz, *opacity, *scaling;
  double box[12], half[3], centre[3], r2;
  float logit_min, log_max_scale;
  const double* cams;                 // [nviews][CAM_WORDS]
  const uint8_t* masks;               // [nviews][mask_h][mask_w] or NULL
  uint8_t* keep;
  int32_t* seen;
};

__global__ void __launch_bounds__(TPB) select_kernel(SelectArgs a) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= a.P) return;
  bool keep = true;
  int32_t seen = 0;
  if (a.flags & (B3GS_SELECT_BOX | B3GS_SELECT_SPHERE | B3GS_SELECT_VIEWS)) {
    const float fx = a.xyz[3 * i], fy = a.xyz[3 * i + 1], fz = a.xyz[3 * i + 2];
    const bool finite = fabsf(fx) <= FLT_MAX && fabsf(fy) <= FLT_MAX && fabsf(fz) <= FLT_MAX;
    const double x = fx, y = fy, z = fz;
    if (a.flags & B3GS_SELECT_BOX) {
      bool in = finite;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double p = ((a.box[4 * k] * x + a.box[4 * k + 1] * y) + a.box[4 * k + 2] * z) + a.box[4 * k + 3];
        in = in && fabs(p) <= a.half[k];
      }
      keep = keep && in;
    }
    if (a.flags & B3GS_SELECT_SPHERE) {
      const double dx = x - a.centre[0], dy = y - a.centre[1], dz = z - a.centre[2];
      keep = keep && finite && (dx * dx + dy * dy) + dz * dz <= a.r2;
    }
    if (a.flags & B3GS_SELECT_VIEWS) {
      for (int v = 0; finite && v < a.nviews; v++) {
        const double* c = a.cams + (size_t)v * CAM_WORDS;
        const double X = ((c[0] * x + c[1] * y) + c[2] * z) + c[3], Y = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
        const double Z = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
        if (!(Z > c[18])) continue;
        const double pu = (c[12] * X) / Z + c[14], pv = (c[13] * Y) / Z + c[15];
        if (!(pu >= 0.0 && pu < c[16] && pv >= 0.0 && pv < c[17])) continue;
        if (a.masks) {
          const int64_t iu = (int64_t)floor(pu), iv = (int64_t)floor(pv);
          if (iu >= a.mask_w || iv >= a.mask_h) continue;           // (never outside the plane, whatever W and H the camera states)
          if (!a.masks[((size_t)v * a.mask_h + (size_t)iv) * a.mask_w + (size_t)iu]) continue;
        }
        seen++;
      }
      keep = keep && seen >= a.min_views;
    }
  }
  if (a.flags & B3GS_SELECT_OPACITY) keep = keep && a.opacity[i] >= a.logit_min;
  if (a.flags & B3GS_SELECT_SCALE) {
    const float m = fmaxf(fmaxf(a.scaling[3 * i], a.scaling[3 * i + 1]), a.scaling[3 * i + 2]);
    keep = keep && m <= a.log_max_scale;
  }
  a.keep[i] = keep ? 1 : 0;
  a.seen[i] = seen;
}

// ---- the sums of a similarity fit --------------------------------------------------------------------------------------
static int sums_blocks(int64_t n) {
  const int64_t b = (n + 8 * TPB - 1) / (8 * TPB);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

struct SumsArgs {
  int64_t N, Nb;
  const float *a, *b, *dist;
  const int32_t* index;
  const uint8_t* mask;
  float gate;
  double oa[3], ob[3];
  int nb;
  double* part;
};

__global__ void __launch_bounds__(TPB) sums_partial_kernel(SumsArgs s) {
  double q[SUMS_Q];
#pragma unroll
  for (int k = 0; k < SUMS_Q; k++) q[k] = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < s.N; i += (int64_t)s.nb * TPB) {
    const int32_t j = s.index[i];
    if (j < 0 || j >= s.Nb) continue;
    if (!(s.dist[i] <= s.gate)) continue;
    if (s.mask && !s.mask[i]) continue;
    double a[3], b[3];
#pragma unroll
    for (int k = 0; k < 3; k++) a[k] = (double)s.a[3 * i + k] - s.oa[k], b[k] = (double)s.b[3 * (size_t)j + k] - s.ob[k];
    q[0] += 1.0;
#pragma unroll
    for (int k = 0; k < 3; k++) q[1 + k] += a[k], q[4 + k] += b[k];
    q[7] += (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) q[8 + 3 * r + c] += b[r] * a[c];
    q[17] += (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
  }
  __shared__ double red[TPB / 64][SUMS_Q];
  b3gs_block_sum_f64<TPB>(q, red, s.part + (size_t)blockIdx.x * SUMS_Q);
}

// one wave: fixed assignment of partials to lanes, fixed tree
__global__ void __launch_bounds__(64) sums_fold_kernel(const double* __restrict__ part, int nb, double* __restrict__ out) {
  for (int k = 0; k < SUMS_Q; k++) {
    const double v = b3gs_wave_fold_f64(part + k, nb, SUMS_Q);
    if (threadIdx.x == 0) out[k] = v;
  }
}

static bool finite_all(const double* v, int n) {
  for (int k = 0; k < n; k++)
    if (!(v[k] >= -DBL_MAX && v[k] <= DBL_MAX)) return false;
  return true;
}
static bool similarity_ok(const B3gsSimilarity* T) {
  return T && finite_all(T->R, 9) && finite_all(T->t, 3) && finite_all(&T->s, 1) && finite_all(&T->ln_s, 1) && finite_all(T->q, 4) &&
         finite_all(T->D1, 9) && finite_all(T->D2, 25) && finite_all(T->D3, 49) && T->s > 0.0;
}

}  // namespace

// ---- C ABI -------------------------------------------------------------------------------------------------------------
extern "C" int b3gs_transform_points(int64_t N, const float* in, const B3gsSimilarity* xf, float* out, b3gs_stream_t stream) {
  static const char* what = "b3gs_transform_points";
  if (N < 0 || N > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 <= N <= 2^31 - 1");
  if (!similarity_ok(xf)) return b3gs_fail(B3GS_ERR_ARG, what, "the similarity is finite with s > 0");
  if (N == 0) return B3GS_OK;
  if (!in || !out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  Xf x;
  x.s = *xf;
  hipLaunchKernelGGL(transform_points_kernel, dim3(blocks_of(N)), dim3(TPB), 0, (hipStream_t)stream, N, in, x, out);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_transform_gaussians(int32_t P, int32_t sh_degree, const float* xyz, const float* rotation, const float* scaling,
                                        const float* features_rest, const B3gsSimilarity* xf, float* out_xyz, float* out_rotation,
                                        float* out_scaling, float* out_features_rest, b3gs_stream_t stream) {
  static const char* what = "b3gs_transform_gaussians";
  if (P < 0) return b3gs_fail(B3GS_ERR_ARG, what, "P >= 0");
  if (sh_degree < 0 || sh_degree > 3) return b3gs_fail(B3GS_ERR_ARG, what, "sh_degree is 0 .. 3");
  if (!similarity_ok(xf)) return b3gs_fail(B3GS_ERR_ARG, what, "the similarity is finite with s > 0");
  if (P == 0) return B3GS_OK;
  if (!xyz || !rotation || !scaling || !out_xyz || !out_rotation || !out_scaling || (sh_degree > 0 && (!features_rest || !out_features_rest)))
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  Xf x;
  x.s = *xf;
  const dim3 grid(blocks_of(P)), block(TPB);
  hipStream_t s = (hipStream_t)stream;
#define B3GS_EDIT_LAUNCH(K)                                                                                                         \
  hipLaunchKernelGGL(transform_gaussians_kernel<K>, grid, block, 0, s, P, xyz, rotation, scaling, features_rest, x, out_xyz, out_rotation, \
                     out_scaling, out_features_rest)
  switch (sh_degree) {
    case 0: B3GS_EDIT_LAUNCH(0); break;
    case 1: B3GS_EDIT_LAUNCH(9); break;
    case 2: B3GS_EDIT_LAUNCH(24); break;
    default: B3GS_EDIT_LAUNCH(45); break;
  }
#undef B3GS_EDIT_LAUNCH
  return b3gs_launch_status(what);
}

extern "C" int b3gs_select_gaussians(int32_t P, const float* xyz, const float* opacity_raw, const float* scaling_raw, const B3gsSelect* sel,
                                     uint8_t* keep, int32_t* seen, b3gs_stream_t stream) {
  static const char* what = "b3gs_select_gaussians";
  if (P < 0) return b3gs_fail(B3GS_ERR_ARG, what, "P >= 0");
  if (!sel) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  const int32_t f = sel->flags;
  if (f & ~(B3GS_SELECT_BOX | B3GS_SELECT_SPHERE | B3GS_SELECT_OPACITY | B3GS_SELECT_SCALE | B3GS_SELECT_VIEWS))
    return b3gs_fail(B3GS_ERR_ARG, what, "unknown test");
  if ((f & B3GS_SELECT_BOX) && (!finite_all(sel->box, 12) || !finite_all(sel->half, 3)))
    return b3gs_fail(B3GS_ERR_ARG, what, "the box is finite");
  if ((f & B3GS_SELECT_SPHERE) && (!finite_all(sel->centre, 3) || !finite_all(&sel->r2, 1)))
    return b3gs_fail(B3GS_ERR_ARG, what, "the sphere is finite");
  if ((f & B3GS_SELECT_OPACITY) && sel->logit_min != sel->logit_min) return b3gs_fail(B3GS_ERR_ARG, what, "logit_min is NaN");
  if ((f & B3GS_SELECT_SCALE) && sel->log_max_scale != sel->log_max_scale) return b3gs_fail(B3GS_ERR_ARG, what, "log_max_scale is NaN");
  if (f & B3GS_SELECT_VIEWS) {
    if (sel->nviews < 1 || sel->nviews > B3GS_MAX_SELECT_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 64 views");
    if (!sel->cameras) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
    if (sel->masks && (sel->mask_h < 1 || sel->mask_w < 1)) return b3gs_fail(B3GS_ERR_ARG, what, "the mask planes are at least 1 x 1");
  }
  if (P == 0) return B3GS_OK;
  if (!keep || !seen) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if ((f & (B3GS_SELECT_BOX | B3GS_SELECT_SPHERE | B3GS_SELECT_VIEWS)) && !xyz) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (((f & B3GS_SELECT_OPACITY) && !opacity_raw) || ((f & B3GS_SELECT_SCALE) && !scaling_raw))
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  SelectArgs a = {};
  a.P = P, a.flags = f, a.nviews = sel->nviews, a.min_views = sel->min_views, a.mask_h = sel->mask_h, a.mask_w = sel->mask_w;
  a.xyz = xyz, a.opacity = opacity_raw, a.scaling = scaling_raw;
  for (int k = 0; k < 12; k++) a.box[k] = sel->box[k];
  for (int k = 0; k < 3; k++) a.half[k] = sel->half[k], a.centre[k] = sel->centre[k];
  a.r2 = sel->r2, a.logit_min = sel->logit_min, a.log_max_scale = sel->log_max_scale;
  a.cams = sel->cameras, a.masks = (f & B3GS_SELECT_VIEWS) ? sel->masks : nullptr;
  a.keep = keep, a.seen = seen;
  hipLaunchKernelGGL(select_kernel, dim3(blocks_of(P)), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_similarity_sums_workspace_bytes(int64_t N) {
  if (N < 1 || N > INT32_MAX) return 0;
  return b3gs_align256((size_t)sums_blocks(N) * SUMS_Q * sizeof(double));
}

extern "C" int b3gs_similarity_sums(int64_t N, const float* a, int64_t Nb, const float* b, const int32_t* index, const float* dist, float gate,
                                    const uint8_t* mask, const double* origin_a, const double* origin_b, double* out, void* workspace,
                                    b3gs_stream_t stream) {
  static const char* what = "b3gs_similarity_sums";
  if (N < 1 || N > INT32_MAX || Nb < 1 || Nb > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 2^31 - 1 points in each cloud");
  if (gate != gate) return b3gs_fail(B3GS_ERR_ARG, what, "gate is NaN");
  if (!a || !b || !index || !dist || !origin_a || !origin_b || !out || !workspace) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!finite_all(origin_a, 3) || !finite_all(origin_b, 3)) return b3gs_fail(B3GS_ERR_ARG, what, "the origins are finite");
  SumsArgs s = {};
  s.N = N, s.Nb = Nb, s.a = a, s.b = b, s.dist = dist, s.index = index, s.mask = mask, s.gate = gate;
  for (int k = 0; k < 3; k++) s.oa[k] = origin_a[k], s.ob[k] = origin_b[k];
  s.nb = sums_blocks(N);
  s.part = static_cast<double*>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sums_partial_kernel, dim3(s.nb), dim3(TPB), 0, st, s);
  hipLaunchKernelGGL(sums_fold_kernel, dim3(1), dim3(64), 0, st, (const double*)s.part, s.nb, out);
  return b3gs_launch_status(what);
}
