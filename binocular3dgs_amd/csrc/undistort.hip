// Undistorting a COLMAP dataset (added to ABI 18; binocular3dgs_amd/undistort.py): seven camera models with lens distortion, the
// map from an output pinhole into the distorted source, and the integer bilinear resampling of up to 8 uint8 images through it.
//
// distort(): ONE fixed sequence of fp64 operations per model (no FMA: the library is built with -ffp-contract=off; every
//   product and sum below is its own rounding, in the order written).  The four polynomial models use +, -, * and, FULL_OPENCV
//   only, one IEEE division: tests/undistort_ref.py restates them in numpy float64 in the same order and gets the same bits.
//   The three fisheye models add sqrt, atan and a division by r.
// Newton inverse (b3gs_camera_points, undistort direction): at most NEWTON_ITERS = 50 iterations from the distorted point;
//   the 2x2 Jacobian from forward differences with h = 1e-6 * max(1, |coordinate|); a point has converged when the squared
//   step du^2 + dv^2 is below NEWTON_STEP2 = 1e-22 (a step of 1e-11 in normalised units).  An iterate whose Jacobian has no
//   positive determinant and trace (it has left the branch of the distortion that contains the optical axis: the point lies
//   behind the fold-over), or a non-finite system, ends the iteration.  An unconverged point comes back as it went in, with
//   converged = 0.
// Launches: one per call, one thread per point / map entry / quad of output pixels; nothing reads the device, no atomics.
#include "b3gs_internal.h"

#include <string.h>

namespace {

constexpr int TPB = 256;
constexpr int NEWTON_ITERS = 50;
constexpr double NEWTON_STEP2 = 1e-22;
constexpr double NEWTON_H = 1e-6;
constexpr double FISHEYE_EPS = 1e-8;
constexpr int32_t MAP_LIMIT = 1 << 30;
// remap: a workgroup is RTX x RTY threads, a thread 4 output pixels of one row: a tile of 64 x 16 output pixels, whose taps
// fall into about as many source rows (16 rows of 64 C bytes: whole cache lines per row at C = 3, 4)
constexpr int RTX = 16, RTY = 16;

// COLMAP's model ids
enum { M_SIMPLE_RADIAL = 2, M_RADIAL = 3, M_OPENCV = 4, M_OPENCV_FISHEYE = 5, M_FULL_OPENCV = 6, M_SIMPLE_RADIAL_FISHEYE = 8,
       M_RADIAL_FISHEYE = 9 };

struct Cam {
  int32_t model;
  double fx, fy, cx, cy;
  double k[8];           // the coefficients behind the focal lengths and the principal point, in COLMAP's order
};

// ---- the camera models -------------------------------------------------------------------------------------------------------
// (the operation order of every line is part of the contract: tests/undistort_ref.py::distort repeats it)
__device__ __forceinline__ void distort(const Cam& c, double u, double v, double* ou, double* ov) {
  const double u2 = u * u, v2 = v * v;
  const double r2 = u2 + v2;
  switch (c.model) {
    case M_SIMPLE_RADIAL: {
      const double rad = c.k[0] * r2;
      *ou = u + u * rad;
      *ov = v + v * rad;
      return;
    }
    case M_RADIAL: {
      const double rad = c.k[0] * r2 + c.k[1] * (r2 * r2);
      *ou = u + u * rad;
      *ov = v + v * rad;
      return;
    }
    case M_OPENCV: {
      const double rad = c.k[0] * r2 + c.k[1] * (r2 * r2);
      const double uv = u * v;
      const double tu = (2.0 * c.k[2]) * uv + c.k[3] * (r2 + 2.0 * u2);
      const double tv = (2.0 * c.k[3]) * uv + c.k[2] * (r2 + 2.0 * v2);
      *ou = (u + u * rad) + tu;
      *ov = (v + v * rad) + tv;
      return;
    }
    case M_FULL_OPENCV: {
      const double r4 = r2 * r2, r6 = r4 * r2;
      const double num = ((1.0 + c.k[0] * r2) + c.k[1] * r4) + c.k[4] * r6;
      const double den = ((1.0 + c.k[5] * r2) + c.k[6] * r4) + c.k[7] * r6;
      const double rad = num / den;
      const double uv = u * v;
      const double tu = (2.0 * c.k[2]) * uv + c.k[3] * (r2 + 2.0 * u2);
      const double tv = (2.0 * c.k[3]) * uv + c.k[2] * (r2 + 2.0 * v2);
      *ou = u * rad + tu;
      *ov = v * rad + tv;
      return;
    }
    case M_OPENCV_FISHEYE: {
      const double r = sqrt(r2);
      if (r < FISHEYE_EPS) break;
      const double th = atan(r);
      const double t2 = th * th, t4 = t2 * t2;
      const double t6 = t4 * t2, t8 = t4 * t4;
      const double thd = th * ((((1.0 + c.k[0] * t2) + c.k[1] * t4) + c.k[2] * t6) + c.k[3] * t8);
      const double s = thd / r;
      *ou = u * s;
      *ov = v * s;
      return;
    }
    case M_SIMPLE_RADIAL_FISHEYE:
    case M_RADIAL_FISHEYE: {
      const double r = sqrt(r2);
      if (r < FISHEYE_EPS) break;
      const double th = atan(r);
      const double s = th / r;
      const double uu = u * s, vv = v * s;
      const double t2 = th * th;
      double rad = c.k[0] * t2;
      if (c.model == M_RADIAL_FISHEYE) rad = rad + c.k[1] * (t2 * t2);
      *ou = uu + uu * rad;
      *ov = vv + vv * rad;
      return;
    }
    default:
      break;
  }
  *ou = u;
  *ov = v;
}

// the normalised point whose distortion is (ud, vd) -> true when the iteration converged (else *ou, *ov are not written)
__device__ __forceinline__ bool undistort(const Cam& c, double ud, double vd, double* ou, double* ov) {
  double u = ud, v = vd;
  for (int it = 0; it < NEWTON_ITERS; it++) {
    const double hu = NEWTON_H * fmax(1.0, fabs(u)), hv = NEWTON_H * fmax(1.0, fabs(v));
    double f0u, f0v, f1u, f1v, f2u, f2v;
    distort(c, u, v, &f0u, &f0v);
    distort(c, u + hu, v, &f1u, &f1v);
    distort(c, u, v + hv, &f2u, &f2v);
    const double j00 = (f1u - f0u) / hu, j10 = (f1v - f0v) / hu;
    const double j01 = (f2u - f0u) / hv, j11 = (f2v - f0v) / hv;
    const double ru = f0u - ud, rv = f0v - vd;
    const double det = j00 * j11 - j01 * j10;
    // off the principal branch (behind the fold-over of the distortion, where a second, mirrored solution lives), singular,
    // infinite or NaN
    if (!(det > 1e-300) || !(det < 1e300) || !(j00 + j11 > 0.0)) return false;
    const double du = (j11 * ru - j01 * rv) / det;
    const double dv = (j00 * rv - j10 * ru) / det;
    const double s2 = du * du + dv * dv;
    if (!(s2 < 1e300)) return false;                                      // infinite or NaN
    u = u - du;
    v = v - dv;
    if (s2 < NEWTON_STEP2) {
      *ou = u;
      *ov = v;
      return true;
    }
  }
  return false;
}

// ---- b3gs_camera_points -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) camera_points_kernel(Cam c, int inverse, int64_t n, const double* __restrict__ xy,
                                                            double* __restrict__ out, uint8_t* __restrict__ converged) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const double x = xy[2 * i], y = xy[2 * i + 1];
  const double u = (x - c.cx) / c.fx, v = (y - c.cy) / c.fy;
  double ou = u, ov = v;
  bool ok = true;
  if (inverse) ok = undistort(c, u, v, &ou, &ov);
  else distort(c, u, v, &ou, &ov);
  out[2 * i] = ok ? c.fx * ou + c.cx : x;
  out[2 * i + 1] = ok ? c.fy * ov + c.cy : y;
  if (converged) converged[i] = ok ? 1 : 0;
}

// ---- b3gs_undistort_map -------------------------------------------------------------------------------------------------------
// a source coordinate (pixel centres at integers) as 24.8 fixed point
__device__ __forceinline__ int32_t to_fixed(double x) {
  const double t = floor(x * 256.0 + 0.5);
  if (!(fabs(t) <= 1.7976931348623157e308)) return -MAP_LIMIT;           // NaN, +-Inf
  return (int32_t)fmin(fmax(t, -(double)MAP_LIMIT), (double)MAP_LIMIT);
}

__global__ void __launch_bounds__(TPB) undistort_map_kernel(Cam c, int W, int H, double fxo, double fyo, double cxo, double cyo,
                                                            int2* __restrict__ map) {
  const int i = blockIdx.x * TPB + threadIdx.x, j = blockIdx.y;
  if (i >= W || j >= H) return;
  const double u = (((double)i + 0.5) - cxo) / fxo, v = (((double)j + 0.5) - cyo) / fyo;
  double du, dv;
  distort(c, u, v, &du, &dv);
  const double x = (c.fx * du + c.cx) - 0.5, y = (c.fy * dv + c.cy) - 0.5;
  map[(size_t)j * W + i] = make_int2(to_fixed(x), to_fixed(y));
}

// ---- b3gs_remap_batch ---------------------------------------------------------------------------------------------------------
struct RemapTable {
  const uint8_t* src[B3GS_MAX_REMAP_VIEWS];
  uint8_t* out[B3GS_MAX_REMAP_VIEWS];
};

// Pixel `idx` of a [.., C] byte image of `total` bytes as one word (channel c in byte c).  C = 3 is ONE unaligned 4-byte load
// that starts at the pixel (the last pixel of the image: one byte earlier, shifted), not three byte loads; the bytes read
// always lie inside the image.
template <int C>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ src, size_t idx, size_t total) {
  if (C == 1) return src[idx];
  if (C == 4) return reinterpret_cast<const uint32_t*>(src)[idx];
  const size_t o = idx * 3;
  uint32_t w;
  if (o + 4 <= total) {
    memcpy(&w, src + o, 4);
    return w;
  }
  if (total >= 4) {
    memcpy(&w, src + o - 1, 4);
    return w >> 8;
  }
  return (uint32_t)src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16);   // a 1 x 1 image
}

// grid (ceil(W / 64), ceil(H / 16), views); block (RTX, RTY)
template <int C>
__device__ __forceinline__ void remap_body(const RemapTable& t, int Hs, int Ws, const int2* __restrict__ map, int H, int W,
                                           uint8_t* __restrict__ valid) {
  const int x = (blockIdx.x * RTX + threadIdx.x) * 4, y = blockIdx.y * RTY + threadIdx.y;
  if (x >= W || y >= H) return;
  const int nv = min(4, W - x);
  const int view = blockIdx.z;
  const uint8_t* __restrict__ src = t.src[view];
  const size_t total = (size_t)Hs * Ws * C;
  const size_t at = (size_t)y * W + x;
  uint8_t px[4 * C];
  uint8_t ok[4];
#pragma unroll
  for (int p = 0; p < 4; p++) {
#pragma unroll
    for (int ch = 0; ch < C; ch++) px[p * C + ch] = 0;
    ok[p] = 0;
    if (p >= nv) continue;
    const int2 m = map[at + p];
    const bool inside = m.x >= -128 && (int64_t)m.x < (int64_t)256 * Ws - 128 && m.y >= -128 && (int64_t)m.y < (int64_t)256 * Hs - 128;
    if (!inside) continue;
    ok[p] = 255;
    const int x0 = m.x >> 8, y0 = m.y >> 8;                             // floor: >> of a negative int is arithmetic
    const uint32_t ax = (uint32_t)(m.x & 255), ay = (uint32_t)(m.y & 255);
    const int xa = min(max(x0, 0), Ws - 1), xb = min(max(x0 + 1, 0), Ws - 1);
    const int ya = min(max(y0, 0), Hs - 1), yb = min(max(y0 + 1, 0), Hs - 1);
    const uint32_t p00 = load_pixel<C>(src, (size_t)ya * Ws + xa, total), p01 = load_pixel<C>(src, (size_t)ya * Ws + xb, total);
    const uint32_t p10 = load_pixel<C>(src, (size_t)yb * Ws + xa, total), p11 = load_pixel<C>(src, (size_t)yb * Ws + xb, total);
    const uint32_t w00 = (256u - ax) * (256u - ay), w01 = ax * (256u - ay), w10 = (256u - ax) * ay, w11 = ax * ay;
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
      const int sh = 8 * ch;
      const uint32_t s = w00 * ((p00 >> sh) & 255u) + w01 * ((p01 >> sh) & 255u) + w10 * ((p10 >> sh) & 255u) + w11 * ((p11 >> sh) & 255u);
      px[p * C + ch] = (uint8_t)((s + 32768u) >> 16);
    }
  }
  uint8_t* __restrict__ o = t.out[view] + at * C;
  if (nv == 4) memcpy(o, px, 4 * C);                                   // (rows of any length: the store need not be aligned)
  else
    for (int b = 0; b < nv * C; b++) o[b] = px[b];
  if (view == 0) {
    if (nv == 4) memcpy(valid + at, ok, 4);
    else
      for (int p = 0; p < nv; p++) valid[at + p] = ok[p];
  }
}

__global__ void __launch_bounds__(RTX * RTY) remap_kernel(RemapTable t, int Hs, int Ws, int C, const int2* __restrict__ map, int H,
                                                          int W, uint8_t* __restrict__ valid) {
  if (C == 1) remap_body<1>(t, Hs, Ws, map, H, W, valid);
  else if (C == 3) remap_body<3>(t, Hs, Ws, map, H, W, valid);
  else remap_body<4>(t, Hs, Ws, map, H, W, valid);
}

static int param_count(int32_t model) {
  switch (model) {
    case M_SIMPLE_RADIAL: case M_SIMPLE_RADIAL_FISHEYE: return 4;
    case M_RADIAL: case M_RADIAL_FISHEYE: return 5;
    case M_OPENCV: case M_OPENCV_FISHEYE: return 8;
    case M_FULL_OPENCV: return 12;
    default: return 0;
  }
}

static int make_cam(const B3gsCameraModel* cam, Cam* c, const char* what) {
  if (!cam) return b3gs_fail(B3GS_ERR_ARG, what, "a camera is needed");
  const int n = param_count(cam->model);
  if (n == 0)
    return b3gs_fail(B3GS_ERR_ARG, what, "unsupported camera model (SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE, FULL_OPENCV, "
                                         "SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE are supported)");
  if (cam->n_params != n) return b3gs_fail(B3GS_ERR_ARG, what, "wrong parameter count for the camera model");
  if (cam->width <= 0 || cam->height <= 0) return b3gs_fail(B3GS_ERR_ARG, what, "the camera's image size is at least 1 x 1");
  const double* p = cam->params;
  *c = Cam{};
  c->model = cam->model;
  const bool one_focal = n == 4 || n == 5;
  c->fx = p[0];
  c->fy = one_focal ? p[0] : p[1];
  c->cx = one_focal ? p[1] : p[2];
  c->cy = one_focal ? p[2] : p[3];
  const int first = one_focal ? 3 : 4;
  for (int i = first; i < n; i++) c->k[i - first] = p[i];
  for (int i = 0; i < n; i++)
    if (!__builtin_isfinite(p[i])) return b3gs_fail(B3GS_ERR_ARG, what, "camera parameters must be finite");
  if (!(c->fx > 0.0) || !(c->fy > 0.0)) return b3gs_fail(B3GS_ERR_ARG, what, "focal lengths must be positive");
  return B3GS_OK;
}

}  // namespace

extern "C" int b3gs_camera_points(const B3gsCameraModel* cam, int32_t inverse, int64_t n, const double* xy, double* out,
                                  uint8_t* converged, b3gs_stream_t stream) {
  static const char* what = "b3gs_camera_points";
  Cam c;
  const int rc = make_cam(cam, &c, what);
  if (rc != B3GS_OK) return rc;
  if (n < 0 || n > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "0 .. 2^31 - 1 points per call");
  if (n == 0) return B3GS_OK;
  if (!xy || !out) return b3gs_fail(B3GS_ERR_ARG, what, "xy and out are needed");
  if (inverse && !converged) return b3gs_fail(B3GS_ERR_ARG, what, "the undistort direction needs the converged bytes");
  hipLaunchKernelGGL(camera_points_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, c, inverse ? 1 : 0, n,
                     xy, out, converged);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_undistort_map(const B3gsCameraModel* cam, int32_t W, int32_t H, double fx, double fy, int32_t* map,
                                  b3gs_stream_t stream) {
  static const char* what = "b3gs_undistort_map";
  Cam c;
  const int rc = make_cam(cam, &c, what);
  if (rc != B3GS_OK) return rc;
  if (W <= 0 || H <= 0 || H > 65535 || (int64_t)W * H > ((int64_t)1 << 28))
    return b3gs_fail(B3GS_ERR_ARG, what, "the output is at least 1 x 1, at most 65535 rows and 2^28 pixels");
  if (!(fx > 0.0) || !(fy > 0.0) || !__builtin_isfinite(fx) || !__builtin_isfinite(fy))
    return b3gs_fail(B3GS_ERR_ARG, what, "the output focal lengths must be positive");
  if (!map || ((uintptr_t)map & 7)) return b3gs_fail(B3GS_ERR_ARG, what, "an 8-byte aligned map is needed");
  hipLaunchKernelGGL(undistort_map_kernel, dim3((W + TPB - 1) / TPB, H), dim3(TPB), 0, (hipStream_t)stream, c, W, H, fx, fy,
                     (double)W * 0.5, (double)H * 0.5, reinterpret_cast<int2*>(map));
  return b3gs_launch_status(what);
}

extern "C" int b3gs_remap_batch(int32_t nviews, const uint8_t* const* src, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map,
                                int32_t H, int32_t W, uint8_t* const* out, uint8_t* valid, b3gs_stream_t stream) {
  static const char* what = "b3gs_remap_batch";
  if (nviews <= 0 || nviews > B3GS_MAX_REMAP_VIEWS || !src || !out) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views are needed");
  if (C != 1 && C != 3 && C != 4) return b3gs_fail(B3GS_ERR_ARG, what, "a source is [Hs, Ws, C] with C in {1, 3, 4}");
  if (Hs <= 0 || Ws <= 0 || Hs > (1 << 20) || Ws > (1 << 20) || (int64_t)Hs * Ws > ((int64_t)1 << 28))
    return b3gs_fail(B3GS_ERR_ARG, what, "a source is at least 1 x 1, at most 2^20 along an axis and 2^28 pixels");
  if (W <= 0 || H <= 0 || (int64_t)W * H > ((int64_t)1 << 28))
    return b3gs_fail(B3GS_ERR_ARG, what, "the output is at least 1 x 1 and at most 2^28 pixels");
  if ((H + RTY - 1) / RTY > 65535) return b3gs_fail(B3GS_ERR_ARG, what, "at most 65535 * 16 output rows");
  if (!map || ((uintptr_t)map & 7) || !valid) return b3gs_fail(B3GS_ERR_ARG, what, "an 8-byte aligned map and the valid plane are needed");
  RemapTable t = {};
  for (int i = 0; i < nviews; i++) {
    if (!src[i] || !out[i]) return b3gs_fail(B3GS_ERR_ARG, what, "src and out are needed for every view");
    if ((uintptr_t)src[i] & 3) return b3gs_fail(B3GS_ERR_ARG, what, "src must be 4-byte aligned");
    t.src[i] = src[i];
    t.out[i] = out[i];
  }
  const int quads = (W + 3) / 4;
  hipLaunchKernelGGL(remap_kernel, dim3((quads + RTX - 1) / RTX, (H + RTY - 1) / RTY, nviews), dim3(RTX, RTY), 0, (hipStream_t)stream, t,
                     Hs, Ws, C, reinterpret_cast<const int2*>(map), H, W, valid);
  return b3gs_launch_status(what);
}
