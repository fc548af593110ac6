// Image metrics of held-out views (ABI 11): the per-view sums behind the reference's two evaluation paths
//   train.py:226-261  training_report  clamp(render, 0, 1) vs clamp(gt, 0, 1): mean L1, mean of per-channel PSNRs
//   metrics.py:37-124 over render.py's PNGs: 8-bit round trip of both images, DTU mask composite, masked PSNR, SSIM
// in ONE launch for every view of a batch plus one fixed-order fold.  Every sum is accumulated in fp64; the fold walks
// the per-workgroup partials in index order (no float atomics): two calls on the same inputs return the same bits.
// SSIM is not computed here: the composited pair written to `prepared_*` is what b3gs_ssim_forward(batch = nviews,
// size_average = 0) takes.
#include "b3gs_internal.h"

namespace {

constexpr int MV = 32;             // views per partial-sum launch: the kernel-argument table below
constexpr int MC = 4;              // channels
constexpr int NQ = 2 * MC + 2;     // partial-sum stride of one workgroup (the ABI's row holds 2C + 2 of them)
constexpr int TPB = 256;

struct MetricTable {
  const float* image[MV];
  const float* gt[MV];
  const float* mask[MV];
  float* prep_image[MV];
  float* prep_gt[MV];
  int32_t mask_channels[MV];
};

// ~8 pixels per thread.  (8 views of 800x600, clamp only: 45 us; ~2 pixels per thread measured 55 us, and the fold of four
// times as many partials 20 instead of 7 us)
static int blocks_per_view(int64_t hw) {
  const int64_t b = (hw + 8 * TPB - 1) / (8 * TPB);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

// clamp to [0,1] (torch.clamp: NaN stays NaN), then the round trip of torchvision's save_image + to_tensor:
// uint8(clamp(x*255 + 0.5, 0, 255)) / 255 -- the multiply and the add are two roundings (the library is built with
// -ffp-contract=off), the uint8 cast truncates, the division is the correctly rounded fp32 one
__device__ __forceinline__ float prepare(float x, int mode) {
  if (mode & B3GS_METRIC_CLAMP) x = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
  if (mode & B3GS_METRIC_QUANTIZE) {
    float t = x * 255.f;
    t = t + 0.5f;
    t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
    x = truncf(t) / 255.f;
  }
  return x;
}

// grid (bpv, views of this chunk): workgroup b of view v walks pixels b*256 + tid, stride bpv*256, all channels of a pixel
// in one thread; it leaves NQ partial sums at part[(view0 + v) * bpv + b]
__global__ void __launch_bounds__(TPB) metrics_partial_kernel(MetricTable t, int C, int64_t hw, int mode, int view0, int bpv,
                                                              double* __restrict__ part) {
  const int v = blockIdx.y;
  const float* __restrict__ img = t.image[v];
  const float* __restrict__ gt = t.gt[v];
  const float* __restrict__ mask = t.mask[v];
  float* __restrict__ pimg = t.prep_image[v];
  float* __restrict__ pgt = t.prep_gt[v];
  const int mstride = t.mask_channels[v] == 1 ? 0 : 1;
  double sa[MC], sq[MC], sm = 0.0, cnt = 0.0;
#pragma unroll
  for (int c = 0; c < MC; c++) sa[c] = sq[c] = 0.0;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < hw; p += (int64_t)bpv * TPB) {
#pragma unroll
    for (int c = 0; c < MC; c++) {
      if (c >= C) break;
      const int64_t e = c * hw + p;
      float r = prepare(img[e], mode), g = prepare(gt[e], mode);
      float m = 1.f;
      if (mask) {
        // metrics.py:99-100  render * mask + (1 - mask): two products and a sum, no fused multiply-add
        m = mask[(int64_t)(c * mstride) * hw + p];
        const float om = 1.f - m;
        r = r * m + om;
        g = g * m + om;
      }
      if (pimg) {
        pimg[e] = r;
        pgt[e] = g;
      }
      const float d = r - g;
      const double dd = (double)d;
      sa[c] += fabs(dd);
      sq[c] += dd * dd;
      if (m == 1.f) {             // image_utils.py:20  mask_bin = (mask == 1.)
        sm += dd * dd;
        cnt += 1.0;
      }
    }
  }
  __shared__ double red[TPB / 64][NQ];
  double q[NQ];
#pragma unroll
  for (int c = 0; c < MC; c++) {
    q[c] = sa[c];
    q[MC + c] = sq[c];
  }
  q[2 * MC] = sm;
  q[2 * MC + 1] = cnt;
  b3gs_block_sum_f64<TPB>(q, red, part + ((int64_t)(view0 + v) * bpv + blockIdx.x) * NQ);
}

// one wave per view: fixed assignment of partials to lanes, fixed tree -> out[v, 2C + 2]
__global__ void __launch_bounds__(64) metrics_fold_kernel(const double* __restrict__ part, int C, int bpv,
                                                          double* __restrict__ out) {
  const int v = blockIdx.x;
  const int nq = 2 * C + 2;
  for (int k = 0; k < nq; k++) {
    // output k of the ABI row -> partial slot: Σ|d| channels 0..C-1, Σd² channels 0..C-1, masked Σd², count
    const int slot = k < C ? k : (k < 2 * C ? MC + (k - C) : 2 * MC + (k - 2 * C));
    const double a = b3gs_wave_fold_f64(part + (int64_t)v * bpv * NQ + slot, bpv, NQ);
    if (threadIdx.x == 0) out[(int64_t)v * nq + k] = a;
  }
}

}  // namespace

extern "C" size_t b3gs_image_metrics_workspace_bytes(int32_t nviews, int32_t C, int32_t H, int32_t W) {
  (void)C;
  if (nviews <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)nviews * (size_t)blocks_per_view((int64_t)H * W) * NQ * sizeof(double);
}

extern "C" int b3gs_image_metrics_batch(int32_t nviews, const B3gsMetricView* views, int32_t C, int32_t H, int32_t W,
                                        int32_t mode, double* out, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_image_metrics_batch";
  if (nviews <= 0 || !views || !out || !workspace || H <= 0 || W <= 0)
    return b3gs_fail(B3GS_ERR_ARG, what, "no views, NULL pointer or empty shape");
  if (C < 1 || C > MC) return b3gs_fail(B3GS_ERR_ARG, what, "1..4 channels");
  if (mode & ~(B3GS_METRIC_CLAMP | B3GS_METRIC_QUANTIZE)) return b3gs_fail(B3GS_ERR_ARG, what, "unknown mode bits");
  for (int i = 0; i < nviews; i++) {
    const B3gsMetricView& v = views[i];
    if (!v.image || !v.gt) return b3gs_fail(B3GS_ERR_ARG, what, "a view without image or gt");
    if (v.mask && v.mask_channels != 1 && v.mask_channels != C)
      return b3gs_fail(B3GS_ERR_ARG, what, "mask_channels must be 1 or C");
    if (!v.prepared_image != !v.prepared_gt)
      return b3gs_fail(B3GS_ERR_ARG, what, "prepared_image and prepared_gt are both set or both NULL");
  }
  const int64_t hw = (int64_t)H * W;
  const int bpv = blocks_per_view(hw);
  double* part = static_cast<double*>(workspace);
  for (int v0 = 0; v0 < nviews; v0 += MV) {
    const int n = nviews - v0 < MV ? nviews - v0 : MV;
    MetricTable t = {};
    for (int k = 0; k < n; k++) {
      const B3gsMetricView& v = views[v0 + k];
      t.image[k] = v.image;
      t.gt[k] = v.gt;
      t.mask[k] = v.mask;
      t.mask_channels[k] = v.mask ? v.mask_channels : 1;
      t.prep_image[k] = v.prepared_image;
      t.prep_gt[k] = v.prepared_gt;
    }
    hipLaunchKernelGGL(metrics_partial_kernel, dim3(bpv, n), dim3(TPB), 0, (hipStream_t)stream, t, (int)C, hw, (int)mode, v0, bpv,
                       part);
  }
  hipLaunchKernelGGL(metrics_fold_kernel, dim3(nviews), dim3(64), 0, (hipStream_t)stream, (const double*)part, (int)C, bpv, out);
  return b3gs_launch_status(what);
}
