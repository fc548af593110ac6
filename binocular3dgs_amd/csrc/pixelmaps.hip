// Per-pixel geometry maps (added to ABI 18): a second walk of the tile lists a finished forward left on the device
// (tile_walk.h), which reduces per PIXEL what contrib.hip reduces per Gaussian.  Five planes of H*W words per view, up to 8
// views per launch:
//
//   median_depth  record depth of the last blended entry whose transmittance T BEFORE the blend was > 0.5: the entry at which T
//                 crosses one half, or the last blended entry when it never does; 0 when nothing was blended.  A copy of the
//                 record's float, no arithmetic.
//   depth_m1      sum of w d  in list order, w = alpha * T: fmaf(d, w, acc), the forward's own statement of its depth image
//   depth_m2      sum of w d d in list order: fmaf(w * d, d, acc)
//   dominant      Gaussian index of the largest w, ties to the first in list order (the rule of contrib.hip); -1: nothing blended
//   count         number of blended entries
//
// Every pixel owns its five words: no atomics, no reduction across lanes, nothing read back.  A pixel's result depends on its
// own list and records alone, so it is the same bits whatever else is in the launch.  Every pixel inside the image is written
// (a NULL plane is skipped), so the planes need no zeroing.
#include "tile_walk.h"

namespace {

struct PixelMapOut {
  float* median;
  float* m1;
  float* m2;
  int32_t* dominant;
  int32_t* count;
};

struct PixelMapBatch {
  BlendBatch b;
  PixelMapOut out[B3GS_MAX_FUSED_VIEWS];
};

__global__ void __launch_bounds__(256) pixel_maps_kernel(PixelMapBatch pb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(pb.b, bid);
  PixelMapOut out;
  select_of_view(pb.b, pb.out, bid, out);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const uint32_t nc = wp.inside ? min(bv.n_contrib[wp.pix], wp.tl.total) : 0u;
  const uint32_t wave_nc = wave_deepest(nc);

  float T = 1.0f, m1 = 0.0f, m2 = 0.0f, median = 0.0f;
  float best_w = -1.0f;      // largest weight so far at this pixel (-1: nothing blended yet) and whose it is
  int32_t best_g = -1, count = 0;
  WalkNoHook none;
  auto on_entry = [&](int g, uint32_t, bool live, u64, float wgt, float, float T_before) {
    const float4 Cc = sh.C[g];   // b, depth, Gaussian index (bits), -
    const float depth = Cc.y;
    const bool better = live && wgt > best_w;
    median = (live && T_before > 0.5f) ? depth : median;
    m1 = live ? __builtin_fmaf(depth, wgt, m1) : m1;
    m2 = live ? __builtin_fmaf(wgt * depth, depth, m2) : m2;
    best_g = better ? (int32_t)__float_as_uint(Cc.z) : best_g;
    best_w = better ? wgt : best_w;
    count += live ? 1 : 0;
  };
  walk_tile(sh, wp, bv, nc, wave_nc, T, none, on_entry, none);
  if (wp.inside) {
    if (out.median) out.median[wp.pix] = median;
    if (out.m1) out.m1[wp.pix] = m1;
    if (out.m2) out.m2[wp.pix] = m2;
    if (out.dominant) out.dominant[wp.pix] = best_g;
    if (out.count) out.count[wp.pix] = count;
  }
}

}  // namespace

extern "C" int b3gs_blend_pixel_maps_batch(int32_t nviews, const B3gsPixelMapView* views, b3gs_stream_t stream) {
  static const char* what = "b3gs_blend_pixel_maps_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (!views) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table");
  for (int k = 0; k < nviews; k++)
    if (const char* bad = check_state(views[k], views[0])) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  PixelMapBatch pb;
  memset(&pb, 0, sizeof(pb));
  const int total = fill_blend_batch(pb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) {
    const B3gsPixelMapView& v = views[k];
    pb.out[k] = PixelMapOut{v.median_depth, v.depth_m1, v.depth_m2, v.dominant, v.count};
  }
  hipLaunchKernelGGL(pixel_maps_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, pb);
  return b3gs_launch_status(what);
}
