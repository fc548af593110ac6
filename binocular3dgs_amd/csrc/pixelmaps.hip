// Per-pixel geometry maps (added to ABI 18): a second walk of the tile lists a finished forward left on the device, which
// reduces per PIXEL what contrib.hip reduces per Gaussian.  Five planes of H*W words per view, up to 8 views per launch:
//
//   median_depth  record depth of the last blended entry whose transmittance T BEFORE the blend was > 0.5: the entry at which T
//                 crosses one half, or the last blended entry when it never does; 0 when nothing was blended.  A copy of the
//                 record's float, no arithmetic.
//   depth_m1      sum of w d  in list order, w = alpha * T: fmaf(d, w, acc), the forward's own statement of its depth image
//   depth_m2      sum of w d d in list order: fmaf(w * d, d, acc)
//   dominant      Gaussian index of the largest w, ties to the first in list order (the rule of contrib.hip); -1: nothing blended
//   count         number of blended entries
//
// The walk is the forward's (render.hip) and contrib.hip's: one 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant,
// the list staged 256 entries at a time through LDS by the same stage_chunk() -- same quadrant cull -- and every entry evaluated
// with the same blend_power() / clamp, so an entry is blended here exactly where the forward blended it.  The saturation stop is
// not evaluated again: a pixel walks the positions below its n_contrib, which already ends in front of the stopping entry.
//
// Every pixel owns its five words: no atomics, no reduction across lanes, nothing read back.  A pixel's result depends on its
// own list and records alone, so it is the same bits whatever else is in the launch.  Every pixel inside the image is written
// (a NULL plane is skipped), so the planes need no zeroing.
#include "blend_common.h"
#include <cstring>

namespace {

constexpr int PIXMAP_CHUNK = 256;

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
  __shared__ TileShared<PIXMAP_CHUNK> sh;
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(pb.b, bid);
  PixelMapOut out = pb.out[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < pb.b.n && bid >= pb.b.v[k].block_base) out = pb.out[k];
  const int W = bv.W, H = bv.H, grid_x = bv.grid_x, ntiles = bv.ntiles;
  const int tile = tile_of_block(bid - bv.block_base, ntiles);
  if (tile >= ntiles) return;
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int px = tile_x * B3GS_TILE + (int)((w & 1) * 8 + (lane & 7));
  const int py = tile_y * B3GS_TILE + (int)((w >> 1) * 8 + (lane >> 3));
  const float fpx = (float)px, fpy = (float)py;
  const bool inside = px < W && py < H;
  const size_t pix = inside ? (size_t)py * W + px : 0;
  const TileList tl = tile_list(bv, tile, true);
  // positions this pixel walks: below its n_contrib, never past the list; none for a pixel outside the image
  const uint32_t nc = inside ? min(bv.n_contrib[pix], tl.total) : 0u;
  uint32_t wave_nc = nc;   // the quadrant's deepest position
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_nc = max(wave_nc, (uint32_t)__shfl_xor((int)wave_nc, d, 64));
  wave_nc = __builtin_amdgcn_readfirstlane(wave_nc);

  float T = 1.0f, m1 = 0.0f, m2 = 0.0f, median = 0.0f;
  float best_w = -1.0f;      // largest weight so far at this pixel (-1: nothing blended yet) and whose it is
  int32_t best_g = -1, count = 0;
  for (uint32_t c0 = 0u;; c0 += (uint32_t)PIXMAP_CHUNK) {
    if (!__syncthreads_or(nc > c0)) break;   // (also the barrier between the last read of a chunk and the next staging)
    stage_chunk(sh, tl, bv.idx_mask, bv.rec, c0, (float)(tile_x * B3GS_TILE), (float)(tile_y * B3GS_TILE));
    __syncthreads();
    if (wave_nc <= c0) continue;
#pragma unroll 1
    for (int pw = 0; pw < PIXMAP_CHUNK / 64; pw++) {
      if (c0 + (uint32_t)(pw * 64) >= wave_nc) break;
      u64 m = uniform_u64(sh.mask[w][pw]);
      while (m) {
        const int g = pw * 64 + __builtin_ctzll(m);
        m &= m - 1ull;
        const uint32_t pos = c0 + (uint32_t)g;
        if (pos >= wave_nc) break;   // (the bits come in rising order)
        const float4 A = sh.A[g];
        const float2 B = *reinterpret_cast<const float2*>(&sh.B[g]);   // cyy, opacity
        const float dx = A.x - fpx, dy = A.y - fpy;
        const float power = blend_power(A, B.x, dx, dy);
        const float alpha = fminf(B3GS_ALPHA_MAX, B.y * __expf(power));
        const bool live = pos < nc && !(power > 0.0f) && !(alpha < B3GS_ALPHA_MIN);
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
        const float4 Cc = sh.C[g];   // b, depth, Gaussian index (bits), -
        const float depth = Cc.y;
        const float wgt = alpha * T;
        const bool better = live && wgt > best_w;
        median = (live && T > 0.5f) ? depth : median;      // T in front of this entry
        m1 = live ? __builtin_fmaf(depth, wgt, m1) : m1;
        m2 = live ? __builtin_fmaf(wgt * depth, depth, m2) : m2;
        best_g = better ? (int32_t)__float_as_uint(Cc.z) : best_g;
        best_w = better ? wgt : best_w;
        count += live ? 1 : 0;
        T = live ? T * (1.0f - alpha) : T;
      }
    }
  }
  if (inside) {
    if (out.median) out.median[pix] = median;
    if (out.m1) out.m1[pix] = m1;
    if (out.m2) out.m2[pix] = m2;
    if (out.dominant) out.dominant[pix] = best_g;
    if (out.count) out.count[pix] = count;
  }
}

}  // namespace

extern "C" int b3gs_blend_pixel_maps_batch(int32_t nviews, const B3gsPixelMapView* views, b3gs_stream_t stream) {
  static const char* what = "b3gs_blend_pixel_maps_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (!views) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table");
  for (int k = 0; k < nviews; k++) {
    const B3gsPixelMapView& v = views[k];
    if (!v.view) return b3gs_fail(B3GS_ERR_ARG, what, "a view without its B3gsScene");
    if (!v.geometry || !v.binning || !v.image) return b3gs_fail(B3GS_ERR_ARG, what, "NULL state buffer in a view");
    if (v.view->W <= 0 || v.view->H <= 0) return b3gs_fail(B3GS_ERR_ARG, what, "W/H must be positive");
    if (v.view->P < 0 || v.view->P != views[0].view->P)
      return b3gs_fail(B3GS_ERR_ARG, what, "the views of one call share P (they are views of one model)");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  PixelMapBatch pb;
  memset(&pb, 0, sizeof(pb));
  pb.b.n = nviews;
  int total = 0;
  for (int k = 0; k < nviews; k++) {
    const B3gsPixelMapView& v = views[k];
    GeomView g;
    ImgView im;
    BinView b;
    b3gs_geom_view(const_cast<char*>(v.geometry), P, &g);
    b3gs_img_view(const_cast<char*>(v.image), v.view->W, v.view->H, &im);
    b3gs_bin_view(const_cast<char*>(v.binning), P, 1, &b);   // the tile lists sit at offset 0 whatever the capacity
    pb.b.v[k] = b3gs_blend_view(*v.view, g, b, im);
    pb.b.v[k].round = 2;       // every tile over segment 1 + segment 2
    pb.b.v[k].block_base = total;
    total += blocks_of(pb.b.v[k]);
    pb.out[k] = PixelMapOut{v.median_depth, v.depth_m1, v.depth_m2, v.dominant, v.count};
  }
  hipLaunchKernelGGL(pixel_maps_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, pb);
  return b3gs_launch_status(what);
}
