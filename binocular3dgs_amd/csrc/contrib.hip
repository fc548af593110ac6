// Per-Gaussian render contribution (added to ABI 18): a second walk of the tile lists a finished forward left on the device
// (tile_walk.h), which attributes every blend weight w = alpha * T to the Gaussian it belongs to.  Four statistics per
// Gaussian, summed over the counted pixels of up to 8 views per launch: sum of w (as an integer: rint(w * 2^32)), number of
// pixels it was blended into, largest w, number of pixels where it holds the largest w.
//
// Everything that reaches memory is an integer: the weight goes through one conversion (w * 2^32 is exact in float32, rint
// makes it an integer below 2^32) and is added in 64 bits, the counts are integer adds, the maximum is an unsigned max of
// float bits (w >= 0).  Integer adds and max commute, so the result does not depend on the order of anything -- waves, tiles,
// views of a batch, launches.
//
// Reduction before memory: the 16 lanes of a DPP row add their integers (two 16-bit halves, so that no carry leaves a lane)
// and take their max in four row operations each; one lane per row adds the row's three figures onto the entry's slot of a
// per-workgroup LDS accumulator; after a staged chunk, thread i flushes slot i: ONE set of three global atomics per (tile,
// list entry) that was blended anywhere in the tile, issued 64 entries per wave instruction.
#include "tile_walk.h"

namespace {

struct ContribBatch {
  BlendBatch b;
  const uint8_t* mask[B3GS_MAX_FUSED_VIEWS];
  uint32_t P;
  B3gsContribOut out;
};

__global__ void __launch_bounds__(256) contrib_kernel(ContribBatch cb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  __shared__ u64 acc_w[WALK_CHUNK];
  __shared__ uint32_t acc_h[WALK_CHUNK], acc_m[WALK_CHUNK];
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(cb.b, bid);
  const uint8_t* mask;
  select_of_view(cb.b, cb.mask, bid, mask);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const unsigned tid = threadIdx.x, lane = tid & 63;
  // a pixel outside the image or masked out walks nothing
  uint32_t nc = 0u;
  if (wp.inside && (!mask || mask[wp.pix])) nc = min(bv.n_contrib[wp.pix], wp.tl.total);
  const uint32_t wave_nc = wave_deepest(nc);

  float T = 1.0f;
  float best_w = -1.0f;      // largest weight so far at this pixel (-1: nothing blended yet) and whose it is
  uint32_t best_g = 0u;
  auto on_stage = [&](int, uint32_t) {
    acc_w[tid] = 0ull;
    acc_h[tid] = 0u;
    acc_m[tid] = 0u;
  };
  auto on_entry = [&](int g, uint32_t, bool live, u64 bal, float wgt, float, float) {
    const bool better = live && wgt > best_w;
    best_g = better ? __float_as_uint(sh.C[g].z) : best_g;
    best_w = better ? wgt : best_w;
    // wgt <= 0.99: the product is exact and below 2^32
    const uint32_t q = (uint32_t)rintf(wgt * 4294967296.0f);
    const uint32_t lo = row_sum_u32(q & 0xFFFFu), hi = row_sum_u32(q >> 16);
    const uint32_t mx = row_max_u32(__float_as_uint(wgt));
    if ((lane & 15u) == 0u) {
      const uint32_t n = (uint32_t)__builtin_popcount((uint32_t)(bal >> (lane & 48u)) & 0xFFFFu);
      if (n) {
        atomicAdd(&acc_w[g], (u64)lo + ((u64)hi << 16));
        atomicAdd(&acc_h[g], n);
        atomicMax(&acc_m[g], mx);
      }
    }
  };
  auto on_chunk_end = [&](uint32_t) {
    const uint32_t n = acc_h[tid];
    if (n) {
      const uint32_t gid = __float_as_uint(sh.C[tid].z);
      if (gid < cb.P) {
        atomicAdd(cb.out.weight_q32 + gid, acc_w[tid]);
        atomicAdd(cb.out.hits + gid, n);
        atomicMax(cb.out.wmax_bits + gid, acc_m[tid]);
      }
    }
  };
  walk_tile(sh, wp, bv, nc, wave_nc, T, on_stage, on_entry, on_chunk_end);
  if (best_w >= 0.0f && best_g < cb.P) atomicAdd(cb.out.dominant + best_g, 1u);
}

}  // namespace

extern "C" int b3gs_blend_contribution_batch(int32_t nviews, const B3gsContribView* views, const B3gsContribOut* out,
                                             b3gs_stream_t stream) {
  static const char* what = "b3gs_blend_contribution_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (!views || !out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table or output table");
  if (!out->weight_q32 || !out->hits || !out->wmax_bits || !out->dominant)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL output array");
  for (int k = 0; k < nviews; k++)
    if (const char* bad = check_state(views[k], views[0], "the views of one call share P (the output arrays are [P])"))
      return b3gs_fail(B3GS_ERR_ARG, what, bad);
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  ContribBatch cb;
  memset(&cb, 0, sizeof(cb));
  cb.P = (uint32_t)P;
  cb.out = *out;
  const int total = fill_blend_batch(cb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) cb.mask[k] = views[k].pixel_mask;
  hipLaunchKernelGGL(contrib_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, cb);
  return b3gs_launch_status(what);
}
