// Feature fields (added to ABI 18): the general continuous pair of reductions of the second walk of a finished forward's tile
// lists (tile_walk.h), next to contrib.hip (the adjoint for one indicator channel), segment.hip (the adjoint for up to 16
// indicator channels; the forward for one-hot features) and pixelmaps.hip.
//
//   b3gs_feature_render_batch   per pixel and channel c: the float32 sum, in list order, of w f[g][c] over the blended entries,
//                               acc = fmaf(f, w, acc) -- the operation, operand order and list order of the forward's colour
//                               accumulation (render.hip), so three channels holding a view's record colours give the bits of
//                               its colour planes over a zero background.  No background term.
//   b3gs_feature_lift_batch     the adjoint: per Gaussian and channel the sum over the blended (view, pixel, entry) of
//                               w Fn[pixel][c], Fn = clamp(F / scale[c], -1, 1), as 64-bit integers of rint(w Fn 2^32).
//
// Channels go in groups of FEAT_GROUP = 8: one workgroup = one (tile, channel group), blockIdx.y the group.  A ragged last group
// has a wave-uniform channel count nch < 8; its registers above nch hold zeros and every loop over the group is unrolled over
// constant indices (no dynamic register index, no scratch).
//
// Render.  At staging thread i loads the group's floats of entry i's Gaussian into LDS next to the staged record; per blended
// entry every lane reads them (one address: a broadcast) and does its 8 fused multiply-adds.  Every pixel owns its words: no
// atomics, no reduction across lanes.
//
// Lift.  Only integer adds reach memory, so the bits do not depend on the order of waves, tiles, views, batches or calls.  A
// walking pixel divides its 8 channel values by scale[c] once (IEEE division) and clamps them to [-1, 1]; per blended entry
// p = w * Fn is one float32 rounding and |p| <= 0.99, so |p| 2^32 is exact and rint makes it an integer m < 2^32; s = +-m is a
// 33-bit signed integer.  The 16 lanes of a DPP row add s as two halves, as contrib.hip does: the low 16 bits unsigned and the
// arithmetically shifted high part signed (two's complement 32-bit adds, sums below 2^21: no carry leaves a lane); one lane
// per row adds hi * 2^16 + lo onto slot [channel][entry] of a per-workgroup LDS accumulator; after a staged chunk, thread i
// flushes entry i (column i of the accumulator: no bank conflict): ONE 64-bit integer global atomic per (tile, list entry,
// channel) that received something.  For Fn = 1 the integer is exactly the q of contrib.hip.  Channel group 0 also sums
// contrib.hip's weight_q32 if it is wanted.
#include "tile_walk.h"

namespace {

constexpr int FEAT_GROUP = 8;

struct FeatRenderBatch {
  BlendBatch b;
  float* out[B3GS_MAX_FUSED_VIEWS];
  const float* feat;   // [P, C]
  uint32_t P, C;
};

struct FeatLiftView {
  const float* maps;
  const uint8_t* mask;
};

struct FeatLiftBatch {
  BlendBatch b;
  FeatLiftView in[B3GS_MAX_FUSED_VIEWS];
  long long* sums;     // [P, C]
  u64* weight;         // [P] or NULL
  uint32_t P, C;
  float scale[B3GS_MAX_FEATURE_CHANNELS];   // by value: the table is host memory and the call reads nothing back
};
static_assert(sizeof(FeatLiftBatch) <= 4096, "the kernel arguments of the lift hold the scale table");

__global__ void __launch_bounds__(256) feature_render_kernel(FeatRenderBatch fb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  __shared__ float4 fe[2][WALK_CHUNK];   // the group's 8 floats of the staged Gaussian: thread i writes column i
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(fb.b, bid);
  float* out;
  select_of_view(fb.b, fb.out, bid, out);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const uint32_t c0 = blockIdx.y * (uint32_t)FEAT_GROUP;
  const uint32_t nch = min((uint32_t)FEAT_GROUP, fb.C - c0);   // wave-uniform (the grid has no group at or behind C)
  const uint32_t nc = wp.inside ? min(bv.n_contrib[wp.pix], wp.tl.total) : 0u;
  const uint32_t wave_nc = wave_deepest(nc);

  float T = 1.0f;
  float acc[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; j++) acc[j] = 0.0f;
  auto on_stage = [&](int id, uint32_t) {
    float f[FEAT_GROUP];
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; j++) f[j] = 0.0f;
    if (id >= 0 && (uint32_t)id < fb.P) {
      const float* row = fb.feat + (size_t)id * fb.C + c0;
#pragma unroll
      for (int j = 0; j < FEAT_GROUP; j++)
        if ((uint32_t)j < nch) f[j] = row[j];
    }
    fe[0][threadIdx.x] = make_float4(f[0], f[1], f[2], f[3]);
    fe[1][threadIdx.x] = make_float4(f[4], f[5], f[6], f[7]);
  };
  auto on_entry = [&](int g, uint32_t, bool, u64, float wgt, float, float) {
    const float4 a = fe[0][g], b = fe[1][g];
    acc[0] = __builtin_fmaf(a.x, wgt, acc[0]);
    acc[1] = __builtin_fmaf(a.y, wgt, acc[1]);
    acc[2] = __builtin_fmaf(a.z, wgt, acc[2]);
    acc[3] = __builtin_fmaf(a.w, wgt, acc[3]);
    acc[4] = __builtin_fmaf(b.x, wgt, acc[4]);
    acc[5] = __builtin_fmaf(b.y, wgt, acc[5]);
    acc[6] = __builtin_fmaf(b.z, wgt, acc[6]);
    acc[7] = __builtin_fmaf(b.w, wgt, acc[7]);
  };
  WalkNoHook none;
  walk_tile(sh, wp, bv, nc, wave_nc, T, on_stage, on_entry, none);
  if (wp.inside) {
    const size_t hw = (size_t)bv.H * bv.W;
    float* o = out + (size_t)c0 * hw + wp.pix;
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; j++)
      if ((uint32_t)j < nch) o[(size_t)j * hw] = acc[j];
  }
}

__global__ void __launch_bounds__(256) feature_lift_kernel(FeatLiftBatch fb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  __shared__ long long acc[FEAT_GROUP][WALK_CHUNK];   // [channel][chunk entry]: thread i zeroes and flushes column i
  __shared__ u64 acc_w[WALK_CHUNK];
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(fb.b, bid);
  FeatLiftView in;
  select_of_view(fb.b, fb.in, bid, in);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const unsigned tid = threadIdx.x, lane = tid & 63;
  const uint32_t c0 = blockIdx.y * (uint32_t)FEAT_GROUP;
  const uint32_t nch = min((uint32_t)FEAT_GROUP, fb.C - c0);   // wave-uniform
  const bool with_w = blockIdx.y == 0 && fb.weight != nullptr;
  // a pixel outside the image or masked out walks nothing
  uint32_t nc = 0u;
  if (wp.inside && (!in.mask || in.mask[wp.pix])) nc = min(bv.n_contrib[wp.pix], wp.tl.total);
  const uint32_t wave_nc = wave_deepest(nc);
  float Fn[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; j++) {
    Fn[j] = 0.0f;
    if ((uint32_t)j < nch) {
      const float sc = fb.scale[c0 + (uint32_t)j];
      if (nc) {
        const size_t hw = (size_t)bv.H * bv.W;
        Fn[j] = fminf(1.0f, fmaxf(-1.0f, in.maps[(size_t)(c0 + (uint32_t)j) * hw + wp.pix] / sc));
      }
    }
  }

  float T = 1.0f;
  auto on_stage = [&](int, uint32_t) {
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; j++) acc[j][tid] = 0ll;
    acc_w[tid] = 0ull;
  };
  auto on_entry = [&](int g, uint32_t, bool, u64, float wgt, float, float) {
    const bool row_lane = (lane & 15u) == 0u;
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; j++) {
      if ((uint32_t)j >= nch) continue;
      // |p| <= 0.99: the product with 2^32 is exact and below 2^32; s = +-m as its low 16 bits and floor(s / 2^16)
      const float p = wgt * Fn[j];
      const uint32_t m = (uint32_t)rintf(fabsf(p) * 4294967296.0f);
      const bool neg = p < 0.0f;
      const uint32_t lo = (neg ? 0u - m : m) & 0xFFFFu;
      const int32_t hi = neg ? -(int32_t)((m + 0xFFFFu) >> 16) : (int32_t)(m >> 16);
      const uint32_t slo = row_sum_u32(lo);
      const int32_t shi = (int32_t)row_sum_u32((uint32_t)hi);
      if (row_lane && (slo | (uint32_t)shi)) atomicAdd(reinterpret_cast<u64*>(&acc[j][g]), (u64)((long long)shi * 65536ll + (long long)slo));
    }
    if (with_w) {
      const uint32_t q = (uint32_t)rintf(wgt * 4294967296.0f);
      const uint32_t lo = row_sum_u32(q & 0xFFFFu), hi = row_sum_u32(q >> 16);
      if (row_lane && (lo | hi)) atomicAdd(&acc_w[g], (u64)lo + ((u64)hi << 16));
    }
  };
  auto on_chunk_end = [&](uint32_t) {
    // (a slot is nonzero only where an entry was staged: the cull mask has no bit beyond the list)
    const uint32_t gid = __float_as_uint(sh.C[tid].z);
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; j++) {
      if ((uint32_t)j >= nch) continue;
      const long long v = acc[j][tid];
      if (v && gid < fb.P) atomicAdd(reinterpret_cast<u64*>(fb.sums + (size_t)gid * fb.C + c0 + (uint32_t)j), (u64)v);
    }
    if (with_w) {
      const u64 v = acc_w[tid];
      if (v && gid < fb.P) atomicAdd(fb.weight + gid, v);
    }
  };
  walk_tile(sh, wp, bv, nc, wave_nc, T, on_stage, on_entry, on_chunk_end);
}

const char* check_channels(int32_t C) {
  return (C < 1 || C > B3GS_MAX_FEATURE_CHANNELS) ? "1..256 channels" : nullptr;
}

}  // namespace

extern "C" int b3gs_feature_render_batch(int32_t nviews, const B3gsFeatureRenderView* views, int32_t C, const float* gaussian_features,
                                         b3gs_stream_t stream) {
  static const char* what = "b3gs_feature_render_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (const char* bad = check_channels(C)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  if (!views || !gaussian_features) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table or Gaussian feature array");
  for (int k = 0; k < nviews; k++) {
    if (const char* bad = check_state(views[k], views[0])) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (!views[k].out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output planes in a view");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  FeatRenderBatch fb;
  memset(&fb, 0, sizeof(fb));
  fb.P = (uint32_t)P;
  fb.C = (uint32_t)C;
  fb.feat = gaussian_features;
  const int total = fill_blend_batch(fb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) fb.out[k] = views[k].out;
  const dim3 grid(total, (C + FEAT_GROUP - 1) / FEAT_GROUP);
  hipLaunchKernelGGL(feature_render_kernel, grid, dim3(256), 0, (hipStream_t)stream, fb);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_feature_lift_batch(int32_t nviews, const B3gsFeatureLiftView* views, int32_t C, const float* scale,
                                       int64_t* sums_q32, uint64_t* weight_q32, b3gs_stream_t stream) {
  static const char* what = "b3gs_feature_lift_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (const char* bad = check_channels(C)) return b3gs_fail(B3GS_ERR_ARG, what, bad);
  if (!views || !scale || !sums_q32) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table, scale table or sums array");
  for (int c = 0; c < C; c++)
    if (!(scale[c] > 0.0f) || !(scale[c] <= 3.4028234663852886e38f))
      return b3gs_fail(B3GS_ERR_ARG, what, "every scale is a finite number > 0");
  for (int k = 0; k < nviews; k++) {
    if (const char* bad = check_state(views[k], views[0])) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (!views[k].maps) return b3gs_fail(B3GS_ERR_ARG, what, "NULL feature maps in a view");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  FeatLiftBatch fb;
  memset(&fb, 0, sizeof(fb));
  fb.P = (uint32_t)P;
  fb.C = (uint32_t)C;
  fb.sums = reinterpret_cast<long long*>(sums_q32);
  fb.weight = reinterpret_cast<u64*>(weight_q32);
  for (int c = 0; c < B3GS_MAX_FEATURE_CHANNELS; c++) fb.scale[c] = c < C ? scale[c] : 1.0f;
  const int total = fill_blend_batch(fb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) fb.in[k] = FeatLiftView{views[k].maps, views[k].pixel_mask};
  const dim3 grid(total, (C + FEAT_GROUP - 1) / FEAT_GROUP);
  hipLaunchKernelGGL(feature_lift_kernel, grid, dim3(256), 0, (hipStream_t)stream, fb);
  return b3gs_launch_status(what);
}
