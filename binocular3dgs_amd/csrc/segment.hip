// Segmentation from 2D label planes (added to ABI 18): two more reductions of the second walk of a finished forward's tile
// lists (tile_walk.h), next to contrib.hip (per Gaussian) and pixelmaps.hip (per pixel).
//
//   b3gs_label_votes_batch    per Gaussian and per label l: the sum of rint(w * 2^32), w = alpha * T, over the blended (view,
//                             pixel, entry) of the Gaussian at pixels whose label byte is l.  What contrib.hip sums under the
//                             pixel mask (labels == l), for every l in ONE walk.
//   b3gs_label_render_batch   per pixel and per label l: S_l = the float32 sum, in list order, of w over the blended entries
//                             whose Gaussian carries label l; the pixel gets the smallest l of the largest S_l > 0, and that S_l.
//
// Votes.  Only integer adds reach memory (w * 2^32 is exact in float32, rint makes it an integer below 2^32, 64-bit adds), so
// the bits do not depend on the order of waves, tiles, views or calls.  A lane's label never changes during the walk: every wave
// forms the set of labels among its walking pixels once, a 16-bit wave-uniform mask (most quadrants hold one label), and per
// blended entry loops over that set only; inside, q is masked to the lanes of the label and the 16 lanes of a DPP row add
// their integers (two 16-bit halves, so that no carry leaves a lane), as contrib.hip does; one lane per row adds the row's sum
// onto slot [label][entry] of a per-workgroup LDS accumulator; after a staged chunk, thread i flushes entry i: ONE global
// 64-bit atomic per (tile, list entry, label) that received anything.  Only the labels present in the workgroup are zeroed and
// flushed.
//
// Label render.  Every pixel owns its two words: no atomics, no reduction across lanes.  The label of an entry's Gaussian is
// staged next to its record and is wave-uniform at every step of the walk, so the NL running sums stay in registers without
// dynamic indexing: S_l = fmaf(w, (label == l) ? 1 : 0, S_l) for every l below NL -- the product with 1 is exact, the fma is
// the float32 add S_l + w; with 0 it leaves S_l as it is (S_l >= 0, w >= 0).  NL is nlabels rounded up to 2, 4, 8 or 16.
#include "tile_walk.h"

namespace {

constexpr uint32_t NO_LABEL = 255u;

struct VoteBatch {
  BlendBatch b;
  const uint8_t* labels[B3GS_MAX_FUSED_VIEWS];
  uint32_t P, nlabels;
  u64* votes;
};

struct LabelOut {
  uint8_t* label;
  float* weight;
};

struct LabelRenderBatch {
  BlendBatch b;
  LabelOut out[B3GS_MAX_FUSED_VIEWS];
  const uint8_t* gaussian_label;
  uint32_t P, nlabels;
};

__global__ void __launch_bounds__(256) label_votes_kernel(VoteBatch vb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  __shared__ u64 acc[B3GS_MAX_LABELS][WALK_CHUNK];   // [label][chunk entry]: thread i zeroes and flushes column i, no bank conflict
  __shared__ uint32_t wg_labels;
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(vb.b, bid);
  const uint8_t* labels;
  select_of_view(vb.b, vb.labels, bid, labels);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const unsigned tid = threadIdx.x, lane = tid & 63;
  // a pixel outside the image or without a label walks nothing
  uint32_t nc = 0u, lab = NO_LABEL;
  if (wp.inside) {
    lab = labels[wp.pix];
    if (lab < vb.nlabels) nc = min(bv.n_contrib[wp.pix], wp.tl.total);
  }
  const uint32_t wave_nc = wave_deepest(nc);
  uint32_t wave_labels = nc ? (1u << (lab & 15u)) : 0u;   // the labels of the quadrant's walking pixels (nc > 0: lab < 16)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_labels |= (uint32_t)__shfl_xor((int)wave_labels, d, 64);
  wave_labels = __builtin_amdgcn_readfirstlane(wave_labels);
  if (tid == 0) wg_labels = 0u;
  __syncthreads();
  if (lane == 0 && wave_labels) atomicOr(&wg_labels, wave_labels);
  __syncthreads();
  const uint32_t tile_labels = __builtin_amdgcn_readfirstlane(wg_labels);

  float T = 1.0f;
  auto on_stage = [&](int, uint32_t) {
    for (uint32_t lm = tile_labels; lm; lm &= lm - 1u) acc[__builtin_ctz(lm)][tid] = 0ull;
  };
  auto on_entry = [&](int g, uint32_t, bool, u64, float wgt, float, float) {
    // wgt <= 0.99: the product is exact and below 2^32
    const uint32_t q = (uint32_t)rintf(wgt * 4294967296.0f);
#pragma unroll 1
    for (uint32_t lm = wave_labels; lm; lm &= lm - 1u) {
      const uint32_t l = (uint32_t)__builtin_ctz(lm);
      const uint32_t ql = lab == l ? q : 0u;
      const uint32_t lo = row_sum_u32(ql & 0xFFFFu), hi = row_sum_u32(ql >> 16);
      if ((lane & 15u) == 0u && (lo | hi)) atomicAdd(&acc[l][g], (u64)lo + ((u64)hi << 16));
    }
  };
  auto on_chunk_end = [&](uint32_t) {
    const uint32_t gid = __float_as_uint(sh.C[tid].z);
    for (uint32_t lm = tile_labels; lm; lm &= lm - 1u) {
      const uint32_t l = (uint32_t)__builtin_ctz(lm);
      const u64 v = acc[l][tid];
      // (a slot is nonzero only where an entry was staged: the cull mask has no bit beyond the list)
      if (v && gid < vb.P) atomicAdd(vb.votes + (size_t)gid * vb.nlabels + l, v);
    }
  };
  walk_tile(sh, wp, bv, nc, wave_nc, T, on_stage, on_entry, on_chunk_end);
}

template <int NL>
__global__ void __launch_bounds__(256) label_render_kernel(LabelRenderBatch lb) {
  __shared__ TileShared<WALK_CHUNK> sh;
  __shared__ uint32_t glab[WALK_CHUNK];   // label of the staged Gaussian; NO_LABEL: none
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(lb.b, bid);
  LabelOut out;
  select_of_view(lb.b, lb.out, bid, out);
  const WalkPixel wp = walk_pixel(bv, bid);
  if (!wp.valid) return;
  const uint32_t nc = wp.inside ? min(bv.n_contrib[wp.pix], wp.tl.total) : 0u;
  const uint32_t wave_nc = wave_deepest(nc);

  float T = 1.0f;
  float S[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) S[l] = 0.0f;
  auto on_stage = [&](int id, uint32_t) {
    uint32_t gl = NO_LABEL;
    if (id >= 0 && (uint32_t)id < lb.P) gl = lb.gaussian_label[id];
    glab[threadIdx.x] = gl < lb.nlabels ? gl : NO_LABEL;
  };
  auto on_entry = [&](int g, uint32_t, bool, u64, float wgt, float, float) {
    const uint32_t el = __builtin_amdgcn_readfirstlane(glab[g]);   // wave-uniform: one entry, one Gaussian
#pragma unroll
    for (int l = 0; l < NL; l++) S[l] = __builtin_fmaf(wgt, el == (uint32_t)l ? 1.0f : 0.0f, S[l]);
  };
  WalkNoHook none;
  walk_tile(sh, wp, bv, nc, wave_nc, T, on_stage, on_entry, none);
  if (wp.inside) {
    float best = 0.0f;
    uint32_t best_l = NO_LABEL;
#pragma unroll
    for (int l = 0; l < NL; l++) {   // rising l and a strict compare: the smallest label of the largest sum, and only a sum > 0
      const bool up = S[l] > best;
      best_l = up ? (uint32_t)l : best_l;
      best = up ? S[l] : best;
    }
    out.label[wp.pix] = (uint8_t)best_l;
    out.weight[wp.pix] = best;
  }
}

}  // namespace

extern "C" int b3gs_label_votes_batch(int32_t nviews, const B3gsLabelVoteView* views, int32_t nlabels, uint64_t* votes_q32,
                                      b3gs_stream_t stream) {
  static const char* what = "b3gs_label_votes_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (nlabels < 1 || nlabels > B3GS_MAX_LABELS) return b3gs_fail(B3GS_ERR_ARG, what, "1..16 labels");
  if (!views || !votes_q32) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table or votes array");
  for (int k = 0; k < nviews; k++) {
    if (const char* bad = check_state(views[k], views[0])) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (!views[k].labels) return b3gs_fail(B3GS_ERR_ARG, what, "NULL label plane in a view");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  VoteBatch vb;
  memset(&vb, 0, sizeof(vb));
  vb.P = (uint32_t)P;
  vb.nlabels = (uint32_t)nlabels;
  vb.votes = reinterpret_cast<u64*>(votes_q32);
  const int total = fill_blend_batch(vb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) vb.labels[k] = views[k].labels;
  hipLaunchKernelGGL(label_votes_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, vb);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_label_render_batch(int32_t nviews, const B3gsLabelRenderView* views, int32_t nlabels,
                                       const uint8_t* gaussian_label, b3gs_stream_t stream) {
  static const char* what = "b3gs_label_render_batch";
  if (nviews < 1 || nviews > B3GS_MAX_FUSED_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views per call");
  if (nlabels < 1 || nlabels > B3GS_MAX_LABELS) return b3gs_fail(B3GS_ERR_ARG, what, "1..16 labels");
  if (!views || !gaussian_label) return b3gs_fail(B3GS_ERR_ARG, what, "NULL view table or Gaussian label array");
  for (int k = 0; k < nviews; k++) {
    if (const char* bad = check_state(views[k], views[0])) return b3gs_fail(B3GS_ERR_ARG, what, bad);
    if (!views[k].label || !views[k].weight) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output plane in a view");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  LabelRenderBatch lb;
  memset(&lb, 0, sizeof(lb));
  lb.P = (uint32_t)P;
  lb.nlabels = (uint32_t)nlabels;
  lb.gaussian_label = gaussian_label;
  const int total = fill_blend_batch(lb.b, nviews, views, P);
  for (int k = 0; k < nviews; k++) lb.out[k] = LabelOut{views[k].label, views[k].weight};
  const dim3 grid(total), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (nlabels <= 2) hipLaunchKernelGGL(label_render_kernel<2>, grid, block, 0, s, lb);
  else if (nlabels <= 4) hipLaunchKernelGGL(label_render_kernel<4>, grid, block, 0, s, lb);
  else if (nlabels <= 8) hipLaunchKernelGGL(label_render_kernel<8>, grid, block, 0, s, lb);
  else hipLaunchKernelGGL(label_render_kernel<16>, grid, block, 0, s, lb);
  return b3gs_launch_status(what);
}
