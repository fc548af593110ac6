// Segmentation from 2D label planes (added to ABI 18): two more reductions of the second walk of a finished forward's tile
// lists that contrib.hip (per Gaussian) and pixelmaps.hip (per pixel) share through blend_common.h.
//
//   b3gs_label_votes_batch    per Gaussian and per label l: the sum of rint(w * 2^32), w = alpha * T, over the blended (view,
//                             pixel, entry) of the Gaussian at pixels whose label byte is l.  What contrib.hip sums under the
//                             pixel mask (labels == l), for every l in ONE walk.
//   b3gs_label_render_batch   per pixel and per label l: S_l = the float32 sum, in list order, of w over the blended entries
//                             whose Gaussian carries label l; the pixel gets the smallest l of the largest S_l > 0, and that S_l.
//
// The walk is the forward's (render.hip): one 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant, the list staged
// 256 entries at a time through LDS by the same stage_chunk() -- same quadrant cull -- and every entry evaluated with the same
// blend_power() / clamp, so an entry is blended here exactly where the forward blended it.  The saturation stop is not
// evaluated again: a pixel walks the positions below its n_contrib, which already ends in front of the stopping entry.
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
#include "blend_common.h"
#include <cstring>

namespace {

constexpr int SEG_CHUNK = 256;
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

template <int CTRL>
__device__ __forceinline__ uint32_t seg_row_move(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// Sum over the 16 lanes of a DPP row; every lane of the row gets the result.  All 64 lanes must be active.
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror  (the row sum of contrib.hip)
__device__ __forceinline__ uint32_t seg_row_sum(uint32_t v) {
  v += seg_row_move<0xB1>(v);
  v += seg_row_move<0x4E>(v);
  v += seg_row_move<0x141>(v);
  v += seg_row_move<0x140>(v);
  return v;
}

__global__ void __launch_bounds__(256) label_votes_kernel(VoteBatch vb) {
  __shared__ TileShared<SEG_CHUNK> sh;
  __shared__ u64 acc[B3GS_MAX_LABELS][SEG_CHUNK];   // [label][chunk entry]: thread i zeroes and flushes column i, no bank conflict
  __shared__ uint32_t wg_labels;
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(vb.b, bid);
  const uint8_t* __restrict__ labels = vb.labels[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < vb.b.n && bid >= vb.b.v[k].block_base) labels = vb.labels[k];
  const int W = bv.W, H = bv.H, grid_x = bv.grid_x, ntiles = bv.ntiles;
  const int tile = tile_of_block(bid - bv.block_base, ntiles);
  if (tile >= ntiles) return;
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int px = tile_x * B3GS_TILE + (int)((w & 1) * 8 + (lane & 7));
  const int py = tile_y * B3GS_TILE + (int)((w >> 1) * 8 + (lane >> 3));
  const float fpx = (float)px, fpy = (float)py;
  const TileList tl = tile_list(bv, tile, true);
  // positions this pixel walks: below its n_contrib, never past the list; none for a pixel outside the image or without a label
  uint32_t nc = 0u, lab = NO_LABEL;
  if (px < W && py < H) {
    const size_t pix = (size_t)py * W + px;
    lab = labels[pix];
    if (lab < vb.nlabels) nc = min(bv.n_contrib[pix], tl.total);
  }
  uint32_t wave_nc = nc;                            // the quadrant's deepest position
  uint32_t wave_labels = nc ? (1u << (lab & 15u)) : 0u;   // the labels of the quadrant's walking pixels (nc > 0: lab < 16)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    wave_nc = max(wave_nc, (uint32_t)__shfl_xor((int)wave_nc, d, 64));
    wave_labels |= (uint32_t)__shfl_xor((int)wave_labels, d, 64);
  }
  wave_nc = __builtin_amdgcn_readfirstlane(wave_nc);
  wave_labels = __builtin_amdgcn_readfirstlane(wave_labels);
  if (tid == 0) wg_labels = 0u;
  __syncthreads();
  if (lane == 0 && wave_labels) atomicOr(&wg_labels, wave_labels);
  __syncthreads();
  const uint32_t tile_labels = __builtin_amdgcn_readfirstlane(wg_labels);

  float T = 1.0f;
  for (uint32_t c0 = 0u;; c0 += (uint32_t)SEG_CHUNK) {
    if (!__syncthreads_or(nc > c0)) break;
    stage_chunk(sh, tl, bv.idx_mask, bv.rec, c0, (float)(tile_x * B3GS_TILE), (float)(tile_y * B3GS_TILE));
    for (uint32_t lm = tile_labels; lm; lm &= lm - 1u) acc[__builtin_ctz(lm)][tid] = 0ull;
    __syncthreads();
    if (wave_nc > c0) {
#pragma unroll 1
      for (int pw = 0; pw < SEG_CHUNK / 64; pw++) {
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
          const float wgt = live ? alpha * T : 0.0f;
          T = live ? T * (1.0f - alpha) : T;
          // wgt <= 0.99: the product is exact and below 2^32
          const uint32_t q = (uint32_t)rintf(wgt * 4294967296.0f);
#pragma unroll 1
          for (uint32_t lm = wave_labels; lm; lm &= lm - 1u) {
            const uint32_t l = (uint32_t)__builtin_ctz(lm);
            const uint32_t ql = lab == l ? q : 0u;
            const uint32_t lo = seg_row_sum(ql & 0xFFFFu), hi = seg_row_sum(ql >> 16);
            if ((lane & 15u) == 0u && (lo | hi)) atomicAdd(&acc[l][g], (u64)lo + ((u64)hi << 16));
          }
        }
      }
    }
    __syncthreads();
    const uint32_t gid = __float_as_uint(sh.C[tid].z);
    for (uint32_t lm = tile_labels; lm; lm &= lm - 1u) {
      const uint32_t l = (uint32_t)__builtin_ctz(lm);
      const u64 v = acc[l][tid];
      // (a slot is nonzero only where an entry was staged: the cull mask has no bit beyond the list)
      if (v && gid < vb.P) atomicAdd(vb.votes + (size_t)gid * vb.nlabels + l, v);
    }
  }
}

template <int NL>
__global__ void __launch_bounds__(256) label_render_kernel(LabelRenderBatch lb) {
  __shared__ TileShared<SEG_CHUNK> sh;
  __shared__ uint32_t glab[SEG_CHUNK];   // label of the staged Gaussian; NO_LABEL: none
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(lb.b, bid);
  LabelOut out = lb.out[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < lb.b.n && bid >= lb.b.v[k].block_base) out = lb.out[k];
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

  float T = 1.0f;
  float S[NL];
#pragma unroll
  for (int l = 0; l < NL; l++) S[l] = 0.0f;
  for (uint32_t c0 = 0u;; c0 += (uint32_t)SEG_CHUNK) {
    if (!__syncthreads_or(nc > c0)) break;   // (also the barrier between the last read of a chunk and the next staging)
    const int id = stage_chunk(sh, tl, bv.idx_mask, bv.rec, c0, (float)(tile_x * B3GS_TILE), (float)(tile_y * B3GS_TILE));
    uint32_t gl = NO_LABEL;
    if (id >= 0 && (uint32_t)id < lb.P) gl = lb.gaussian_label[id];
    glab[tid] = gl < lb.nlabels ? gl : NO_LABEL;
    __syncthreads();
    if (wave_nc <= c0) continue;
#pragma unroll 1
    for (int pw = 0; pw < SEG_CHUNK / 64; pw++) {
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
        const uint32_t el = __builtin_amdgcn_readfirstlane(glab[g]);   // wave-uniform: one entry, one Gaussian
        const float wgt = live ? alpha * T : 0.0f;
        T = live ? T * (1.0f - alpha) : T;
#pragma unroll
        for (int l = 0; l < NL; l++) S[l] = __builtin_fmaf(wgt, el == (uint32_t)l ? 1.0f : 0.0f, S[l]);
      }
    }
  }
  if (inside) {
    float best = 0.0f;
    uint32_t best_l = NO_LABEL;
#pragma unroll
    for (int l = 0; l < NL; l++) {   // rising l and a strict compare: the smallest label of the largest sum, and only a sum > 0
      const bool up = S[l] > best;
      best_l = up ? (uint32_t)l : best_l;
      best = up ? S[l] : best;
    }
    out.label[pix] = (uint8_t)best_l;
    out.weight[pix] = best;
  }
}

// the state checks the two entry points share; -> NULL or what is wrong
template <typename View>
const char* check_state(const View& v, const View& first) {
  if (!v.view) return "a view without its B3gsScene";
  if (!v.geometry || !v.binning || !v.image) return "NULL state buffer in a view";
  if (v.view->W <= 0 || v.view->H <= 0) return "W/H must be positive";
  if (!first.view || v.view->P < 0 || v.view->P != first.view->P) return "the views of one call share P (they are views of one model)";
  return nullptr;
}

template <typename View>
BlendView blend_view_of(const View& v, int32_t P, int block_base) {
  GeomView g;
  ImgView im;
  BinView b;
  b3gs_geom_view(const_cast<char*>(v.geometry), P, &g);
  b3gs_img_view(const_cast<char*>(v.image), v.view->W, v.view->H, &im);
  b3gs_bin_view(const_cast<char*>(v.binning), P, 1, &b);   // the tile lists sit at offset 0 whatever the capacity
  BlendView bv = b3gs_blend_view(*v.view, g, b, im);
  bv.round = 2;       // every tile over segment 1 + segment 2
  bv.block_base = block_base;
  return bv;
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
  vb.b.n = nviews;
  vb.P = (uint32_t)P;
  vb.nlabels = (uint32_t)nlabels;
  vb.votes = reinterpret_cast<u64*>(votes_q32);
  int total = 0;
  for (int k = 0; k < nviews; k++) {
    vb.b.v[k] = blend_view_of(views[k], P, total);
    total += blocks_of(vb.b.v[k]);
    vb.labels[k] = views[k].labels;
  }
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
  lb.b.n = nviews;
  lb.P = (uint32_t)P;
  lb.nlabels = (uint32_t)nlabels;
  lb.gaussian_label = gaussian_label;
  int total = 0;
  for (int k = 0; k < nviews; k++) {
    lb.b.v[k] = blend_view_of(views[k], P, total);
    total += blocks_of(lb.b.v[k]);
    lb.out[k] = LabelOut{views[k].label, views[k].weight};
  }
  const dim3 grid(total), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (nlabels <= 2) hipLaunchKernelGGL(label_render_kernel<2>, grid, block, 0, s, lb);
  else if (nlabels <= 4) hipLaunchKernelGGL(label_render_kernel<4>, grid, block, 0, s, lb);
  else if (nlabels <= 8) hipLaunchKernelGGL(label_render_kernel<8>, grid, block, 0, s, lb);
  else hipLaunchKernelGGL(label_render_kernel<16>, grid, block, 0, s, lb);
  return b3gs_launch_status(what);
}
