// The second walk of a finished forward's tile lists, stated once for the kernels that reduce it: contrib.hip (per Gaussian),
// pixelmaps.hip (per pixel), segment.hip (votes per Gaussian and label, label render per pixel), features.hip (feature render per
// pixel and channel, feature lift per Gaussian and channel).
//
// The walk is the forward's (render.hip): one 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant, the list staged
// WALK_CHUNK entries at a time through LDS by the same stage_chunk() -- same quadrant cull -- and every entry evaluated with the
// same blend_power() / clamp, the same test `pos < nc && !(power > 0) && !(alpha < ALPHA_MIN)` and the same update of T, so an
// entry is blended here exactly where the forward blended it.  The saturation stop is not evaluated again: a pixel walks the
// positions below its n_contrib, which already ends in front of the stopping entry.
//
// A kernel states what is its own -- which pixels walk (nc), its accumulators, and three hooks -- and walk_tile() owns the
// rest: the loop, its barriers, the skip decisions and T.  The hooks are lambdas taken by reference and inlined into the one
// loop; what they capture by reference stays in registers.
#pragma once
#include "blend_common.h"
#include <cstring>
#include <type_traits>

namespace {

constexpr int WALK_CHUNK = 256;

// ---- device ------------------------------------------------------------------------------------------------------------------
// What a thread knows before it walks: its tile and its pixel.  valid: the workgroup has a tile (workgroup-uniform; a kernel
// returns on !valid BEFORE any barrier, and reads nothing else of the struct).
struct WalkPixel {
  bool valid, inside;       // inside: the pixel lies in the image
  int tile_x, tile_y, px, py;
  float fpx, fpy;
  size_t pix;               // py * W + px (0 outside the image)
  TileList tl;              // both segments
};
__device__ __forceinline__ WalkPixel walk_pixel(const BlendView& bv, int bid) {
  WalkPixel p = {};
  const int tile = tile_of_block(bid - bv.block_base, bv.ntiles);
  p.valid = tile < bv.ntiles;
  if (!p.valid) return p;
  p.tile_x = tile % bv.grid_x;
  p.tile_y = tile / bv.grid_x;
  const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  p.px = p.tile_x * B3GS_TILE + (int)((w & 1) * 8 + (lane & 7));
  p.py = p.tile_y * B3GS_TILE + (int)((w >> 1) * 8 + (lane >> 3));
  p.fpx = (float)p.px;
  p.fpy = (float)p.py;
  p.inside = p.px < bv.W && p.py < bv.H;
  p.pix = p.inside ? (size_t)p.py * bv.W + p.px : 0;
  p.tl = tile_list(bv, tile, true);
  return p;
}

// A kernel's own per-view table (masks, output planes), picked as select_view() picks the view: a chain of wave-uniform
// selects, never a dynamic index into the argument block (which the compiler would copy to scratch memory).  The pick goes
// into the caller's variable: returned by value, a row of five pointers (pixelmaps.hip) took the whole table to scratch.
template <typename T>
__device__ __forceinline__ void select_of_view(const BlendBatch& batch, const T (&table)[B3GS_MAX_FUSED_VIEWS], int bid, T& v) {
  v = table[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < batch.n && bid >= batch.v[k].block_base) v = table[k];
}

// the quadrant's deepest position: the largest nc of the wave, wave-uniform
__device__ __forceinline__ uint32_t wave_deepest(uint32_t nc) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nc = max(nc, (uint32_t)__shfl_xor((int)nc, d, 64));
  return __builtin_amdgcn_readfirstlane(nc);
}

// the hook of a kernel that has nothing to do there
struct WalkNoHook {
  template <typename... A>
  __device__ __forceinline__ void operator()(A...) const {}
};

// Walk the tile's list.  nc: the positions this pixel walks (below its n_contrib, never past the list; 0: none); wave_nc =
// wave_deepest(nc); T: the pixel's transmittance, 1 before the walk.  Every thread of the workgroup calls this.
//   on_stage(id, c0)       every thread, after it staged entry c0 + tid (Gaussian id, -1 beyond the list) and before the barrier
//                          that publishes the chunk: stores of its own per-chunk LDS next to the staged records
//   on_entry(g, pos, live, ballot, wgt, alpha, T)
//                          all 64 lanes of a wave, per entry (slot g of the chunk, list position pos) that at least one lane
//                          blends, in list order: live = this lane blends it, ballot = the live lanes, wgt = alpha * T (0 where
//                          not live), T = the transmittance in FRONT of the entry.  walk_tile updates T afterwards.
//   on_chunk_end(c0)       every thread, after a barrier behind the chunk's walk: flushes of what on_entry left in LDS.  With
//                          WalkNoHook there is no such barrier: the loop's first one also stands between a chunk's last read
//                          and the next staging.
template <int CHUNK, typename OnStage, typename OnEntry, typename OnChunkEnd>
__device__ __forceinline__ void walk_tile(TileShared<CHUNK>& sh, const WalkPixel& wp, const BlendView& bv, uint32_t nc,
                                          uint32_t wave_nc, float& T, OnStage& on_stage, OnEntry& on_entry,
                                          OnChunkEnd& on_chunk_end) {
  const unsigned w = threadIdx.x >> 6;
  for (uint32_t c0 = 0u;; c0 += (uint32_t)CHUNK) {
    if (!__syncthreads_or(nc > c0)) break;
    const int id = stage_chunk(sh, wp.tl, bv.idx_mask, bv.rec, c0, (float)(wp.tile_x * B3GS_TILE), (float)(wp.tile_y * B3GS_TILE));
    on_stage(id, c0);
    __syncthreads();
    if (wave_nc > c0) {
#pragma unroll 1
      for (int pw = 0; pw < CHUNK / 64; pw++) {
        if (c0 + (uint32_t)(pw * 64) >= wave_nc) break;
        u64 m = uniform_u64(sh.mask[w][pw]);
        while (m) {
          const int g = pw * 64 + __builtin_ctzll(m);
          m &= m - 1ull;
          const uint32_t pos = c0 + (uint32_t)g;
          if (pos >= wave_nc) break;   // (the bits come in rising order)
          const float4 A = sh.A[g];
          const float2 B = *reinterpret_cast<const float2*>(&sh.B[g]);   // cyy, opacity
          const float dx = A.x - wp.fpx, dy = A.y - wp.fpy;
          const float power = blend_power(A, B.x, dx, dy);
          const float alpha = fminf(B3GS_ALPHA_MAX, B.y * __expf(power));
          const bool live = pos < nc && !(power > 0.0f) && !(alpha < B3GS_ALPHA_MIN);
          const u64 ballot = __builtin_amdgcn_ballot_w64(live);
          if (ballot == 0ull) continue;
          on_entry(g, pos, live, ballot, live ? alpha * T : 0.0f, alpha, T);
          T = live ? T * (1.0f - alpha) : T;
        }
      }
    }
    if constexpr (!std::is_same<OnChunkEnd, WalkNoHook>::value) {
      __syncthreads();
      on_chunk_end(c0);
    }
  }
}

// Reductions over the 16 lanes of a DPP row; every lane of the row gets the result.  All 64 lanes must be active.
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
template <int CTRL>
__device__ __forceinline__ uint32_t row_move(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t row_sum_u32(uint32_t v) {
  v += row_move<0xB1>(v);
  v += row_move<0x4E>(v);
  v += row_move<0x141>(v);
  v += row_move<0x140>(v);
  return v;
}
__device__ __forceinline__ uint32_t row_max_u32(uint32_t v) {
  v = max(v, row_move<0xB1>(v));
  v = max(v, row_move<0x4E>(v));
  v = max(v, row_move<0x141>(v));
  v = max(v, row_move<0x140>(v));
  return v;
}

// ---- host: what the launchers of these kernels share ---------------------------------------------------------------------------
// The state checks of one view of a call; -> NULL or what is wrong.  same_p: the message for views that differ in P.
template <typename View>
const char* check_state(const View& v, const View& first, const char* same_p = "the views of one call share P (they are views of one model)") {
  if (!v.view) return "a view without its B3gsScene";
  if (!v.geometry || !v.binning || !v.image) return "NULL state buffer in a view";
  if (v.view->W <= 0 || v.view->H <= 0) return "W/H must be positive";
  if (!first.view || v.view->P < 0 || v.view->P != first.view->P) return same_p;
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

// fill a (zeroed) batch from the checked views of a call; -> the workgroups of the launch, one per tile
template <typename View>
int fill_blend_batch(BlendBatch& batch, int32_t nviews, const View* views, int32_t P) {
  batch.n = nviews;
  int total = 0;
  for (int k = 0; k < nviews; k++) {
    batch.v[k] = blend_view_of(views[k], P, total);
    total += blocks_of(batch.v[k]);
  }
  return total;
}

}  // namespace
