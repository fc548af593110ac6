// Per-Gaussian render contribution (added to ABI 18): a second walk of the tile lists a finished forward left on the device,
// which attributes every blend weight w = alpha * T to the Gaussian it belongs to.  Four statistics per Gaussian, summed over
// the counted pixels of up to 8 views per launch: sum of w (as an integer: rint(w * 2^32)), number of pixels it was blended
// into, largest w, number of pixels where it holds the largest w.
//
// The walk is the forward's (render.hip): one 256-thread workgroup per 16x16 tile, one wave per 8x8 quadrant, the list staged
// 256 entries at a time through LDS by the same stage_chunk() -- same quadrant cull -- and every entry evaluated with the same
// blend_power() / clamp, so an entry is blended here exactly where the forward blended it.  The saturation stop is not
// evaluated again: a pixel walks the positions below its n_contrib, which already ends in front of the stopping entry.
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
#include "blend_common.h"
#include <cstring>

namespace {

constexpr int CONTRIB_CHUNK = 256;

struct ContribBatch {
  BlendBatch b;
  const uint8_t* mask[B3GS_MAX_FUSED_VIEWS];
  uint32_t P;
  B3gsContribOut out;
};

template <int CTRL>
__device__ __forceinline__ uint32_t row_move(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// Reductions over the 16 lanes of a DPP row; every lane of the row gets the result.  All 64 lanes must be active.
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
  v += row_move<0xB1>(v);
  v += row_move<0x4E>(v);
  v += row_move<0x141>(v);
  v += row_move<0x140>(v);
  return v;
}
__device__ __forceinline__ uint32_t row_max(uint32_t v) {
  v = max(v, row_move<0xB1>(v));
  v = max(v, row_move<0x4E>(v));
  v = max(v, row_move<0x141>(v));
  v = max(v, row_move<0x140>(v));
  return v;
}

__global__ void __launch_bounds__(256) contrib_kernel(ContribBatch cb) {
  __shared__ TileShared<CONTRIB_CHUNK> sh;
  __shared__ u64 acc_w[CONTRIB_CHUNK];
  __shared__ uint32_t acc_h[CONTRIB_CHUNK], acc_m[CONTRIB_CHUNK];
  const int bid = (int)blockIdx.x;
  const BlendView bv = select_view(cb.b, bid);
  const uint8_t* __restrict__ mask = cb.mask[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < cb.b.n && bid >= cb.b.v[k].block_base) mask = cb.mask[k];
  const int W = bv.W, H = bv.H, grid_x = bv.grid_x, ntiles = bv.ntiles;
  const int tile = tile_of_block(bid - bv.block_base, ntiles);
  if (tile >= ntiles) return;
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const unsigned tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int px = tile_x * B3GS_TILE + (int)((w & 1) * 8 + (lane & 7));
  const int py = tile_y * B3GS_TILE + (int)((w >> 1) * 8 + (lane >> 3));
  const float fpx = (float)px, fpy = (float)py;
  const TileList tl = tile_list(bv, tile, true);
  // positions this pixel walks: below its n_contrib, never past the list; none for a pixel outside the image or masked out
  uint32_t nc = 0u;
  if (px < W && py < H) {
    const size_t pix = (size_t)py * W + px;
    if (!mask || mask[pix]) nc = min(bv.n_contrib[pix], tl.total);
  }
  uint32_t wave_nc = nc;   // the quadrant's deepest position
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wave_nc = max(wave_nc, (uint32_t)__shfl_xor((int)wave_nc, d, 64));
  wave_nc = __builtin_amdgcn_readfirstlane(wave_nc);

  float T = 1.0f;
  float best_w = -1.0f;      // largest weight so far at this pixel (-1: nothing blended yet) and whose it is
  uint32_t best_g = 0u;
  for (uint32_t c0 = 0u;; c0 += (uint32_t)CONTRIB_CHUNK) {
    if (!__syncthreads_or(nc > c0)) break;
    stage_chunk(sh, tl, bv.idx_mask, bv.rec, c0, (float)(tile_x * B3GS_TILE), (float)(tile_y * B3GS_TILE));
    acc_w[tid] = 0ull;
    acc_h[tid] = 0u;
    acc_m[tid] = 0u;
    __syncthreads();
    if (wave_nc > c0) {
#pragma unroll 1
      for (int pw = 0; pw < CONTRIB_CHUNK / 64; pw++) {
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
          const u64 bal = __builtin_amdgcn_ballot_w64(live);
          if (bal == 0ull) continue;
          const float wgt = live ? alpha * T : 0.0f;
          T = live ? T * (1.0f - alpha) : T;
          const bool better = live && wgt > best_w;
          best_g = better ? __float_as_uint(sh.C[g].z) : best_g;
          best_w = better ? wgt : best_w;
          // wgt <= 0.99: the product is exact and below 2^32
          const uint32_t q = (uint32_t)rintf(wgt * 4294967296.0f);
          const uint32_t lo = row_sum(q & 0xFFFFu), hi = row_sum(q >> 16);
          const uint32_t mx = row_max(__float_as_uint(wgt));
          if ((lane & 15u) == 0u) {
            const uint32_t n = (uint32_t)__builtin_popcount((uint32_t)(bal >> (lane & 48u)) & 0xFFFFu);
            if (n) {
              atomicAdd(&acc_w[g], (u64)lo + ((u64)hi << 16));
              atomicAdd(&acc_h[g], n);
              atomicMax(&acc_m[g], mx);
            }
          }
        }
      }
    }
    __syncthreads();
    const uint32_t n = acc_h[tid];
    if (n) {
      const uint32_t gid = __float_as_uint(sh.C[tid].z);
      if (gid < cb.P) {
        atomicAdd(cb.out.weight_q32 + gid, acc_w[tid]);
        atomicAdd(cb.out.hits + gid, n);
        atomicMax(cb.out.wmax_bits + gid, acc_m[tid]);
      }
    }
  }
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
  for (int k = 0; k < nviews; k++) {
    const B3gsContribView& v = views[k];
    if (!v.view) return b3gs_fail(B3GS_ERR_ARG, what, "a view without its B3gsScene");
    if (!v.geometry || !v.binning || !v.image) return b3gs_fail(B3GS_ERR_ARG, what, "NULL state buffer in a view");
    if (v.view->W <= 0 || v.view->H <= 0) return b3gs_fail(B3GS_ERR_ARG, what, "W/H must be positive");
    if (v.view->P < 0 || v.view->P != views[0].view->P)
      return b3gs_fail(B3GS_ERR_ARG, what, "the views of one call share P (the output arrays are [P])");
  }
  const int32_t P = views[0].view->P;
  if (P == 0) return B3GS_OK;
  ContribBatch cb;
  memset(&cb, 0, sizeof(cb));
  cb.b.n = nviews;
  cb.P = (uint32_t)P;
  cb.out = *out;
  int total = 0;
  for (int k = 0; k < nviews; k++) {
    const B3gsContribView& v = views[k];
    GeomView g;
    ImgView im;
    BinView b;
    b3gs_geom_view(const_cast<char*>(v.geometry), P, &g);
    b3gs_img_view(const_cast<char*>(v.image), v.view->W, v.view->H, &im);
    b3gs_bin_view(const_cast<char*>(v.binning), P, 1, &b);   // the tile lists sit at offset 0 whatever the capacity
    cb.b.v[k] = b3gs_blend_view(*v.view, g, b, im);
    cb.b.v[k].round = 2;       // every tile over segment 1 + segment 2
    cb.b.v[k].block_base = total;
    total += blocks_of(cb.b.v[k]);
    cb.mask[k] = v.pixel_mask;
  }
  hipLaunchKernelGGL(contrib_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, cb);
  return b3gs_launch_status(what);
}
