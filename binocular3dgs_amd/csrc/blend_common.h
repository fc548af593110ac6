// Device functions shared by the kernels that walk a tile's list pixel by pixel: the blend (render.hip) and, through
// tile_walk.h, the second walks (contrib.hip, pixelmaps.hip, segment.hip, features.hip).  All of it is force-inlined: one workgroup -> tile
// map, the two-segment tile list, the LDS staging with its quadrant cull and the exponent of the Gaussian, so that a second
// walk of the lists takes every skip decision from the same instructions as the forward that wrote n_contrib.
#pragma once
#include "b3gs_internal.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ unsigned lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
__device__ __forceinline__ u64 uniform_u64(u64 v) {
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// XCD-aware tile assignment: workgroup b is observed to run on XCD b % 8; give each XCD a
// contiguous band of tiles.  Placement only affects L2 hit rate, never results.
__device__ __forceinline__ int tile_of_block(int bid, int ntiles) {
  const int per = (ntiles + 7) >> 3;
  return (bid & 7) * per + (bid >> 3);
}
// workgroups a view takes in a launch that gives every tile one workgroup (a multiple of 8: whole XCD classes)
inline int blocks_of(const BlendView& v) { return ((v.ntiles + 7) / 8) * 8; }

// Pick the view a workgroup belongs to.  The table travels in the kernel arguments; a chain of
// wave-uniform selects (scalar moves, once per workgroup) avoids dynamic indexing of the argument
// block, which the compiler would otherwise copy to scratch memory.
__device__ __forceinline__ BlendView select_view(const BlendBatch& batch, int bid) {
  BlendView v = batch.v[0];
#pragma unroll
  for (int k = 1; k < B3GS_MAX_FUSED_VIEWS; k++)
    if (k < batch.n && bid >= batch.v[k].block_base) v = batch.v[k];
  return v;
}

// CHUNK = Gaussians staged per round (a multiple of 64, at most the 256 threads of the workgroup)
template <int CHUNK>
struct TileShared {
  float4 A[CHUNK];  // x, y, cxx, cxy
  float4 B[CHUNK];  // cyy, opacity, r, g
  float4 C[CHUNK];  // b, depth, Gaussian index (bits), -
  u64 mask[4][CHUNK / 64];   // [quadrant][producer wave]
};

// A tile's list is the concatenation of up to two segments (two-round binning, b3gs_internal.h BinJob::K1): positions
// [0, len1) live in point_list at r1.x, positions [len1, len1 + len2) in point_list2 at r2.x.
struct TileList {
  const uint32_t* list1;
  const uint32_t* list2;
  uint32_t first1, first2, len1, total;
};
__device__ __forceinline__ TileList tile_list(const BlendView& bv, int tile, bool with_segment2) {
  uint2 r1 = bv.ranges[tile];
  if (r1.y <= r1.x) r1 = make_uint2(0u, 0u);   // empty tiles hold (0xFFFFFFFF, 0)
  uint2 r2 = with_segment2 ? bv.ranges2[tile] : make_uint2(0u, 0u);
  if (r2.y <= r2.x) r2 = make_uint2(0u, 0u);
  TileList t;
  t.list1 = bv.point_list;
  t.list2 = bv.point_list2;
  t.first1 = r1.x;
  t.first2 = r2.x;
  t.len1 = r1.y - r1.x;
  t.total = t.len1 + (r2.y - r2.x);
  return t;
}

// Stage one chunk: lane `tid` fetches list position (q0 + tid); returns the Gaussian id (or -1).
template <int CHUNK>
__device__ __forceinline__ int stage_chunk(TileShared<CHUNK>& sh, const TileList& tl, uint32_t idx_mask,
                                           const float4* __restrict__ rec, uint32_t q0, float tile_px, float tile_py) {
  const unsigned tid = threadIdx.x;
  const uint32_t q = q0 + tid;
  int id = -1;
  // bit q of `hits`: the staged Gaussian can reach quadrant q.  (A bit mask and a rolled loop over the quadrants: the four
  // exact tests unrolled side by side were what set the register count of BOTH blend kernels -- 70 instead of 44 VGPRs for
  // the forward -- and staging runs once per 256 list entries.)
  uint32_t hits = 0u;
  if (CHUNK < 256 && tid >= (unsigned)CHUNK) return id;  // whole waves: wave-uniform exit
  if (q < tl.total) {
    const uint32_t word = q < tl.len1 ? tl.list1[tl.first1 + q] : tl.list2[tl.first2 + (q - tl.len1)];
    id = (int)(word & idx_mask);
    const float4* r = rec + 4 * (size_t)id;
    const float4 r0 = r[0], r1 = r[1], r2 = r[2];
    sh.A[tid] = r0;
    sh.B[tid] = r1;
    sh.C[tid] = make_float4(r2.x, r2.y, __int_as_float(id), 0.f);
    // footprint [x-ex, x+ex] x [y-ey, y+ey] against the four 8x8 quadrants (pixel centres
    // tile_p + {0..7} and tile_p + {8..15})
    const float lx = r0.x - r2.z - tile_px, hx = r0.x + r2.z - tile_px;
    const float ly = r0.y - r2.w - tile_py, hy = r0.y + r2.w - tile_py;
    const bool xl = (lx <= 7.0f) && (hx >= 0.0f), xr = (lx <= 15.0f) && (hx >= 8.0f);
    const bool yt = (ly <= 7.0f) && (hy >= 0.0f), yb = (ly <= 15.0f) && (hy >= 8.0f);
    hits = (uint32_t)(xl && yt) | ((uint32_t)(xr && yt) << 1) | ((uint32_t)(xl && yb) << 2) | ((uint32_t)(xr && yb) << 3);
    // Exact test for the quadrants the bounding box reaches: the smallest value of the quadratic form
    // over the quadrant's pixel rectangle against tau = ln(255 opacity) (alpha >= 1/255 <=> form <= tau).
    // One thread does this once per staged Gaussian; every candidate it removes saves a 64-lane evaluation
    // in each direction.  Conservative: continuous rectangle >= pixel centres, plus a rounding margin.
    if (hits) {
      const float cxx = r0.z, cxy = r0.w, cyy = r1.x;
      const float tau = __logf(255.0f * r1.y) * 1.0005f + 2e-3f;
      const float icx = __builtin_amdgcn_rcpf(cxx), icy = __builtin_amdgcn_rcpf(cyy);
      const float ox = tile_px - r0.x, oy = tile_py - r0.y;   // rectangle corner relative to the mean
#pragma unroll 1
      for (int qd = 0; qd < 4; qd++) {
        if (!((hits >> qd) & 1u)) continue;
        const float ax = ox + (float)((qd & 1) * 8), bx = ax + 7.0f;
        const float ay = oy + (float)((qd >> 1) * 8), by = ay + 7.0f;
        const bool inside = (ax <= 0.0f) && (bx >= 0.0f) && (ay <= 0.0f) && (by >= 0.0f);
        float fmin = 3.0e38f;
#pragma unroll
        for (int e = 0; e < 2; e++) {
          const float dx = e ? bx : ax;                                   // vertical edge
          const float dy = fminf(fmaxf(-cxy * dx * icy, ay), by);
          fmin = fminf(fmin, 0.5f * (cxx * dx * dx + cyy * dy * dy) + cxy * dx * dy);
          const float ey = e ? by : ay;                                   // horizontal edge
          const float ex = fminf(fmaxf(-cxy * ey * icx, ax), bx);
          fmin = fminf(fmin, 0.5f * (cxx * ex * ex + cyy * ey * ey) + cxy * ex * ey);
        }
        // (a NaN anywhere fails `!(fmin > tau)`'s complement only by keeping the candidate)
        if (!(inside || !(fmin > tau))) hits &= ~(1u << qd);
      }
    }
  }
  const unsigned w = tid >> 6;
#pragma unroll
  for (int qd = 0; qd < 4; qd++) {
    const u64 m = __ballot((hits >> qd) & 1u);
    if ((tid & 63) == 0) sh.mask[qd][w] = m;
  }
  return id;
}

// the exponent of a Gaussian at a pixel: the products and their order are the skip decisions of every walk of a tile list
__device__ __forceinline__ float blend_power(const float4& A, float cyy, float dx, float dy) {
  const float q = __builtin_fmaf(cyy * dy, dy, (A.z * dx) * dx);
  return __builtin_fmaf(-A.w * dx, dy, -0.5f * q);
}

}  // namespace
