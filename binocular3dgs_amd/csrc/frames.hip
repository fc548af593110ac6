// Frames of a rendered path (ABI 12): the three uint8 images the reference's spiral.py:101-131 writes per frame -- the
// render, the gray depth map and the turbo colour map of that depth map -- for up to 8 views of one W x H per call, without a
// host read.  Launches (whatever the view count):
//   1 minmax    per-workgroup min / max of every view's depth (comparisons only: exact); zeroes the histograms
//   2 value     folds the partials, v = 1 - (1 - (depth - min) / (max - min)) * alpha into the workspace, histogram of the
//               top 11 key bits of v
//   3 pick      per view and target rank: the bucket that holds it, the rank inside that bucket
//   4 hist      next 11 bits of the values inside the picked buckets      5 pick
//   6 hist      last 10 bits                                              7 pick  -> the exact order statistics
//   8 encode    4 pixels per thread: rgb, gray, colour map (12 bytes per image per thread)
// The order statistics come from a radix select on order-preserving keys of v: histograms in LDS, flushed with integer
// atomics (counts do not depend on the order of the additions), the pick reads them in a fixed order.  No float atomics:
// the same inputs give the same bits on every call.
#include "b3gs_internal.h"

#include <float.h>

namespace {

constexpr int FV = B3GS_MAX_FRAME_VIEWS;
constexpr int NT = 4;              // target ranks per view: the two neighbours of each of the two percentile positions
constexpr int TPB = 256;
constexpr int NB1 = 2048, NB2 = 2048, NB3 = 1024;   // key bits 31..21, 20..10, 9..0

struct FrameTable {
  const float* rgb[FV];
  const float* depth[FV];
  const float* alpha[FV];
  uint8_t* rgb_out[FV];
  uint8_t* gray_out[FV];
  uint8_t* cmap_out[FV];
  int32_t need_v[FV];              // the view's v is needed (gray, colour map or bounds)
};

// the two percentile positions of np.interp(ps * (n / 100), [1..n], sort(v)) and the ranks they read (host-computed: they
// depend on n and the percentile only)
struct Targets {
  double q[2];                     // ps[k] * fp32(n / 100), in fp64
  int64_t j[2];                    // 0-based rank of the left neighbour when 1 <= q < n
  uint32_t rank[NT];               // q[0]: rank[0], rank[1]; q[1]: rank[2], rank[3]
};

struct Work {
  float* v;                        // [nv][n4]
  float2* part;                    // [nv][bpv]  min, max of a workgroup's pixels
  float2* mm;                      // [nv]       min, max of the view
  uint32_t* hist1;                 // [nv][NB1]
  uint32_t* hist2;                 // [nv][NT][NB2]
  uint32_t* hist3;                 // [nv][NT][NB3]
  uint2* st;                       // [3][nv][NT]  after pass k: (key prefix, rank inside the prefix's bucket)
  size_t hist_words;
};

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ~8 pixels per thread
static int blocks_per_view(int64_t n) {
  const int64_t b = (n + 8 * TPB - 1) / (8 * TPB);
  return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

static size_t carve(int nv, int64_t n, Work* w, char* base) {
  const int64_t n4 = (n + 3) & ~(int64_t)3;
  const int bpv = blocks_per_view(n);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += align256(bytes);
    return p;
  };
  Work t;
  t.v = (float*)take((size_t)nv * n4 * sizeof(float));
  t.part = (float2*)take((size_t)nv * bpv * sizeof(float2));
  t.mm = (float2*)take((size_t)nv * sizeof(float2));
  t.hist_words = (size_t)nv * (NB1 + NT * NB2 + NT * NB3);
  t.hist1 = (uint32_t*)take(t.hist_words * sizeof(uint32_t));
  t.hist2 = t.hist1 ? t.hist1 + (size_t)nv * NB1 : nullptr;
  t.hist3 = t.hist2 ? t.hist2 + (size_t)nv * NT * NB2 : nullptr;
  t.st = (uint2*)take((size_t)3 * nv * NT * sizeof(uint2));
  if (w) *w = t;
  return off;
}

// order-preserving key of a float (NaN of either sign sorts like the largest / smallest values; v is never -0)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// torchvision's save_image quantiser: x*255, + 0.5 (two roundings: built with -ffp-contract=off), clamp, truncate.  NaN
// gives 0, as the x86 conversion the reference runs on does.
__device__ __forceinline__ uint32_t quant(float x) {
  float t = x * 255.f;
  t = t + 0.5f;
  t = t > 0.f ? t : 0.f;
  t = t < 255.f ? t : 255.f;
  return (uint32_t)t;
}

// min / max of a block's values -> every thread
__device__ float2 block_minmax(float mn, float mx) {
  __shared__ float2 red[TPB / 64];
  mn = b3gs_wave_min(mn);
  mx = b3gs_wave_max(mx);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = make_float2(mn, mx);
  __syncthreads();
  float2 r = red[0];
#pragma unroll
  for (int k = 1; k < TPB / 64; k++) r = make_float2(fminf(r.x, red[k].x), fmaxf(r.y, red[k].y));
  return r;
}

// grid (bpv, nv)
__global__ void __launch_bounds__(TPB) frames_minmax_kernel(FrameTable t, int64_t n, int bpv, Work w) {
  const int v = blockIdx.y;
  const size_t gb = (size_t)v * bpv + blockIdx.x, nblk = (size_t)gridDim.y * bpv;
  for (size_t i = gb * TPB + threadIdx.x; i < w.hist_words; i += nblk * TPB) w.hist1[i] = 0u;
  if (!t.need_v[v]) return;
  const float* __restrict__ depth = t.depth[v];
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < n; p += (int64_t)bpv * TPB) {
    const float d = depth[p];
    mn = fminf(mn, d);
    mx = fmaxf(mx, d);
  }
  const float2 r = block_minmax(mn, mx);
  if (threadIdx.x == 0) w.part[(size_t)v * bpv + blockIdx.x] = r;
}

// grid (bpv, nv): v of every pixel (spiral.py:119-120, fp32, that op order) and the histogram of its top 11 key bits
__global__ void __launch_bounds__(TPB) frames_value_kernel(FrameTable t, int64_t n, int64_t n4, int bpv, Work w) {
  const int v = blockIdx.y;
  if (!t.need_v[v]) return;
  __shared__ uint32_t h[NB1];
  for (int i = threadIdx.x; i < NB1; i += TPB) h[i] = 0u;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < bpv; i += TPB) {
    const float2 q = w.part[(size_t)v * bpv + i];
    mn = fminf(mn, q.x);
    mx = fmaxf(mx, q.y);
  }
  const float2 r = block_minmax(mn, mx);      // (its barriers also order the zeroing of h before the adds below)
  if (blockIdx.x == 0 && threadIdx.x == 0) w.mm[v] = r;
  const float range = r.y - r.x;
  const float* __restrict__ depth = t.depth[v];
  const float* __restrict__ alpha = t.alpha[v];
  float* __restrict__ out = w.v + (size_t)v * n4;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < n; p += (int64_t)bpv * TPB) {
    const float d = 1.f - (depth[p] - r.x) / range;
    const float e = d * alpha[p];
    const float val = 1.f - e;
    out[p] = val;
    atomicAdd(&h[fkey(val) >> 21], 1u);
  }
  __syncthreads();
  uint32_t* __restrict__ g = w.hist1 + (size_t)v * NB1;
  for (int i = threadIdx.x; i < NB1; i += TPB)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

// the histogram slot every target uses in pass `pass` (1 or 2): targets whose buckets agree share the first one's slot
__device__ __forceinline__ void target_slots(const uint2* st_prev, uint32_t pre[NT], int slot[NT]) {
#pragma unroll
  for (int k = 0; k < NT; k++) {
    pre[k] = st_prev[k].x;
    slot[k] = k;
    for (int m = k - 1; m >= 0; m--)
      if (pre[m] == pre[k]) slot[k] = slot[m];
  }
}

// grid (bpv, nv): pass 1 -- histogram of key bits 20..10 of the values whose top 11 bits are a target's bucket; pass 2 --
// bits 9..0 of those whose top 22 bits are
__global__ void __launch_bounds__(TPB) frames_hist_kernel(FrameTable t, int pass, int64_t n, int64_t n4, int bpv, Work w) {
  const int v = blockIdx.y;
  if (!t.need_v[v]) return;
  const int nb = pass == 1 ? NB2 : NB3;
  const int shift_hi = pass == 1 ? 21 : 10;
  const int shift_lo = pass == 1 ? 10 : 0;
  __shared__ uint32_t h[NT * NB2];
  for (int i = threadIdx.x; i < NT * nb; i += TPB) h[i] = 0u;
  uint32_t pre[NT];
  int slot[NT];
  const int nv = gridDim.y;
  target_slots(w.st + ((size_t)(pass - 1) * nv + v) * NT, pre, slot);
  __syncthreads();
  const float* __restrict__ val = w.v + (size_t)v * n4;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < n; p += (int64_t)bpv * TPB) {
    const uint32_t key = fkey(val[p]);
    const uint32_t hi = key >> shift_hi, bin = (key >> shift_lo) & (uint32_t)(nb - 1);
#pragma unroll
    for (int k = 0; k < NT; k++)
      if (slot[k] == k && hi == pre[k]) atomicAdd(&h[k * nb + bin], 1u);
  }
  __syncthreads();
  uint32_t* __restrict__ g = (pass == 1 ? w.hist2 + (size_t)v * NT * NB2 : w.hist3 + (size_t)v * NT * NB3);
  for (int k = 0; k < NT; k++) {
    if (slot[k] != k) continue;
    for (int i = threadIdx.x; i < nb; i += TPB)
      if (h[k * nb + i]) atomicAdd(&g[k * nb + i], h[k * nb + i]);
  }
}

// grid (NT, nv): the bucket of pass `pass` (0, 1, 2) that holds target rank blockIdx.x, and the rank inside it
__global__ void __launch_bounds__(TPB) frames_pick_kernel(FrameTable t, int pass, Targets tg, Work w) {
  const int v = blockIdx.y, k = blockIdx.x, nv = gridDim.y;
  if (!t.need_v[v]) return;
  const uint32_t* hist;
  int nb, bits;
  uint32_t prefix = 0, rank = tg.rank[k];
  if (pass == 0) {
    hist = w.hist1 + (size_t)v * NB1;
    nb = NB1;
    bits = 11;
  } else {
    uint32_t pre[NT];
    int slot[NT];
    const uint2* prev = w.st + ((size_t)(pass - 1) * nv + v) * NT;
    target_slots(prev, pre, slot);
    prefix = pre[k];
    rank = prev[k].y;
    nb = pass == 1 ? NB2 : NB3;
    bits = pass == 1 ? 11 : 10;
    hist = (pass == 1 ? w.hist2 + ((size_t)v * NT + slot[k]) * NB2 : w.hist3 + ((size_t)v * NT + slot[k]) * NB3);
  }
  const int per = nb / TPB;                    // 8 or 4 consecutive bins per thread
  const int b0 = threadIdx.x * per;
  uint32_t c[NB1 / TPB];
  uint32_t s = 0;
  for (int i = 0; i < per; i++) {
    c[i] = hist[b0 + i];
    s += c[i];
  }
  // inclusive scan of the per-thread sums (Hillis-Steele in LDS: fixed order)
  __shared__ uint32_t sc[2][TPB];
  int cur = 0;
  sc[0][threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const uint32_t x = sc[cur][threadIdx.x] + (threadIdx.x >= (unsigned)d ? sc[cur][threadIdx.x - d] : 0u);
    sc[cur ^ 1][threadIdx.x] = x;
    cur ^= 1;
    __syncthreads();
  }
  uint32_t before = sc[cur][threadIdx.x] - s;
  if (rank >= before && rank < before + s) {   // exactly one thread: the counts of a bucket add up to its size > rank
    for (int i = 0; i < per; i++) {
      if (rank < before + c[i]) {
        w.st[((size_t)pass * nv + v) * NT + k] = make_uint2((prefix << bits) | (uint32_t)(b0 + i), rank - before);
        break;
      }
      before += c[i];
    }
  }
}

// np.interp(q, [1..n], sorted) from the two order statistics it reads (numpy's arr_interp: left / right ends, an exact hit,
// slope * (q - x_j) + y_j; fp64, no fused multiply-add)
__device__ double interp_at(double q, int64_t j, int64_t n, double a, double b) {
  if (q < 1.0 || q >= (double)n) return a;
  const double xj = (double)(j + 1);
  if (q == xj) return a;
  const double slope = (b - a) / ((double)(j + 2) - xj);
  return slope * (q - xj) + a;
}

// grid (ceil(n / 4 / TPB), nv): 4 pixels per thread, 12 bytes per output image
__global__ void __launch_bounds__(TPB) frames_encode_kernel(FrameTable t, int64_t n, int64_t n4, int vec, Targets tg, Work w,
                                                            const uint8_t* __restrict__ lut_g, double* __restrict__ bounds) {
  const int v = blockIdx.y, nv = gridDim.y;
  __shared__ uint8_t lut[256 * 3];
  uint8_t* __restrict__ cmap = t.cmap_out[v];
  uint8_t* __restrict__ gray = t.gray_out[v];
  uint8_t* __restrict__ rgbo = t.rgb_out[v];
  if (cmap)
    for (int i = threadIdx.x; i < 256 * 3; i += TPB) lut[i] = lut_g[i];
  // the view's bounds (visualize_cmap: lo / hi = percentiles -/+ fp32 eps, curved in fp64)
  bool empty = true;
  double lo_c = 0.0, den = 1.0;
  if (t.need_v[v]) {
    const float2 mm = w.mm[v];
    empty = !(mm.y > mm.x);
    double b[2] = {NAN, NAN};
    if (!empty) {
      const uint2* st = w.st + ((size_t)2 * nv + v) * NT;
      for (int k = 0; k < 2; k++)
        b[k] = interp_at(tg.q[k], tg.j[k], n, (double)unkey(st[2 * k].x), (double)unkey(st[2 * k + 1].x));
    }
    if (bounds && blockIdx.x == 0 && threadIdx.x == 0) {
      bounds[2 * v] = b[0];
      bounds[2 * v + 1] = b[1];
    }
    const double eps = (double)FLT_EPSILON;
    const double lo = b[0] - eps, hi = b[1] + eps;
    const double lc = -log(lo + 1e-6), hc = -log(hi + 1e-6);
    lo_c = lc < hc ? lc : hc;                  // np.minimum (the bounds are finite here)
    den = fabs(hc - lc);
  }
  __syncthreads();
  const int64_t qi = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int64_t p0 = 4 * qi;
  if (p0 >= n) return;
  const int np = n - p0 < 4 ? (int)(n - p0) : 4;
  const bool full = vec && np == 4;
  const float* __restrict__ val = w.v + (size_t)v * n4;

  if (rgbo) {
    const float* __restrict__ rgb = t.rgb[v];
    uint32_t b[12];
    if (full) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float4 x = *reinterpret_cast<const float4*>(rgb + c * n + p0);
        b[c] = quant(x.x);
        b[3 + c] = quant(x.y);
        b[6 + c] = quant(x.z);
        b[9 + c] = quant(x.w);
      }
      uint32_t* o = reinterpret_cast<uint32_t*>(rgbo + 12 * qi);
      o[0] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
      o[1] = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
      o[2] = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
    } else {
      for (int i = 0; i < np; i++)
        for (int c = 0; c < 3; c++) rgbo[3 * (p0 + i) + c] = (uint8_t)quant(rgb[c * n + p0 + i]);
    }
  }
  if (!gray && !cmap) return;
  float x[4];
  if (full) {
    const float4 q = *reinterpret_cast<const float4*>(val + p0);
    x[0] = q.x;
    x[1] = q.y;
    x[2] = q.z;
    x[3] = q.w;
  } else {
    for (int i = 0; i < 4; i++) x[i] = i < np ? val[p0 + i] : 0.f;
  }
  if (gray) {
    uint32_t g[4];
#pragma unroll
    for (int i = 0; i < 4; i++) g[i] = empty ? 0u : quant(x[i]);
    if (full) {
      uint32_t* o = reinterpret_cast<uint32_t*>(gray + 12 * qi);
      o[0] = g[0] | g[0] << 8 | g[0] << 16 | g[1] << 24;
      o[1] = g[1] | g[1] << 8 | g[2] << 16 | g[2] << 24;
      o[2] = g[2] | g[3] << 8 | g[3] << 16 | g[3] << 24;
    } else {
      for (int i = 0; i < np; i++)
        for (int c = 0; c < 3; c++) gray[3 * (p0 + i) + c] = (uint8_t)g[i];
    }
  }
  if (cmap) {
    int idx[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int id = 0;
      if (!empty) {
        // curve_fn in fp32 (x + 1e-6 and log of a float32 array), normalised in fp64, clip, nan_to_num, int(x * 256)
        const float s = x[i] + 1e-6f;
        const float cv = -(float)log((double)s);
        double z = ((double)cv - lo_c) / den;
        z = z != z ? 0.0 : (z < 0.0 ? 0.0 : (z > 1.0 ? 1.0 : z));
        id = (int)(z * 256.0);
        id = id > 255 ? 255 : id;
      }
      idx[i] = 3 * id;
    }
    if (full) {
      uint32_t b[12];
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int c = 0; c < 3; c++) b[3 * i + c] = lut[idx[i] + c];
      uint32_t* o = reinterpret_cast<uint32_t*>(cmap + 12 * qi);
      o[0] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
      o[1] = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
      o[2] = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
    } else {
      for (int i = 0; i < np; i++)
        for (int c = 0; c < 3; c++) cmap[3 * (p0 + i) + c] = lut[idx[i] + c];
    }
  }
}

}  // namespace

extern "C" size_t b3gs_frames_workspace_bytes(int32_t nviews, int32_t H, int32_t W) {
  if (nviews <= 0 || nviews > FV || H <= 0 || W <= 0) return 0;
  return carve(nviews, (int64_t)H * W, nullptr, nullptr);
}

extern "C" int b3gs_encode_frames_batch(int32_t nviews, const B3gsFrameView* views, int32_t H, int32_t W, double percentile,
                                        const uint8_t* lut, void* workspace, double* bounds_out, b3gs_stream_t stream) {
  static const char* what = "b3gs_encode_frames_batch";
  if (nviews <= 0 || nviews > FV || !views || !workspace || H <= 0 || W <= 0)
    return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views, a workspace and a non-empty shape are needed");
  const int64_t n = (int64_t)H * W;
  if (n > ((int64_t)1 << 24)) return b3gs_fail(B3GS_ERR_ARG, what, "at most 2^24 pixels per view");
  if (!(percentile >= 0.0 && percentile <= 100.0)) return b3gs_fail(B3GS_ERR_ARG, what, "percentile must lie in [0, 100]");
  if ((uintptr_t)workspace & 255) return b3gs_fail(B3GS_ERR_ARG, what, "workspace must be 256-byte aligned");
  FrameTable t = {};
  bool any_v = false, any_cmap = false, vec = (n % 4) == 0;
  for (int i = 0; i < nviews; i++) {
    const B3gsFrameView& f = views[i];
    t.rgb[i] = f.rgb;
    t.depth[i] = f.depth;
    t.alpha[i] = f.alpha;
    t.rgb_out[i] = f.rgb_out;
    t.gray_out[i] = f.gray_out;
    t.cmap_out[i] = f.cmap_out;
    t.need_v[i] = (f.gray_out || f.cmap_out || bounds_out) ? 1 : 0;
    if (f.rgb_out && !f.rgb) return b3gs_fail(B3GS_ERR_ARG, what, "rgb_out without rgb");
    if (t.need_v[i] && (!f.depth || !f.alpha)) return b3gs_fail(B3GS_ERR_ARG, what, "gray / colour map / bounds without depth and alpha");
    any_v = any_v || t.need_v[i];
    any_cmap = any_cmap || f.cmap_out;
    if (f.rgb_out) vec = vec && !((uintptr_t)f.rgb & 15) && !((uintptr_t)f.rgb_out & 3);
    if (f.gray_out) vec = vec && !((uintptr_t)f.gray_out & 3);
    if (f.cmap_out) vec = vec && !((uintptr_t)f.cmap_out & 3);
  }
  if (any_cmap && !lut) return b3gs_fail(B3GS_ERR_ARG, what, "a colour map needs the 256 x 3 LUT");
  Work w;
  carve(nviews, n, &w, static_cast<char*>(workspace));
  const int64_t n4 = (n + 3) & ~(int64_t)3;
  const int bpv = blocks_per_view(n);
  hipStream_t s = (hipStream_t)stream;

  // np.interp positions: ps = [50 - p/2, 50 + p/2] (fp64) times acc_w[-1] / 100 (fp32: the cumsum of fp32 ones)
  Targets tg = {};
  const float f100 = (float)n / 100.0f;
  const double ps[2] = {50.0 - percentile / 2, 50.0 + percentile / 2};
  for (int k = 0; k < 2; k++) {
    const double q = ps[k] * (double)f100;
    tg.q[k] = q;
    uint32_t r0, r1;
    if (q < 1.0) {
      r0 = r1 = 0;
      tg.j[k] = 0;
    } else if (q >= (double)n) {
      r0 = r1 = (uint32_t)(n - 1);
      tg.j[k] = n - 1;
    } else {
      const int64_t j = (int64_t)floor(q) - 1;
      tg.j[k] = j;
      r0 = (uint32_t)j;
      r1 = (uint32_t)(j + 1);
    }
    tg.rank[2 * k] = r0;
    tg.rank[2 * k + 1] = r1;
  }

  if (any_v) {
    hipLaunchKernelGGL(frames_minmax_kernel, dim3(bpv, nviews), dim3(TPB), 0, s, t, n, bpv, w);
    hipLaunchKernelGGL(frames_value_kernel, dim3(bpv, nviews), dim3(TPB), 0, s, t, n, n4, bpv, w);
    if (any_cmap || bounds_out) {
      hipLaunchKernelGGL(frames_pick_kernel, dim3(NT, nviews), dim3(TPB), 0, s, t, 0, tg, w);
      hipLaunchKernelGGL(frames_hist_kernel, dim3(bpv, nviews), dim3(TPB), 0, s, t, 1, n, n4, bpv, w);
      hipLaunchKernelGGL(frames_pick_kernel, dim3(NT, nviews), dim3(TPB), 0, s, t, 1, tg, w);
      hipLaunchKernelGGL(frames_hist_kernel, dim3(bpv, nviews), dim3(TPB), 0, s, t, 2, n, n4, bpv, w);
      hipLaunchKernelGGL(frames_pick_kernel, dim3(NT, nviews), dim3(TPB), 0, s, t, 2, tg, w);
    }
  }
  const int64_t quads = (n + 3) / 4;
  hipLaunchKernelGGL(frames_encode_kernel, dim3((unsigned)((quads + TPB - 1) / TPB), nviews), dim3(TPB), 0, s, t, n, n4,
                     vec ? 1 : 0, tg, w, lut, bounds_out);
  return b3gs_launch_status(what);
}
