// Ground-truth preparation (ABI 13): what the reference does to every dataset image before the first iteration --
//   utils/general_utils.py:22-28  PILtoTorch: PIL.Image.resize(size) with its default filter (BICUBIC, 8 bits per channel), / 255
//   utils/camera_utils.py:22-57   loadCam: alpha split, white-background composite
//   scene/cameras.py:40-47        clamp(0, 1), multiply by the alpha mask
//   train.py:110-120              the DTU background mask (a threshold and a 49-step loop over an input that never changes)
// -- for up to 8 views per call, from the uint8 source at its own size to planar float32, bit for bit, without a host read.
// Launches (whatever the view count; a pass nobody needs is not launched):
//   1 rows     the horizontal pass of the resize: a workgroup brings the span of ONE source row its output pixels read into
//              LDS with 16-byte loads over the byte stream (premultiplying RGBA on the way), every thread produces all
//              channels of its output pixels from LDS with its own taps; writes the [Hs, W, C] uint8 intermediate
//   2 finish   the vertical pass over that intermediate (threads along x, 4 pixels = 4C bytes per thread and tap, the taps
//              of one output row are the same for the whole workgroup), un-premultiply, / 255, composite, clamp, mask;
//              writes planar [C', H, W] float32
//   3 dtu      max over channels < threshold and the running AND over the 50 rows y-49..y: one thread per column and
//              64-row segment, started 49 rows early (exact: the window never looks further back)
// The resize is integer work: the coefficient tables (22 fractional bits, built on the host in float64, one per distinct
// (in, out) and axis) arrive as device int32 [2 + ksize][out]: row 0 = first source index, row 1 = tap count, rows 2.. = taps
// (transposed, so that consecutive output pixels read consecutive words).  The device never evaluates the cubic.  A pass is
// clip8((2^21 + sum pixel * K) >> 22); the horizontal pass comes first and is stored as uint8.  A table is never trusted for
// memory safety: every source index is clamped to the row / column it belongs to.
#include "b3gs_internal.h"

#include <string.h>

namespace {

constexpr int GV = B3GS_MAX_GT_VIEWS;
constexpr int PB = 22;                       // fractional bits of a tap
constexpr int TPB = 256;
constexpr int LDS_CHUNKS = 2048;             // 16-byte chunks of a source-row span in LDS (32 KB)
constexpr int MAX_TILE = 1024;               // output pixels of one row a workgroup produces at most
constexpr int QPB = 128;                     // finish: threads (= quads of pixels) per workgroup
constexpr int DTU_WINDOW = 50;               // rows y-49..y
constexpr int DTU_SEG = 64;

struct GtTable {
  const uint8_t* src[GV];
  uint8_t* tmp[GV];                          // [Hs, W, C] (NULL: no horizontal pass for this view)
  const int32_t* tab_x[GV];
  const int32_t* tab_y[GV];
  float* image[GV];
  float* alpha[GV];
  float* bg_mask[GV];
  int32_t Hs[GV], Ws[GV], C[GV], ks_x[GV], ks_y[GV], tile[GV];
};

__device__ __forceinline__ uint32_t clip8(int32_t v) { return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v); }

// Pillow's premultiply of one RGBA word (alpha in the top byte): c' = ((c*a + 128) >> 8 + c*a + 128) >> 8
__device__ __forceinline__ uint32_t premul_word(uint32_t w) {
  const uint32_t a = w >> 24;
  uint32_t r = w & 0xff000000u;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const uint32_t t = ((w >> (8 * c)) & 255u) * a + 128u;
    r |= (((t >> 8) + t) >> 8) << (8 * c);
  }
  return r;
}

__device__ __forceinline__ uint32_t unpremul(uint32_t c, uint32_t a) {
  if (a == 0u || a == 255u) return c;
  const uint32_t d = (255u * c) / a;
  return d > 255u ? 255u : d;
}

// ---- 1: horizontal pass ------------------------------------------------------------------------------------------------
// grid (tiles of the output row, source rows, views); block TPB
template <int C>
__device__ __forceinline__ void rows_body(const GtTable& t, int v, int W, uint4* lds) {
  const int Hs = t.Hs[v], Ws = t.Ws[v], ks = t.ks_x[v], tile = t.tile[v];
  const int y = blockIdx.y;
  const int x0 = blockIdx.x * tile;
  if (y >= Hs || x0 >= W || !t.tmp[v]) return;
  const int x1 = min(x0 + tile, W);
  const int32_t* tab = t.tab_x[v];
  // the span of source pixels this tile reads (first indices are non-decreasing in x)
  int lo0 = min(max(tab[x0], 0), Ws);
  int end = min(max(tab[x1 - 1] + min(max(tab[W + x1 - 1], 0), ks), lo0), Ws);
  const size_t total = (size_t)Hs * Ws * C;                       // bytes of the image
  const size_t first = ((size_t)y * Ws + lo0) * C;                // byte offset of the span
  const size_t first16 = first & ~(size_t)15;
  const int shift = (int)(first - first16);
  int nchunks = (int)((((size_t)y * Ws + end) * C - first16 + 15) >> 4);
  nchunks = min(nchunks, LDS_CHUNKS);
  const uint8_t* src = t.src[v];
  for (int i = threadIdx.x; i < nchunks; i += TPB) {
    const size_t off = first16 + (size_t)i * 16;
    uint4 q;
    if (off + 16 <= total) {
      q = *reinterpret_cast<const uint4*>(src + off);
    } else {                                                      // the last bytes of the image
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (int b = 0; b < 16; b++)
        if (off + b < total) w[b >> 2] |= (uint32_t)src[off + b] << (8 * (b & 3));
      q = make_uint4(w[0], w[1], w[2], w[3]);
    }
    if (C == 4) {                                                 // (16-byte chunks of an aligned RGBA image hold whole pixels)
      q.x = premul_word(q.x);
      q.y = premul_word(q.y);
      q.z = premul_word(q.z);
      q.w = premul_word(q.w);
    }
    lds[i] = q;
  }
  __syncthreads();
  const uint8_t* px = reinterpret_cast<const uint8_t*>(lds);
  const int span_bytes = nchunks * 16;
  uint8_t* out = t.tmp[v] + (size_t)y * W * C;
  for (int x = x0 + threadIdx.x; x < x1; x += TPB) {
    const int lo = min(max(tab[x], lo0), Ws);
    const int n = min(max(tab[W + x], 0), ks);
    int base = shift + (lo - lo0) * C;
    int32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (PB - 1);
    for (int j = 0; j < n; j++, base += C) {
      if (base + C > span_bytes) break;                           // (only a malformed table gets here)
      const int32_t k = tab[(size_t)(2 + j) * W + x];
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] += k * (int32_t)px[base + c];
    }
#pragma unroll
    for (int c = 0; c < C; c++) out[(size_t)x * C + c] = (uint8_t)clip8(acc[c] >> PB);
  }
}

__global__ void __launch_bounds__(TPB) gt_rows_kernel(GtTable t, int W) {
  __shared__ uint4 lds[LDS_CHUNKS];
  const int v = blockIdx.z;
  const int C = t.C[v];
  if (C == 1) rows_body<1>(t, v, W, lds);
  else if (C == 3) rows_body<3>(t, v, W, lds);
  else rows_body<4>(t, v, W, lds);
}

// ---- 2: vertical pass and the float statements --------------------------------------------------------------------------
// 4 pixels of one row (4C bytes) into C words; pixels >= nvalid read nothing and are zero
template <int C>
__device__ __forceinline__ void load_quad(const uint8_t* p, int nvalid, bool aligned, bool premul, uint32_t (&w)[C]) {
  if (nvalid >= 4 && aligned) {                                   // rows of a multiple of 4 bytes: a quad starts on a word
#pragma unroll
    for (int i = 0; i < C; i++) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
  } else if (nvalid >= 4) {
    memcpy(w, p, 4 * C);
  } else {
#pragma unroll
    for (int i = 0; i < C; i++) w[i] = 0u;
    for (int b = 0; b < nvalid * C; b++) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
  }
  if (C == 4 && premul) {
#pragma unroll
    for (int i = 0; i < C; i++) w[i] = premul_word(w[i]);
  }
}

// grid (quads of the output row / QPB, H, views); block QPB
template <int C>
__device__ __forceinline__ void finish_body(const GtTable& t, int v, int W, int H, int white) {
  const int y = blockIdx.y;
  const int x = (blockIdx.x * QPB + threadIdx.x) * 4;
  if (x >= W) return;
  const int nvalid = min(4, W - x);
  const int Hs = t.Hs[v];
  const bool hpass = t.tmp[v] != nullptr, vpass = t.tab_y[v] != nullptr;
  const uint8_t* in = hpass ? t.tmp[v] : t.src[v];               // [Hs, W, C] either way
  const bool resized = hpass || vpass;
  const bool premul = C == 4 && resized && !hpass;               // the horizontal pass has premultiplied already
  const bool aligned = (((size_t)W * C) & 3) == 0;                // (src and tmp start 16-byte aligned)
  uint32_t val[4 * C];                                            // byte b of the quad = channel b % C of pixel b / C
  if (vpass) {
    const int32_t* tab = t.tab_y[v];
    const int lo = min(max(tab[y], 0), Hs);
    const int n = min(min(max(tab[H + y], 0), t.ks_y[v]), Hs - lo);
    int32_t acc[4 * C];
#pragma unroll
    for (int b = 0; b < 4 * C; b++) acc[b] = 1 << (PB - 1);
    for (int j = 0; j < n; j++) {
      const int32_t k = tab[(size_t)(2 + j) * H + y];
      uint32_t w[C];
      load_quad<C>(in + ((size_t)(lo + j) * W + x) * C, nvalid, aligned, premul, w);
#pragma unroll
      for (int b = 0; b < 4 * C; b++) acc[b] += k * (int32_t)((w[b >> 2] >> (8 * (b & 3))) & 255u);
    }
#pragma unroll
    for (int b = 0; b < 4 * C; b++) val[b] = clip8(acc[b] >> PB);
  } else {
    uint32_t w[C];
    load_quad<C>(in + ((size_t)y * W + x) * C, nvalid, aligned, premul, w);
#pragma unroll
    for (int b = 0; b < 4 * C; b++) val[b] = (w[b >> 2] >> (8 * (b & 3))) & 255u;
  }
  constexpr int CO = C == 1 ? 1 : 3;                              // channels of original_image
  float img[CO][4], msk[4] = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
  for (int p = 0; p < 4; p++) {
    float m = 1.f;
    if (C == 4) {
      const uint32_t a = val[p * C + 3];
      if (resized) {
#pragma unroll
        for (int c = 0; c < 3; c++) val[p * C + c] = unpremul(val[p * C + c], a);
      }
      m = (float)a / 255.0f;
      msk[p] = m;
    }
#pragma unroll
    for (int c = 0; c < CO; c++) {
      float g = (float)val[p * C + c] / 255.0f;
      if (C == 4 && white) {                                      // gt * mask + 1 * (1 - mask): three roundings, no FMA
        const float a0 = g * m;
        const float a1 = 1.0f - m;
        g = a0 + a1;
      }
      g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);
      if (C == 4) g = g * m;
      img[c][p] = g;
    }
  }
  const size_t hw = (size_t)H * W, at = (size_t)y * W + x;
  const bool vec = nvalid == 4 && ((hw | at) & 3) == 0;           // (the planes start 16-byte aligned: checked on the host)
#pragma unroll
  for (int c = 0; c < CO; c++) {
    float* o = t.image[v] + c * hw + at;
    if (vec) *reinterpret_cast<float4*>(o) = make_float4(img[c][0], img[c][1], img[c][2], img[c][3]);
    else
      for (int p = 0; p < nvalid; p++) o[p] = img[c][p];
  }
  if (C == 4 && t.alpha[v]) {
    float* o = t.alpha[v] + at;
    if (vec) *reinterpret_cast<float4*>(o) = make_float4(msk[0], msk[1], msk[2], msk[3]);
    else
      for (int p = 0; p < nvalid; p++) o[p] = msk[p];
  }
}

__global__ void __launch_bounds__(QPB) gt_finish_kernel(GtTable t, int W, int H, int white) {
  const int v = blockIdx.z;
  const int C = t.C[v];
  if (C == 1) finish_body<1>(t, v, W, H, white);
  else if (C == 3) finish_body<3>(t, v, W, H, white);
  else finish_body<4>(t, v, W, H, white);
}

// ---- 3: DTU background mask ---------------------------------------------------------------------------------------------
// m0 = (max over channels of the final image) < thr; out[y, x] = AND of m0[max(0, y - 49) .. y, x].  `run` counts the dark
// rows that end at y; started 49 rows above the segment it is exact wherever it is compared (with min(y + 1, 50)).
// grid (W / TPB, segments of DTU_SEG rows, views); block TPB
__global__ void __launch_bounds__(TPB) gt_dtu_kernel(GtTable t, int W, int H, float thr) {
  const int v = blockIdx.z;
  const int x = blockIdx.x * TPB + threadIdx.x;
  float* out = t.bg_mask[v];
  if (x >= W || !out) return;
  const int CO = t.C[v] == 1 ? 1 : 3;
  const float* img = t.image[v];
  const size_t hw = (size_t)H * W;
  const int y0 = blockIdx.y * DTU_SEG, y1 = min(y0 + DTU_SEG, H);
  int run = 0;
  for (int y = max(y0 - (DTU_WINDOW - 1), 0); y < y1; y++) {
    float m = img[(size_t)y * W + x];
    for (int c = 1; c < CO; c++) {
      const float g = img[c * hw + (size_t)y * W + x];
      m = g > m ? g : m;
    }
    run = m < thr ? run + 1 : 0;
    if (y >= y0) out[(size_t)y * W + x] = run >= min(y + 1, DTU_WINDOW) ? 1.f : 0.f;
  }
}

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// output pixels per workgroup of the horizontal pass such that the span they read fits the LDS buffer; 0: it never fits
static int pick_tile(int Ws, int W, int C) {
  const double scale = (double)Ws / W, support = 2.0 * (scale > 1.0 ? scale : 1.0);
  // span <= (tile - 1) * scale + 2 * support + 2 pixels, plus the 15 bytes in front of an unaligned start
  const double cap_px = (double)(LDS_CHUNKS * 16 - 16) / C - 2.0 * support - 3.0;
  if (cap_px < 0.0) return 0;
  double tile = cap_px / scale + 1.0;
  if (tile > MAX_TILE) tile = MAX_TILE;
  int ti = (int)tile;
  if (ti > W) ti = W;
  return ti < 1 ? 0 : ti;
}

static int check_views(int32_t nviews, const B3gsGtView* views, int32_t H, int32_t W, const char* what) {
  if (nviews <= 0 || nviews > GV || !views || H <= 0 || W <= 0)
    return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views and a non-empty output shape are needed");
  if ((int64_t)H * W > ((int64_t)1 << 28)) return b3gs_fail(B3GS_ERR_ARG, what, "at most 2^28 output pixels per view");
  for (int i = 0; i < nviews; i++) {
    const B3gsGtView& g = views[i];
    if (g.Hs <= 0 || g.Ws <= 0 || (g.C != 1 && g.C != 3 && g.C != 4))
      return b3gs_fail(B3GS_ERR_ARG, what, "a source is [Hs, Ws, C] with C in {1, 3, 4}");
    if ((int64_t)g.Hs * g.Ws > ((int64_t)1 << 28)) return b3gs_fail(B3GS_ERR_ARG, what, "at most 2^28 source pixels per view");
    if ((g.Ws != W) != (g.tab_x != nullptr) || (g.Hs != H) != (g.tab_y != nullptr))
      return b3gs_fail(B3GS_ERR_ARG, what, "a coefficient table goes with every axis whose size changes, and with no other");
    if ((g.tab_x && g.ks_x < 1) || (g.tab_y && g.ks_y < 1)) return b3gs_fail(B3GS_ERR_ARG, what, "a table has at least one tap row");
    if (g.tab_x && pick_tile(g.Ws, W, g.C) == 0)
      return b3gs_fail(B3GS_ERR_ARG, what, "horizontal scale too large: the taps of one output pixel do not fit the LDS buffer");
  }
  return B3GS_OK;
}

}  // namespace

extern "C" size_t b3gs_gt_workspace_bytes(int32_t nviews, const B3gsGtView* views, int32_t H, int32_t W) {
  if (nviews <= 0 || nviews > GV || !views || W <= 0) return 0;
  size_t total = 256;
  for (int i = 0; i < nviews; i++)
    if (views[i].Ws != W && views[i].Hs > 0 && views[i].C > 0) total += align256((size_t)views[i].Hs * W * views[i].C);
  return total;
}

extern "C" int b3gs_prepare_gt_batch(int32_t nviews, const B3gsGtView* views, int32_t H, int32_t W, int32_t white_background,
                                     float dtu_threshold, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_prepare_gt_batch";
  const int rc = check_views(nviews, views, H, W, what);
  if (rc != B3GS_OK) return rc;
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (!(dtu_threshold >= 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the DTU threshold is >= 0 (0: no mask)");
  GtTable t = {};
  char* ws = static_cast<char*>(workspace);
  size_t off = 0;
  int max_hs = 0, max_tiles = 0;
  bool any_dtu = false;
  for (int i = 0; i < nviews; i++) {
    const B3gsGtView& g = views[i];
    if (!g.src || !g.image) return b3gs_fail(B3GS_ERR_ARG, what, "src and image are needed for every view");
    if (((uintptr_t)g.src & 15) || ((uintptr_t)g.image & 15) || ((uintptr_t)g.alpha & 15))
      return b3gs_fail(B3GS_ERR_ARG, what, "src, image and alpha must be 16-byte aligned");
    if (g.C == 4 && !g.alpha) return b3gs_fail(B3GS_ERR_ARG, what, "an RGBA source needs the alpha output");
    if (dtu_threshold > 0.f && !g.bg_mask) return b3gs_fail(B3GS_ERR_ARG, what, "a DTU threshold needs the bg_mask output");
    t.src[i] = g.src;
    t.Hs[i] = g.Hs;
    t.Ws[i] = g.Ws;
    t.C[i] = g.C;
    t.tab_x[i] = g.tab_x;
    t.tab_y[i] = g.tab_y;
    t.ks_x[i] = g.ks_x;
    t.ks_y[i] = g.ks_y;
    t.image[i] = g.image;
    t.alpha[i] = g.C == 4 ? g.alpha : nullptr;
    t.bg_mask[i] = dtu_threshold > 0.f ? g.bg_mask : nullptr;
    any_dtu = any_dtu || t.bg_mask[i];
    if (g.tab_x) {
      t.tmp[i] = reinterpret_cast<uint8_t*>(ws + off);
      off += align256((size_t)g.Hs * W * g.C);
      t.tile[i] = pick_tile(g.Ws, W, g.C);
      max_hs = g.Hs > max_hs ? g.Hs : max_hs;
      const int tiles = (W + t.tile[i] - 1) / t.tile[i];
      max_tiles = tiles > max_tiles ? tiles : max_tiles;
    }
  }
  if (max_hs > 65535 || H > 65535) return b3gs_fail(B3GS_ERR_ARG, what, "at most 65535 rows");
  hipStream_t s = (hipStream_t)stream;
  if (max_tiles > 0) hipLaunchKernelGGL(gt_rows_kernel, dim3(max_tiles, max_hs, nviews), dim3(TPB), 0, s, t, W);
  const int quads = (W + 3) / 4;
  hipLaunchKernelGGL(gt_finish_kernel, dim3((quads + QPB - 1) / QPB, H, nviews), dim3(QPB), 0, s, t, W, H, white_background ? 1 : 0);
  if (any_dtu)
    hipLaunchKernelGGL(gt_dtu_kernel, dim3((W + TPB - 1) / TPB, (H + DTU_SEG - 1) / DTU_SEG, nviews), dim3(TPB), 0, s, t, W, H,
                       dtu_threshold);
  return b3gs_launch_status(what);
}
