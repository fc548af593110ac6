// LPIPS (VGG16, version 0.1) of held-out views (added to ABI 18): the third number of the reference's metrics.py:103-117.
//   lpipsPyTorch/modules/networks.py:50-63,88-96  z-score, VGG16 `features` up to relu5_3, taps after relu1_2 .. relu5_3
//   lpipsPyTorch/modules/utils.py:6-8             f / (sqrt(sum_c f^2) + 1e-10)
//   lpipsPyTorch/modules/lpips.py:30-36           sum_c w_c (fx - fy)^2, mean over the pixels, sum over the five layers
// Thirteen 3x3 convolutions as implicit GEMMs on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf
// chain; one chain per chunk of four input channels, the chunk sums added in order), four floor-mode 2x2 max-pools, five
// taps.  Activations are planar [image, channel, y, x] float32; the 2 n images of n pairs run together (x_0 .. x_{n-1},
// y_0 .. y_{n-1}).  A tap runs right after its layer, so no tap features are kept.
// The tap is fp64 from the float32 features; its pixel sum is per-workgroup partials folded in index order (no float atomics):
// a pair has the same bits alone and at any position of a batch.
#include "b3gs_internal.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NCONV = B3GS_LPIPS_CONVS;   // 13
constexpr int NTAP = B3GS_LPIPS_TAPS;     // 5
constexpr int TPB = 256;
constexpr int NT = 128;                   // pixels of a workgroup's tile: four waves, 32 each
constexpr int TAP_BLOCKS = 256;           // most partial sums per (pair, tap)

const int CONV_CIN[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int CONV_COUT[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int CONV_GROUP[NCONV] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};   // the last convolution of a group is tapped
const int TAP_C[NTAP] = {64, 128, 256, 512, 512};

struct ConvArgs {
  const float* in0;      // images [0, nsplit): planes of Cin * HW floats each
  const float* in1;      // images [nsplit, n)
  int nsplit;
  const float* w;        // packed [Cin / CH][KCP][Cout]  (B3gsLpipsWeights)
  const float* bias;     // [Cout]
  float* out;            // [n, Cout, H, W]
  int Cin, Cout, H, W;
  int zscore;            // first layer: 0 none, 1 (x - shift) / scale, 2 the same of 2 x - 1
  float shift[3], scale[3];
};

// One workgroup: 32 TM output channels x 128 pixels (linear pixel index y W + x of ONE image), K = 9 Cin in chunks of CH input
// channels: k = 9 c + 3 ky + kx inside a chunk.  A chunk's weights [KCP][32 TM] and its im2col tile [KCP][128] (zero outside
// the image and beyond HW) are staged in LDS; wave w owns pixels 32 w .. 32 w + 31 and all 32 TM channels.
// MFMA operands (one VGPR each): lane l gives A[row = l & 31][k = l >> 5] and B[k = l >> 5][col = l & 31]; accumulator register
// r of lane l is D[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31].  Rows are output channels, columns pixels.
template <int TM, int CH>
__global__ void __launch_bounds__(TPB) conv3x3_kernel(ConvArgs a) {
  constexpr int KC = 9 * CH, KCP = (KC + 1) & ~1, MT = 32 * TM;
  __shared__ float As[KCP * MT];
  __shared__ float Bs[KCP * NT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int HW = a.H * a.W;
  const int p0 = blockIdx.x * NT, co0 = blockIdx.y * MT, img = blockIdx.z;
  const float* __restrict__ in = img < a.nsplit ? a.in0 + (size_t)img * a.Cin * HW : a.in1 + (size_t)(img - a.nsplit) * a.Cin * HW;
  // the pixel this thread stages: column j of the im2col tile, rows (tid >> 7) + 2 i
  const int j = tid & (NT - 1), khalf = tid >> 7;
  const int p = p0 + j;
  const bool pin = p < HW;
  const int py = pin ? p / a.W : 0, px = pin ? p - py * a.W : 0;

  // blocked sum over K: every chunk's MFMA chain starts from 0 and its result is added to `tot` in chunk order (an add per
  // chunk instead of one 9 Cin long chain: the rounding error grows with the number of chunks, not with K)
  f32x16 tot[TM];
#pragma unroll
  for (int t = 0; t < TM; t++)
#pragma unroll
    for (int e = 0; e < 16; e++) tot[t][e] = 0.f;

  const int nchunks = a.Cin / CH;
  for (int ch = 0; ch < nchunks; ch++) {
    __syncthreads();
    const float* __restrict__ wsrc = a.w + (size_t)ch * KCP * a.Cout + co0;
    for (int idx = tid; idx < KCP * MT; idx += TPB) {
      const int k = idx / MT, m = idx - k * MT;
      As[idx] = wsrc[(size_t)k * a.Cout + m];
    }
#pragma unroll 4
    for (int i = 0; i < KCP / 2; i++) {
      const int k = 2 * i + khalf;
      const int c = k / 9, t = k - 9 * c, ky = t / 3, kx = t - 3 * ky;
      const int y = py + ky - 1, x = px + kx - 1;
      float v = 0.f;
      if (k < KC && pin && y >= 0 && y < a.H && x >= 0 && x < a.W) {
        const int cc = ch * CH + c;
        v = in[(size_t)cc * HW + y * a.W + x];
        if constexpr (CH == 3) {           // the first layer (networks.py:50-51); the padding stays zero AFTER this step
          if (a.zscore == 2) {
            v = 2.f * v;
            v = v - 1.f;
          }
          if (a.zscore) {
            v = v - (c == 0 ? a.shift[0] : c == 1 ? a.shift[1] : a.shift[2]);
            v = v / (c == 0 ? a.scale[0] : c == 1 ? a.scale[1] : a.scale[2]);   // IEEE division
          }
        }
      }
      Bs[k * NT + j] = v;
    }
    __syncthreads();
    f32x16 acc[TM];
#pragma unroll
    for (int t = 0; t < TM; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[t][e] = 0.f;
#pragma unroll 2
    for (int kk = 0; kk < KCP; kk += 2) {
      const float b = Bs[(kk + h) * NT + wave * 32 + r];
#pragma unroll
      for (int t = 0; t < TM; t++) {
        const float av = As[(kk + h) * MT + t * 32 + r];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < TM; t++) tot[t] = tot[t] + acc[t];
  }
  // bias + ReLU; lane l writes pixel p0 + 32 wave + (l & 31) of 16 TM channels
  const int pw = p0 + wave * 32 + r;
  if (pw < HW) {
    float* __restrict__ o = a.out + (size_t)img * a.Cout * HW + pw;
#pragma unroll
    for (int t = 0; t < TM; t++)
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const int co = co0 + t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float v = tot[t][e] + a.bias[co];
        o[(size_t)co * HW] = v > 0.f ? v : 0.f;
      }
  }
}

// 2x2 stride-2 max-pool, floor mode: an odd last row or column is dropped.  planes = images * channels.
__global__ void __launch_bounds__(TPB) maxpool_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t planes, int H,
                                                      int W, int Ho, int Wo) {
  const int64_t total = planes * Ho * Wo;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (int64_t)gridDim.x * TPB) {
    const int xo = (int)(i % Wo);
    const int64_t q = i / Wo;
    const int yo = (int)(q % Ho);
    const int64_t pl = q / Ho;
    const float* s = in + (pl * H + 2 * yo) * W + 2 * xo;
    out[i] = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[W], s[W + 1]));
  }
}

static int tap_blocks(int hw) {
  const int b = (hw + TPB - 1) / TPB;
  return b < 1 ? 1 : (b > TAP_BLOCKS ? TAP_BLOCKS : b);
}

// grid (blocks, pairs): thread = pixel (stride blocks * 256).  fp64 from the float32 features:
//   nx = sqrt(sum_c fx^2) + 1e-10, ny likewise;  d = fx / nx - fy / ny;  s += w_c d^2  (c ascending)
// -> one partial per workgroup at part[(pair * NTAP + tap) * TAP_BLOCKS + block]
__global__ void __launch_bounds__(TPB) tap_partial_kernel(const float* __restrict__ feat, int npairs, int C, int hw,
                                                          const float* __restrict__ lin, int tap, double* __restrict__ part) {
  const int pair = blockIdx.y;
  const float* __restrict__ fx = feat + (size_t)pair * C * hw;
  const float* __restrict__ fy = feat + (size_t)(npairs + pair) * C * hw;
  double s = 0.0;
  for (int p = blockIdx.x * TPB + threadIdx.x; p < hw; p += gridDim.x * TPB) {
    double sx = 0.0, sy = 0.0;
    for (int c = 0; c < C; c++) {
      const double vx = (double)fx[(size_t)c * hw + p], vy = (double)fy[(size_t)c * hw + p];
      sx += vx * vx;
      sy += vy * vy;
    }
    const double nx = sqrt(sx) + 1e-10, ny = sqrt(sy) + 1e-10;
    double acc = 0.0;
    for (int c = 0; c < C; c++) {
      const double d = (double)fx[(size_t)c * hw + p] / nx - (double)fy[(size_t)c * hw + p] / ny;
      acc += (double)lin[c] * (d * d);
    }
    s += acc;
  }
  __shared__ double red[TPB / 64][1];
  const double q[1] = {s};
  b3gs_block_sum_f64<TPB>(q, red, part + ((size_t)pair * NTAP + tap) * TAP_BLOCKS + blockIdx.x);
}

struct FoldArgs {
  int nblocks[NTAP];
  double hw[NTAP];
};
// one wave per (pair, tap): the partials in index order, then the mean over the layer's pixels
__global__ void __launch_bounds__(64) tap_fold_kernel(const double* __restrict__ part, FoldArgs f, double* __restrict__ out) {
  const int pair = blockIdx.x, tap = blockIdx.y;
  const double a = b3gs_wave_fold_f64(part + ((size_t)pair * NTAP + tap) * TAP_BLOCKS, f.nblocks[tap], 1);
  if (threadIdx.x == 0) out[(size_t)pair * NTAP + tap] = a / f.hw[tap];
}

struct Plan {
  size_t act_floats;     // one of the two activation buffers (floats), for n images
  size_t part_off;       // byte offset of the tap partials
  size_t bytes;
};
static Plan plan(int nimages, int npairs, int H, int W) {
  Plan p;
  p.act_floats = (size_t)nimages * 64 * (size_t)H * (size_t)W;
  p.part_off = 2 * b3gs_align256(p.act_floats * sizeof(float));
  p.bytes = p.part_off + b3gs_align256((size_t)(npairs > 0 ? npairs : 1) * NTAP * TAP_BLOCKS * sizeof(double));
  return p;
}

static void launch_conv(const ConvArgs& a, int n, hipStream_t s) {
  const int HW = a.H * a.W;
  const int gx = (HW + NT - 1) / NT;
  if (a.Cin == 3)
    hipLaunchKernelGGL((conv3x3_kernel<2, 3>), dim3(gx, a.Cout / 64, n), dim3(TPB), 0, s, a);
  else if (a.Cout == 64)
    hipLaunchKernelGGL((conv3x3_kernel<2, 4>), dim3(gx, a.Cout / 64, n), dim3(TPB), 0, s, a);
  else
    hipLaunchKernelGGL((conv3x3_kernel<4, 4>), dim3(gx, a.Cout / 128, n), dim3(TPB), 0, s, a);
}

// The network over n images (x: the first nsplit of them, y: the rest).  feats != null: tapped layers are written there;
// out != null: the taps of npairs = n / 2 pairs.
static void run(int n, int nsplit, const float* x, const float* y, int H, int W, const B3gsLpipsWeights* wt, int normalize,
                float* const* feats, double* out, void* workspace, hipStream_t s) {
  const Plan pl = plan(n, out ? n / 2 : 0, H, W);
  char* base = static_cast<char*>(workspace);
  float* buf[2] = {reinterpret_cast<float*>(base), reinterpret_cast<float*>(base + pl.part_off / 2)};
  double* part = reinterpret_cast<double*>(base + pl.part_off);
  FoldArgs fold = {};
  const float* cur = nullptr;
  int which = 0, h = H, w = W;
  for (int l = 0; l < NCONV; l++) {
    const int g = CONV_GROUP[l];
    const bool tapped = l + 1 == NCONV || CONV_GROUP[l + 1] != g;
    if (l > 0 && CONV_GROUP[l - 1] != g) {               // the pool in front of groups 2..5
      const int ho = h / 2, wo = w / 2;
      const int64_t planes = (int64_t)n * CONV_CIN[l], total = planes * ho * wo;
      const int64_t nb = (total + TPB - 1) / TPB;
      hipLaunchKernelGGL(maxpool_kernel, dim3((unsigned)(nb > 65536 ? 65536 : nb)), dim3(TPB), 0, s, cur, buf[which], planes, h, w, ho, wo);
      cur = buf[which];
      which ^= 1;
      h = ho;
      w = wo;
    }
    ConvArgs a = {};
    a.in0 = l == 0 ? x : cur;
    a.in1 = l == 0 ? y : nullptr;
    a.nsplit = l == 0 ? nsplit : n;
    a.w = wt->conv_w[l];
    a.bias = wt->conv_b[l];
    a.out = (tapped && feats) ? feats[g] : buf[which];
    a.Cin = CONV_CIN[l];
    a.Cout = CONV_COUT[l];
    a.H = h;
    a.W = w;
    a.zscore = l == 0 ? (normalize ? 2 : 1) : 0;
    for (int c = 0; c < 3; c++) {
      a.shift[c] = wt->shift[c];
      a.scale[c] = wt->scale[c];
    }
    launch_conv(a, n, s);
    cur = a.out;
    if (a.out == buf[which]) which ^= 1;
    if (tapped && out) {
      const int hw = h * w, nb = tap_blocks(hw);
      fold.nblocks[g] = nb;
      fold.hw[g] = (double)hw;
      hipLaunchKernelGGL(tap_partial_kernel, dim3(nb, n / 2), dim3(TPB), 0, s, cur, n / 2, TAP_C[g], hw, wt->lin[g], g, part);
    }
  }
  if (out) hipLaunchKernelGGL(tap_fold_kernel, dim3(n / 2, NTAP), dim3(64), 0, s, (const double*)part, fold, out);
}

static const char* check_common(int32_t n, int32_t H, int32_t W, const B3gsLpipsWeights* wt, const void* workspace) {
  if (n < 1 || n > B3GS_LPIPS_MAX_PAIRS) return "1..8 pairs (or images) per call";
  if (H < B3GS_LPIPS_MIN_SIDE || W < B3GS_LPIPS_MIN_SIDE) return "H and W must be at least 16: the fifth layer would be empty";
  if ((int64_t)H * W > (int64_t)1 << 24) return "at most 2^24 pixels per image";
  if (!wt || !workspace) return "NULL weights or workspace";
  for (int l = 0; l < NCONV; l++)
    if (!wt->conv_w[l] || !wt->conv_b[l]) return "NULL convolution weights";
  for (int c = 0; c < 3; c++)
    if (!(wt->scale[c] != 0.f)) return "a scale of zero";
  return nullptr;
}

}  // namespace

extern "C" size_t b3gs_lpips_workspace_bytes(int32_t npairs, int32_t H, int32_t W) {
  if (npairs < 1 || npairs > B3GS_LPIPS_MAX_PAIRS || H < B3GS_LPIPS_MIN_SIDE || W < B3GS_LPIPS_MIN_SIDE ||
      (int64_t)H * W > (int64_t)1 << 24)
    return 0;
  return plan(2 * npairs, npairs, H, W).bytes;
}

extern "C" int b3gs_lpips_batch(int32_t npairs, const float* x, const float* y, int32_t H, int32_t W, const B3gsLpipsWeights* weights,
                                int32_t normalize, double* out, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_lpips_batch";
  if (const char* msg = check_common(npairs, H, W, weights, workspace)) return b3gs_fail(B3GS_ERR_ARG, what, msg);
  if (!x || !y || !out) return b3gs_fail(B3GS_ERR_ARG, what, "NULL x, y or out");
  for (int g = 0; g < NTAP; g++)
    if (!weights->lin[g]) return b3gs_fail(B3GS_ERR_ARG, what, "NULL lin weights");
  run(2 * npairs, npairs, x, y, H, W, weights, normalize, nullptr, out, workspace, (hipStream_t)stream);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_lpips_features(int32_t nimages, const float* x, int32_t H, int32_t W, const B3gsLpipsWeights* weights,
                                   int32_t normalize, float* const* feats, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_lpips_features";
  if (const char* msg = check_common(nimages, H, W, weights, workspace)) return b3gs_fail(B3GS_ERR_ARG, what, msg);
  if (!x || !feats) return b3gs_fail(B3GS_ERR_ARG, what, "NULL x or feats");
  for (int g = 0; g < NTAP; g++)
    if (!feats[g]) return b3gs_fail(B3GS_ERR_ARG, what, "NULL feature map");
  run(nimages, nimages, x, nullptr, H, W, weights, normalize, feats, nullptr, workspace, (hipStream_t)stream);
  return b3gs_launch_status(what);
}
