// The matcher cloud (ABI 14): everything the reference's submodules/dense_matcher/triangulate.py does AFTER the dense matcher
// has produced its keypoints --
//   b3gs_triangulate_matches   lines 165-219: DLT of every match (fp64, one-sided Jacobi SVD of the 4x4 system, as OpenCV's
//                              triangulatePoints solves it), both projections in the operation order of point_world2depth
//                              (fp32, no FMA), the reprojection filter, the frame filter, the bilinear colour; kept rows
//                              written densely IN INPUT ORDER
//   b3gs_background_sheet      lines 221-238: the world point of depth 10 behind every (near-)white pixel of a DTU view
//   b3gs_cloud_grow_round      lines 264-379: one round of the growth loop
// Compaction (the first two): every thread leaves a 16-byte record (x, y, z, rgb | keep << 24) and every 256-thread block its
// kept count; one block scans the block counts; the third kernel ranks the records inside a block with a ballot.  No atomics
// pick a slot, so the order of the output is the order of the input.
//
// The growth round is two launches:
//   1 ssim     one WAVE per candidate c = seed + noise * alpha.  Lane 0's projection into the two views decides patch_mask;
//              a wave whose candidate leaves either frame exits before it samples anything (ssim * 0 >= threshold is false).
//              A live wave samples the 2 x 121 patch positions (lane l: positions l and l + 64) from the uint8 images with the
//              arithmetic of grid_sample(bilinear, zeros, align_corners=False) on image / 255, accumulates the five windowed
//              sums per channel in fp64 (the fp32 samples enter exactly; the cancellation in E[x^2] - mu^2 is where the
//              reference's own fp32 result is noisy), folds them across the wave and forms _ssim_v2 and its channel mean.
//              A selected candidate is added to the count grids of the round's two views at once.
//   2 append   ONE workgroup of 1024 threads walks the candidates in order, 1024 at a time: a selected candidate is accepted
//              when in both views its lookup in an all-ones mask is non-zero and its grid cell holds <= 2 points (itself and
//              this round's other selected candidates included, as torch.unique over cat(points_all, new_points) counts
//              them); a ballot scan gives the accepted ones consecutive slots behind *length.  Rejected ones leave the two
//              grids again, accepted ones enter the grids of the other views: after the round every grid holds exactly the
//              cloud.  *length keeps counting past `capacity` (nothing is written there, the overflow word is set), so a run
//              that overflowed still ends with the length it needs and the host replays it once with larger buffers.
// The count grids replace the reference's two torch.unique(round(uv), dim=0) over the whole cloud.  A count is only read
// at a new point whose all-ones lookup is non-zero: its unnormalised coordinate u * W / (W - 1) - 0.5 lies in (-1, W), so
// u lies in (-0.5 + 1 / (2W), W - 0.5 - 1 / (2W)) and rintf(u) in [0, W - 1].  A grid of [-1, W] x [-1, H] cells -- one cell
// of margin -- therefore holds every count that is read; a point that rounds outside it is not counted.  The kernel checks
// this (bit 1 of the overflow word) instead of trusting it.
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int APPEND_TPB = 1024;
constexpr int PATCH = 11;
constexpr int NPATCH = PATCH * PATCH;

struct Rec {            // one candidate row of a compaction
  float x, y, z;
  uint32_t rgbk;        // r | g << 8 | b << 16 | keep << 24
};

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int64_t nblocks(int64_t n) { return (n + TPB - 1) / TPB; }

// ---- fp32 statements, in the reference's order (the Makefile compiles with -ffp-contract=off) ---------------------------
// matmul(M[:3,:3], p) + M[:3,3] of a row-major 4x4
__device__ __forceinline__ void rot_trans(const float* M, float px, float py, float pz, float& x, float& y, float& z) {
  x = (M[0] * px + M[1] * py + M[2] * pz) + M[3];
  y = (M[4] * px + M[5] * py + M[6] * pz) + M[7];
  z = (M[8] * px + M[9] * py + M[10] * pz) + M[11];
}

// point_world2depth: K @ (R p + t), uv = xy / z
__device__ __forceinline__ void world2uv(const float* K, const float* M, float px, float py, float pz, float& u, float& v) {
  float x, y, z;
  rot_trans(M, px, py, pz, x, y, z);
  const float ix = K[0] * x + K[1] * y + K[2] * z;
  const float iy = K[3] * x + K[4] * y + K[5] * z;
  const float iz = K[6] * x + K[7] * y + K[8] * z;
  u = ix / iz;
  v = iy / iz;
}

// map_points_to_image: uv = xy / z, *= focal, += center
__device__ __forceinline__ void map_to_image(const float* M, float px, float py, float pz, float fx, float fy, float cx, float cy,
                                             float& u, float& v) {
  float x, y, z;
  rot_trans(M, px, py, pz, x, y, z);
  u = (x / z) * fx + cx;
  v = (y / z) * fy + cy;
}

// grid_sample's unnormalisation (align_corners=False) of a normalised coordinate
__device__ __forceinline__ float unnormalize(float g, int size) { return ((g + 1.0f) * (float)size - 1.0f) / 2.0f; }

// bilinear, zeros padding, of a uint8 [H,W,3] image at unnormalised (ix, iy), corners in grid_sample's order nw, ne, sw, se;
// DIV255: every channel value is divided by 255 BEFORE it is weighted, as sampling `image / 255.0` does
template <bool DIV255>
__device__ __forceinline__ void bilinear3(const uint8_t* img, int W, int H, float ix, float iy, float (&out)[3]) {
  out[0] = out[1] = out[2] = 0.0f;
  if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) return;      // (NaN: nothing is in bounds)
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
  const float w[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)};
  const int xs[4] = {x0, x1, x0, x1}, ys[4] = {y0, y0, y1, y1};
#pragma unroll
  for (int k = 0; k < 4; k++) {                                                   // nw, ne, sw, se
    if (xs[k] >= 0 && xs[k] < W && ys[k] >= 0 && ys[k] < H) {
      const uint8_t* p = img + ((size_t)ys[k] * W + xs[k]) * 3;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float val = DIV255 ? (float)p[c] / 255.0f : (float)p[c];
        out[c] = out[c] + val * w[k];
      }
    }
  }
}

// the same lookup in an all-ones image: is the result non-zero?
__device__ __forceinline__ bool ones_lookup(int W, int H, float ix, float iy) {
  if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) return false;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0;
  const float fx1 = fx0 + 1.0f, fy1 = fy0 + 1.0f;
  const float w[4] = {(fx1 - ix) * (fy1 - iy), (ix - fx0) * (fy1 - iy), (fx1 - ix) * (iy - fy0), (ix - fx0) * (iy - fy0)};
  const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (xs[k] >= 0 && xs[k] < W && ys[k] >= 0 && ys[k] < H) s = s + w[k];
  return s != 0.0f;
}

// (uv / (W - 1, H - 1)) * 2 - 1, unnormalised again
__device__ __forceinline__ void frame_coords(float u, float v, int W, int H, float& ix, float& iy) {
  ix = unnormalize((u / (float)(W - 1)) * 2.0f - 1.0f, W);
  iy = unnormalize((v / (float)(H - 1)) * 2.0f - 1.0f, H);
}

// cell of the count grid ([H + 2, W + 2], one cell of margin), or -1
__device__ __forceinline__ int grid_cell(float u, float v, int W, int H) {
  const float ru = rintf(u), rv = rintf(v);                                       // round half to even, as torch.round
  if (!(ru >= -1.0f && ru <= (float)W && rv >= -1.0f && rv <= (float)H)) return -1;
  return ((int)rv + 1) * (W + 2) + ((int)ru + 1);
}

// ---- DLT ---------------------------------------------------------------------------------------------------------------------
// right singular vector of the smallest singular value of the 4x4 A (rows x*P[2] - P[0], y*P[2] - P[1] of both views): one-sided
// Jacobi (Hestenes) on A itself -- no A^T A, so the error is eps * cond, not eps * cond^2
__device__ void smallest_right_singular(double (&A)[4][4], double (&X)[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 30; sweep++) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
      for (int q = p + 1; q < 4; q++) {
        double a = 0, b = 0, g = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          a += A[r][p] * A[r][p];
          b += A[r][q] * A[r][q];
          g += A[r][p] * A[r][q];
        }
        if (fabs(g) <= 1e-15 * sqrt(a * b) || g == 0.0) continue;
        changed = true;
        const double zeta = (b - a) / (2.0 * g);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const double ap = A[r][p], aq = A[r][q];
          A[r][p] = c * ap - s * aq;
          A[r][q] = s * ap + c * aq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - s * vq;
          V[r][q] = s * vp + c * vq;
        }
      }
    if (!changed) break;
  }
  int best = 0;
  double bn = 0;
  for (int j = 0; j < 4; j++) {
    double n = 0;
    for (int r = 0; r < 4; r++) n += A[r][j] * A[r][j];
    if (j == 0 || n < bn) {
      bn = n;
      best = j;
    }
  }
  for (int r = 0; r < 4; r++) X[r] = V[r][best];
}

struct TriArgs {
  int N, W, H;
  const float *proj_ref, *proj_src, *K, *w2c_ref, *w2c_src, *kp_ref, *kp_src;
  const uint8_t* image;
  float thr;
  Rec* rec;
  int32_t* block_count;
};

__device__ __forceinline__ void block_count_store(bool keep, int32_t* block_count) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  int total;
  b3gs_block_rank<TPB, 1>(keep, wave_n, &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TPB) triangulate_kernel(TriArgs a) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  bool keep = false;
  if (i < a.N) {
    const float x0 = a.kp_ref[2 * i], y0 = a.kp_ref[2 * i + 1], x1 = a.kp_src[2 * i], y1 = a.kp_src[2 * i + 1];
    double A[4][4], X[4];
    for (int k = 0; k < 4; k++) {
      A[0][k] = (double)x0 * (double)a.proj_ref[8 + k] - (double)a.proj_ref[k];
      A[1][k] = (double)y0 * (double)a.proj_ref[8 + k] - (double)a.proj_ref[4 + k];
      A[2][k] = (double)x1 * (double)a.proj_src[8 + k] - (double)a.proj_src[k];
      A[3][k] = (double)y1 * (double)a.proj_src[8 + k] - (double)a.proj_src[4 + k];
    }
    smallest_right_singular(A, X);
    // the homogeneous point leaves triangulatePoints as float32 and is divided by its last component in float32
    const float hx = (float)X[0], hy = (float)X[1], hz = (float)X[2], hw = (float)X[3];
    const float px = hx / hw, py = hy / hw, pz = hz / hw;
    float ur, vr, us, vs;
    world2uv(a.K, a.w2c_ref, px, py, pz, ur, vr);
    world2uv(a.K, a.w2c_src, px, py, pz, us, vs);
    const float dr0 = ur - x0, dr1 = vr - y0, ds0 = us - x1, ds1 = vs - y1;
    const float nr = sqrtf(dr0 * dr0 + dr1 * dr1), ns = sqrtf(ds0 * ds0 + ds1 * ds1);
    const float wm = (float)(a.W - 1), hm = (float)(a.H - 1);
    keep = nr < a.thr && ns < a.thr && ur >= 0.0f && ur <= wm && vr >= 0.0f && vr <= hm && us >= 0.0f && us <= wm && vs >= 0.0f &&
           vs <= hm;
    Rec r = {px, py, pz, 0u};
    if (keep) {
      float ix, iy, col[3];
      frame_coords(ur, vr, a.W, a.H, ix, iy);
      bilinear3<false>(a.image, a.W, a.H, ix, iy, col);
      uint32_t w = 1u << 24;
      for (int c = 0; c < 3; c++) {
        const float f = col[c] < 0.0f ? 0.0f : (col[c] > 255.0f ? 255.0f : col[c]);
        w |= ((uint32_t)(int)f & 255u) << (8 * c);                                // truncation, as astype(uint8)
      }
      r.rgbk = w;
    }
    a.rec[i] = r;
  }
  block_count_store(keep, a.block_count);
}

struct SheetArgs {
  int W, H;
  const uint8_t* image;
  const float *inv_kt, *c2w;
  float depth;
  Rec* rec;
  int32_t* block_count;
};

__global__ void __launch_bounds__(TPB) sheet_kernel(SheetArgs a) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  bool keep = false;
  if (i < a.W * a.H) {
    const int y = i / a.W, x = i - y * a.W;
    const uint8_t* p = a.image + (size_t)i * 3;
    const uint8_t m = max(p[0], max(p[1], p[2]));
    keep = m >= 254;
    // depth2point_cam: ndc = (x / (W-1), y / (H-1), z); cam_xy = ndc_xy * (W-1, H-1) * z; cam @ inverse(intrinsic^T)
    const float z = a.depth;
    const float wm = (float)(a.W - 1), hm = (float)(a.H - 1);
    const float qx = (((float)x / wm) * wm) * z, qy = (((float)y / hm) * hm) * z;
    const float* Mi = a.inv_kt;
    const float c0 = qx * Mi[0] + qy * Mi[3] + z * Mi[6];
    const float c1 = qx * Mi[1] + qy * Mi[4] + z * Mi[7];
    const float c2 = qx * Mi[2] + qy * Mi[5] + z * Mi[8];
    // [cam, 1] @ c2w^T
    const float* E = a.c2w;
    Rec r;
    r.x = c0 * E[0] + c1 * E[1] + c2 * E[2] + E[3];
    r.y = c0 * E[4] + c1 * E[5] + c2 * E[6] + E[7];
    r.z = c0 * E[8] + c1 * E[9] + c2 * E[10] + E[11];
    r.rgbk = keep ? 0x01ffffffu : 0u;
    a.rec[i] = r;
  }
  block_count_store(keep, a.block_count);
}

// one block: exclusive scan of the block counts in place, the total to *count
__global__ void __launch_bounds__(B3GS_SCAN_TPB) scan_blocks_kernel(int32_t* block_count, int nb, int32_t* count) {
  b3gs_scan_block_sums(block_count, nb, count);
}

__global__ void __launch_bounds__(TPB) compact_kernel(const Rec* rec, int n, const int32_t* block_offset, float* points, uint8_t* colors) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int i = blockIdx.x * TPB + threadIdx.x;
  Rec r = {0.f, 0.f, 0.f, 0u};
  if (i < n) r = rec[i];
  const bool keep = (r.rgbk >> 24) != 0u;
  int total;
  const int slot = block_offset[blockIdx.x] + b3gs_block_rank<TPB, 1>(keep, wave_n, &total);
  if (!keep) return;
  if (slot >= n) return;                                                          // (cannot happen: the outputs hold n rows)
  points[3 * (size_t)slot] = r.x;
  points[3 * (size_t)slot + 1] = r.y;
  points[3 * (size_t)slot + 2] = r.z;
  colors[3 * (size_t)slot] = (uint8_t)(r.rgbk & 255u);
  colors[3 * (size_t)slot + 1] = (uint8_t)((r.rgbk >> 8) & 255u);
  colors[3 * (size_t)slot + 2] = (uint8_t)((r.rgbk >> 16) & 255u);
}

// ---- growth ----------------------------------------------------------------------------------------------------------------
struct GrowArgs {
  B3gsCloudGrow io;
  uint8_t* sel;        // [candidates]
  float* uv;           // [candidates, 4] ref u, v, src u, v of the selected candidates
};

__device__ __forceinline__ void candidate_of(const B3gsCloudGrow& g, int c, float& px, float& py, float& pz) {
  const int i = c / g.n_samples;
  int s = g.seed_idx[i];
  s = s < 0 ? 0 : (s >= g.n_start ? g.n_start - 1 : s);
  const float* sp = g.points + 3 * (size_t)s;
  const float* nz = g.noise + 3 * (size_t)c;
  px = __fadd_rn(sp[0], __fmul_rn(nz[0], g.alpha));
  py = __fadd_rn(sp[1], __fmul_rn(nz[1], g.alpha));
  pz = __fadd_rn(sp[2], __fmul_rn(nz[2], g.alpha));
}

// grid (n_views, blocks of the starting cloud)
__global__ void __launch_bounds__(TPB) grow_count_kernel(B3gsCloudGrow g) {
  const int v = blockIdx.x;
  const int i = blockIdx.y * TPB + threadIdx.x;
  if (i >= g.n_start) return;
  float u, w;
  map_to_image(g.w2c + 16 * v, g.points[3 * (size_t)i], g.points[3 * (size_t)i + 1], g.points[3 * (size_t)i + 2], g.fx, g.fy, g.cx,
               g.cy, u, w);
  const int cell = grid_cell(u, w, g.W, g.H);
  if (cell >= 0) atomicAdd(g.grids + (size_t)v * (g.H + 2) * (g.W + 2) + cell, 1);
}

// one wave per candidate; block = 4 waves
__global__ void __launch_bounds__(TPB) grow_ssim_kernel(GrowArgs a) {
  const B3gsCloudGrow& g = a.io;
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (TPB / B3GS_WAVE) + (threadIdx.x >> 6);
  const int ncand = g.n_seeds * g.n_samples;
  if (c >= ncand) return;
  float px, py, pz, ur, vr, us, vs;
  candidate_of(g, c, px, py, pz);
  map_to_image(g.w2c + 16 * g.ref, px, py, pz, g.fx, g.fy, g.cx, g.cy, ur, vr);
  map_to_image(g.w2c + 16 * g.src, px, py, pz, g.fx, g.fy, g.cx, g.cy, us, vs);
  const float Wf = (float)g.W, Hf = (float)g.H;
  const bool live = ur >= 0.0f && ur < Wf && vr >= 0.0f && vr < Hf && us >= 0.0f && us < Wf && vs >= 0.0f && vs < Hf;
  if (!live) {                                                                    // (wave-uniform)
    if (lane == 0) {
      a.sel[c] = 0;
      if (g.debug_ssim) g.debug_ssim[c] = 0.0f;
      if (g.debug_mask) g.debug_mask[c] = 0;
    }
    return;
  }
  const uint8_t* img_r = g.images + (size_t)g.ref * g.H * g.W * 3;
  const uint8_t* img_s = g.images + (size_t)g.src * g.H * g.W * 3;
  double acc[3][5];
#pragma unroll
  for (int ch = 0; ch < 3; ch++)
#pragma unroll
    for (int k = 0; k < 5; k++) acc[ch][k] = 0.0;
  for (int p = lane; p < NPATCH; p += B3GS_WAVE) {
    const float ox = (float)(p % PATCH - PATCH / 2), oy = (float)(p / PATCH - PATCH / 2);
    const double w = (double)g.window[p];
    float xs[3], xr[3];
    // grid_normal = grid * 2 / (W, H) - 1
    bilinear3<true>(img_s, g.W, g.H, unnormalize(((us + ox) * 2.0f) / Wf - 1.0f, g.W), unnormalize(((vs + oy) * 2.0f) / Hf - 1.0f, g.H), xs);
    bilinear3<true>(img_r, g.W, g.H, unnormalize(((ur + ox) * 2.0f) / Wf - 1.0f, g.W), unnormalize(((vr + oy) * 2.0f) / Hf - 1.0f, g.H), xr);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const double x = (double)xs[ch], y = (double)xr[ch];
      acc[ch][0] += w * x;
      acc[ch][1] += w * y;
      acc[ch][2] += w * (x * x);
      acc[ch][3] += w * (y * y);
      acc[ch][4] += w * (x * y);
    }
  }
  double mean = 0.0;
#pragma unroll
  for (int ch = 0; ch < 3; ch++) {
    const double mu1 = b3gs_wave_sum(acc[ch][0]), mu2 = b3gs_wave_sum(acc[ch][1]);
    const double s1 = b3gs_wave_sum(acc[ch][2]) - mu1 * mu1, s2 = b3gs_wave_sum(acc[ch][3]) - mu2 * mu2;
    const double s12 = b3gs_wave_sum(acc[ch][4]) - mu1 * mu2;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    mean += ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
  }
  const float ssim = (float)(mean / 3.0);
  if (lane != 0) return;
  const bool sel = ssim >= g.ssim_threshold;
  a.sel[c] = sel ? 1 : 0;
  if (g.debug_ssim) g.debug_ssim[c] = ssim;
  if (g.debug_mask) g.debug_mask[c] = 1;
  if (sel) {
    a.uv[4 * (size_t)c] = ur;
    a.uv[4 * (size_t)c + 1] = vr;
    a.uv[4 * (size_t)c + 2] = us;
    a.uv[4 * (size_t)c + 3] = vs;
    const size_t gs = (size_t)(g.H + 2) * (g.W + 2);
    const int cr = grid_cell(ur, vr, g.W, g.H), cs = grid_cell(us, vs, g.W, g.H);   // (live: always inside)
    if (cr >= 0) atomicAdd(g.grids + g.ref * gs + cr, 1);
    if (cs >= 0) atomicAdd(g.grids + g.src * gs + cs, 1);
  }
}

// ONE block.  Pass 1 decides every selected candidate while the grids still hold all of them (the reference counts over
// cat(points_all, new_points) once); pass 2 ranks the accepted ones and moves the grids to "exactly the cloud".
__global__ void __launch_bounds__(APPEND_TPB) grow_append_kernel(GrowArgs a) {
  const B3gsCloudGrow& g = a.io;
  __shared__ int wave_n[APPEND_TPB / B3GS_WAVE];
  const int ncand = g.n_seeds * g.n_samples;
  const size_t gs = (size_t)(g.H + 2) * (g.W + 2);
  for (int c = threadIdx.x; c < ncand; c += APPEND_TPB) {
    if (a.sel[c] == 0) continue;
    const float ur = a.uv[4 * (size_t)c], vr = a.uv[4 * (size_t)c + 1], us = a.uv[4 * (size_t)c + 2], vs = a.uv[4 * (size_t)c + 3];
    float ixr, iyr, ixs, iys;
    frame_coords(ur, vr, g.W, g.H, ixr, iyr);
    frame_coords(us, vs, g.W, g.H, ixs, iys);
    const bool mr = ones_lookup(g.W, g.H, ixr, iyr), ms = ones_lookup(g.W, g.H, ixs, iys);
    const int cr = grid_cell(ur, vr, g.W, g.H), cs = grid_cell(us, vs, g.W, g.H);
    if ((mr && cr < 0) || (ms && cs < 0)) atomicOr(g.overflow, 2);                // the margin of the grid was not enough
    const int nr = cr >= 0 ? g.grids[g.ref * gs + cr] : 0, ns = cs >= 0 ? g.grids[g.src * gs + cs] : 0;
    a.sel[c] = (mr && ms && cr >= 0 && cs >= 0 && nr <= 2 && ns <= 2) ? 2 : 1;
  }
  __syncthreads();
  int base = *g.length;
  const uint8_t* img_r = g.images + (size_t)g.ref * g.H * g.W * 3;
  for (int c0 = 0; c0 < ncand; c0 += APPEND_TPB) {
    const int c = c0 + threadIdx.x;
    const int state = c < ncand ? a.sel[c] : 0;
    const bool acc = state == 2;
    int total;
    const int before = b3gs_block_rank<APPEND_TPB, 1>(acc, wave_n, &total);
    if (state == 1) {
      const int cr = grid_cell(a.uv[4 * (size_t)c], a.uv[4 * (size_t)c + 1], g.W, g.H);
      const int cs = grid_cell(a.uv[4 * (size_t)c + 2], a.uv[4 * (size_t)c + 3], g.W, g.H);
      if (cr >= 0) atomicSub(g.grids + g.ref * gs + cr, 1);
      if (cs >= 0) atomicSub(g.grids + g.src * gs + cs, 1);
    }
    if (acc) {
      const long long slot = (long long)base + before;
      float px, py, pz;
      candidate_of(g, c, px, py, pz);
      if (slot < g.capacity) {
        float col[3], ixr, iyr;
        frame_coords(a.uv[4 * (size_t)c], a.uv[4 * (size_t)c + 1], g.W, g.H, ixr, iyr);
        bilinear3<true>(img_r, g.W, g.H, ixr, iyr, col);
        for (int k = 0; k < 3; k++) g.colors[3 * (size_t)slot + k] = col[k] * 255.0f;
        g.points[3 * (size_t)slot] = px;
        g.points[3 * (size_t)slot + 1] = py;
        g.points[3 * (size_t)slot + 2] = pz;
      } else {
        atomicOr(g.overflow, 1);
      }
      for (int v = 0; v < g.n_views; v++) {
        if (v == g.ref || v == g.src) continue;
        float u, w;
        map_to_image(g.w2c + 16 * v, px, py, pz, g.fx, g.fy, g.cx, g.cy, u, w);
        const int cell = grid_cell(u, w, g.W, g.H);
        if (cell >= 0) atomicAdd(g.grids + v * gs + cell, 1);
      }
    }
    base += total;
    __syncthreads();                                                              // wave_n is rewritten by the next chunk
  }
  if (threadIdx.x == 0) *g.length = base;
}

}  // namespace

extern "C" size_t b3gs_cloud_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return 256 + align256((size_t)n * sizeof(Rec)) + align256((size_t)(nblocks(n) + 1) * sizeof(int32_t)) + align256((size_t)n);
}

static int launch_compaction(Rec* rec, int32_t* block_count, int n, float* points, uint8_t* colors, int32_t* count, hipStream_t s) {
  const int nb = (int)nblocks(n);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(B3GS_SCAN_TPB), 0, s, block_count, nb, count);
  if (nb > 0) hipLaunchKernelGGL(compact_kernel, dim3(nb), dim3(TPB), 0, s, (const Rec*)rec, n, (const int32_t*)block_count, points, colors);
  return 0;
}

extern "C" int b3gs_triangulate_matches(int32_t N, const float* proj_ref, const float* proj_src, const float* intrinsic,
                                        const float* w2c_ref, const float* w2c_src, const float* kp_ref, const float* kp_src,
                                        const uint8_t* image, int32_t W, int32_t H, float reproj_threshold, float* points,
                                        uint8_t* colors, int32_t* count, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_triangulate_matches";
  if (N < 0 || N > (1 << 28)) return b3gs_fail(B3GS_ERR_ARG, what, "0 .. 2^28 matches per call");
  if (W < 2 || H < 2 || (int64_t)W * H > ((int64_t)1 << 28)) return b3gs_fail(B3GS_ERR_ARG, what, "the image is at least 2 x 2 and at most 2^28 pixels");
  if (!proj_ref || !proj_src || !intrinsic || !w2c_ref || !w2c_src || !image || !count)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL matrix, image or count pointer");
  if (!(reproj_threshold > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the reprojection threshold is positive");
  if (N > 0 && (!kp_ref || !kp_src || !points || !colors)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL keypoint or output pointer");
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  TriArgs a = {N, W, H, proj_ref, proj_src, intrinsic, w2c_ref, w2c_src, kp_ref, kp_src, image, reproj_threshold,
               reinterpret_cast<Rec*>(ws), reinterpret_cast<int32_t*>(ws + align256((size_t)N * sizeof(Rec)))};
  if (N > 0) hipLaunchKernelGGL(triangulate_kernel, dim3((unsigned)nblocks(N)), dim3(TPB), 0, s, a);
  launch_compaction(a.rec, a.block_count, N, points, colors, count, s);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_background_sheet(const uint8_t* image, int32_t W, int32_t H, const float* inv_intrinsic_t, const float* c2w,
                                     float depth, float* points, uint8_t* colors, int32_t* count, void* workspace,
                                     b3gs_stream_t stream) {
  static const char* what = "b3gs_background_sheet";
  if (W < 2 || H < 2 || (int64_t)W * H > ((int64_t)1 << 28)) return b3gs_fail(B3GS_ERR_ARG, what, "the image is at least 2 x 2 and at most 2^28 pixels");
  if (!image || !inv_intrinsic_t || !c2w || !points || !colors || !count) return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!(depth > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the depth is positive");
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  const int n = W * H;
  SheetArgs a = {W, H, image, inv_intrinsic_t, c2w, depth, reinterpret_cast<Rec*>(ws),
                 reinterpret_cast<int32_t*>(ws + align256((size_t)n * sizeof(Rec)))};
  hipLaunchKernelGGL(sheet_kernel, dim3((unsigned)nblocks(n)), dim3(TPB), 0, s, a);
  launch_compaction(a.rec, a.block_count, n, points, colors, count, s);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_cloud_grow_round(const B3gsCloudGrow* io, b3gs_stream_t stream) {
  static const char* what = "b3gs_cloud_grow_round";
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "io is NULL");
  const B3gsCloudGrow& g = *io;
  if (g.h_patch_size != PATCH / 2) return b3gs_fail(B3GS_ERR_ARG, what, "h_patch_size=5 (an 11x11 window) is the only supported patch");
  if (g.W < 2 || g.H < 2 || (int64_t)g.W * g.H > ((int64_t)1 << 26)) return b3gs_fail(B3GS_ERR_ARG, what, "the images are at least 2 x 2 and at most 2^26 pixels");
  if (g.n_views < 2 || g.n_views > B3GS_CLOUD_MAX_VIEWS) return b3gs_fail(B3GS_ERR_ARG, what, "2..16 views");
  if (g.ref < 0 || g.ref >= g.n_views || g.src < 0 || g.src >= g.n_views || g.ref == g.src)
    return b3gs_fail(B3GS_ERR_ARG, what, "ref and src are two different views");
  if (g.n_seeds < 1 || g.n_samples < 1 || (int64_t)g.n_seeds * g.n_samples > (1 << 24))
    return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 2^24 candidates per round");
  if (g.n_start < 1 || g.capacity < g.n_start) return b3gs_fail(B3GS_ERR_ARG, what, "a non-empty starting cloud that fits the capacity is needed");
  if (!g.images || !g.w2c || !g.window || !g.seed_idx || !g.noise || !g.points || !g.colors || !g.length || !g.overflow || !g.grids)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!g.workspace || ((uintptr_t)g.workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (!(g.ssim_threshold > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the SSIM threshold is positive");
  hipStream_t s = (hipStream_t)stream;
  const int ncand = g.n_seeds * g.n_samples;
  char* ws = static_cast<char*>(g.workspace);
  GrowArgs a = {g, reinterpret_cast<uint8_t*>(ws + align256((size_t)ncand * sizeof(Rec))), reinterpret_cast<float*>(ws)};
  if (g.init) {
    if (hipMemsetAsync(g.grids, 0, (size_t)g.n_views * (g.H + 2) * (g.W + 2) * sizeof(int32_t), s) != hipSuccess)
      return b3gs_fail(B3GS_ERR_HIP, what, "clearing the count grids failed");
    hipLaunchKernelGGL(grow_count_kernel, dim3(g.n_views, (unsigned)nblocks(g.n_start)), dim3(TPB), 0, s, g);
  }
  hipLaunchKernelGGL(grow_ssim_kernel, dim3((ncand + TPB / B3GS_WAVE - 1) / (TPB / B3GS_WAVE)), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(grow_append_kernel, dim3(1), dim3(APPEND_TPB), 0, s, a);
  return b3gs_launch_status(what);
}
