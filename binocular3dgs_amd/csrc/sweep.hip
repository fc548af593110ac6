// The plane-sweep stereo matcher (ABI 15; binocular3dgs_amd/sweep_matcher.py): keypoint matches of a
// calibrated view pair without a network.  Per direction (a -> b and b -> a, blockIdx.y) and per node of the reference view
// (pixels 3 + i stride, row-major) --
//   1 gray      integer luma (77 R + 150 G + 29 B + 128) >> 8 of both images, as uint8 (a quarter of the float traffic)
//   2 score     one lane per node.  The node's own centred 7x7 patch is staged once in LDS ([49][64] floats, lane-minor: no bank
//               conflict), with its mean and its sum of squares.  The loop over the D inverse-depth hypotheses maps the 49 patch
//               pixels through the hypothesis' homography (wave-uniform: scalar loads), samples the other gray bilinearly through
//               the cache and forms the ZNCC from three running sums.  The four best (score, k) so far stay in registers, with
//               the scores next to the best: no per-hypothesis score array exists anywhere.  After the loop: threshold,
//               uniqueness against the best score outside k* +- 1 (among any four hypotheses at most three lie within k* +- 1),
//               three-point parabola.
//   3 check     a node with a value is projected into the other view with its refined inverse depth; the other direction's
//               node nearest to it must hold a value within cyc_steps steps of the inverse depth seen from there
//   4, 5        ordered compaction: block counts, one scan, ranked writes (as cloud.hip) -- the output is in node order
// Every float statement is written in the order of tests/sweep_ref.py (the Makefile compiles with -ffp-contract=off).
// Loads are clamped to the image: a tap outside the frame invalidates its hypothesis and reads pixel (0, 0) instead.
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 64;             // score: one wave per block, so that small images still spread over the CUs
constexpr int CTPB = 256;           // check / compact
constexpr int RADIUS = 3;
constexpr int PATCH = 2 * RADIUS + 1;
constexpr int NTAPS = PATCH * PATCH;
constexpr float NONE = -1.0f;

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Args {
  B3gsSweepPair io;
  int nx, ny, n;                    // nodes per row / column / image
  uint8_t* gray;                    // [2, H, W]
  float* rec;                       // [2, n, 2] target pixel of a kept node
  uint8_t* keep;                    // [2, n]
  int32_t* block_count;             // [2, nb + 1]
  int nb;                           // compaction blocks per direction
};

__global__ void __launch_bounds__(CTPB) gray_kernel(Args a) {
  const int i = blockIdx.x * CTPB + threadIdx.x;
  if (i >= a.io.W * a.io.H) return;
  const uint8_t* p = (blockIdx.y ? a.io.image_b : a.io.image_a) + (size_t)i * 3;
  a.gray[(size_t)blockIdx.y * a.io.W * a.io.H + i] = (uint8_t)((77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8);
}

__global__ void __launch_bounds__(TPB) score_kernel(Args a) {
  __shared__ float da[NTAPS][TPB];
  const B3gsSweepPair& g = a.io;
  const int dir = blockIdx.y, lane = threadIdx.x;
  const int node = blockIdx.x * TPB + lane;
  const bool live = node < a.n;
  const int W = g.W, H = g.H, D = g.D;
  const uint8_t* own = a.gray + (size_t)dir * W * H;
  const uint8_t* other = a.gray + (size_t)(1 - dir) * W * H;
  const float* hom = g.homographies + (size_t)dir * D * 9;
  const int nd = live ? node : 0;
  const int y = RADIUS + (nd / a.nx) * g.stride, x = RADIUS + (nd % a.nx) * g.stride;   // <= H - 4, W - 4: the patch is inside
  float sa = 0.0f;
  for (int t = 0; t < NTAPS; t++) {
    const float v = (float)own[(y + t / PATCH - RADIUS) * W + (x + t % PATCH - RADIUS)];
    da[t][lane] = v;
    sa = sa + v;
  }
  const float ma = sa / (float)NTAPS;
  float va = 0.0f;
  for (int t = 0; t < NTAPS; t++) {
    const float d = da[t][lane] - ma;
    da[t][lane] = d;
    va = va + d * d;
  }
  const float px = (float)x, py = (float)y, wm = (float)(W - 1), hm = (float)(H - 1), wc = (float)(W - 2), hc = (float)(H - 2);
  // the four best valid (score, k), best first; ties keep the smaller k in front
  float s0 = -INFINITY, s1 = -INFINITY, s2 = -INFINITY, s3 = -INFINITY;
  int k0 = -1, k1 = -1, k2 = -1, k3 = -1;
  float left = 0.0f, right = 0.0f, prev = 0.0f;
  bool lvalid = false, rvalid = false, pvalid = false;
  const bool textured = va / (float)NTAPS >= g.min_var;
  if (live && textured) {
    for (int k = 0; k < D; k++) {
      const float* h = hom + 9 * k;
      const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6], h7 = h[7], h8 = h[8];
      bool ok = true;
      float sb = 0.0f, sbb = 0.0f, cov = 0.0f;
      for (int dy = 0; dy < PATCH; dy++) {
        const float ty = py + (float)(dy - RADIUS);
#pragma unroll
        for (int dx = 0; dx < PATCH; dx++) {
          const float tx = px + (float)(dx - RADIUS);
          const float hx = (h0 * tx + h1 * ty) + h2;
          const float hy = (h3 * tx + h4 * ty) + h5;
          const float hw = (h6 * tx + h7 * ty) + h8;
          const bool front = hw > 0.0f;
          const float r = 1.0f / (front ? hw : 1.0f);
          float u = hx * r, v = hy * r;
          const bool good = front && u >= 0.0f && u <= wm && v >= 0.0f && v <= hm;   // (NaN: not good)
          ok = ok && good;
          u = good ? u : 0.0f;
          v = good ? v : 0.0f;
          const float x0 = fminf(floorf(u), wc), y0 = fminf(floorf(v), hc);
          const float fx = u - x0, fy = v - y0;
          const uint8_t* q = other + (int)y0 * W + (int)x0;                          // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2
          const float top = (float)q[0] * (1.0f - fx) + (float)q[1] * fx;
          const float bot = (float)q[W] * (1.0f - fx) + (float)q[W + 1] * fx;
          const float b = (top * (1.0f - fy) + bot * fy) - ma;
          sb = sb + b;
          sbb = sbb + b * b;
          cov = cov + da[dy * PATCH + dx][lane] * b;
        }
      }
      const float vb = sbb - (sb * sb) / (float)NTAPS;
      const float den = va * vb;
      const float s = den > 1e-6f ? cov / sqrtf(den) : 0.0f;
      if (k0 >= 0 && k == k0 + 1) {
        right = s;
        rvalid = ok;
      }
      if (ok) {
        if (s > s0) {
          s3 = s2, k3 = k2, s2 = s1, k2 = k1, s1 = s0, k1 = k0, s0 = s, k0 = k;
          left = prev, lvalid = pvalid, rvalid = false;
        } else if (s > s1) {
          s3 = s2, k3 = k2, s2 = s1, k2 = k1, s1 = s, k1 = k;
        } else if (s > s2) {
          s3 = s2, k3 = k2, s2 = s, k2 = k;
        } else if (s > s3) {
          s3 = s, k3 = k;
        }
      }
      prev = s;
      pvalid = ok;
    }
  }
  if (!live) return;
  // best valid score outside k0 +- 1: the first of the three runners-up that is not a neighbour
  float second = -INFINITY;
  if (k1 >= 0 && abs(k1 - k0) > 1) second = s1;
  else if (k2 >= 0 && abs(k2 - k0) > 1) second = s2;
  else if (k3 >= 0 && abs(k3 - k0) > 1) second = s3;
  const bool has = k0 >= 0 && s0 >= g.min_score && !(second > s0 - g.margin);
  float off = 0.0f;
  const bool can = k0 > 0 && k0 < D - 1 && lvalid && rvalid;
  if (can) {
    const float denom = (left - 2.0f * s0) + right;
    if (denom < 0.0f) off = (0.5f * (left - right)) / denom;
  }
  const size_t o = (size_t)dir * a.n + node;
  g.node_invd[o] = has ? g.inv_far + g.step * ((float)k0 + off) : NONE;
  g.node_score[o] = k0 >= 0 ? s0 : 0.0f;
  g.node_k[o] = k0;
}

__global__ void __launch_bounds__(CTPB) check_kernel(Args a) {
  __shared__ int wave_n[CTPB / B3GS_WAVE];
  const B3gsSweepPair& g = a.io;
  const int dir = blockIdx.y;
  const int node = blockIdx.x * CTPB + threadIdx.x;
  bool keep = false;
  if (node < a.n) {
    const float invd_own = g.node_invd[(size_t)dir * a.n + node];
    if (invd_own != NONE) {
      const float* m = g.proj + 12 * dir;
      const float x = (float)(RADIUS + (node % a.nx) * g.stride), y = (float)(RADIUS + (node / a.nx) * g.stride);
      const float hx = ((m[0] * x + m[1] * y) + m[2]) + m[9] * invd_own;
      const float hy = ((m[3] * x + m[4] * y) + m[5]) + m[10] * invd_own;
      const float hw = ((m[6] * x + m[7] * y) + m[8]) + m[11] * invd_own;
      const bool front = hw > 0.0f;
      const float r = 1.0f / (front ? hw : 1.0f);
      const float qx = hx * r, qy = hy * r, inb = invd_own * r;
      const float i = rintf((qx - (float)RADIUS) / (float)g.stride), j = rintf((qy - (float)RADIUS) / (float)g.stride);
      if (front && i >= 0.0f && i <= (float)(a.nx - 1) && j >= 0.0f && j <= (float)(a.ny - 1)) {
        const float invd_there = g.node_invd[(size_t)(1 - dir) * a.n + (int)j * a.nx + (int)i];
        keep = invd_there != NONE && fabsf(invd_there - inb) <= g.cyc_steps * g.step;
      }
      a.rec[2 * ((size_t)dir * a.n + node)] = qx;
      a.rec[2 * ((size_t)dir * a.n + node) + 1] = qy;
    }
    a.keep[(size_t)dir * a.n + node] = keep ? 1 : 0;
  }
  int total;
  b3gs_block_rank<CTPB, 1>(keep, wave_n, &total);
  if (threadIdx.x == 0) a.block_count[(size_t)dir * (a.nb + 1) + blockIdx.x] = total;
}

// one block per direction: exclusive scan of the block counts in place, the total to count[dir]
__global__ void __launch_bounds__(B3GS_SCAN_TPB) scan_kernel(Args a) {
  b3gs_scan_block_sums(a.block_count + (size_t)blockIdx.x * (a.nb + 1), a.nb, a.io.count + blockIdx.x);
}

__global__ void __launch_bounds__(CTPB) compact_kernel(Args a) {
  __shared__ int wave_n[CTPB / B3GS_WAVE];
  const B3gsSweepPair& g = a.io;
  const int dir = blockIdx.y;
  const int node = blockIdx.x * CTPB + threadIdx.x;
  const bool keep = node < a.n && a.keep[(size_t)dir * a.n + node] != 0;
  int total;
  const int slot = a.block_count[(size_t)dir * (a.nb + 1) + blockIdx.x] + b3gs_block_rank<CTPB, 1>(keep, wave_n, &total);
  if (!keep) return;
  if (slot >= a.n) return;                                                          // (cannot happen: the outputs hold n rows)
  const size_t o = (size_t)dir * a.n + slot, in = (size_t)dir * a.n + node;
  g.kp_source[2 * o] = (float)(RADIUS + (node % a.nx) * g.stride);
  g.kp_source[2 * o + 1] = (float)(RADIUS + (node / a.nx) * g.stride);
  g.kp_target[2 * o] = a.rec[2 * in];
  g.kp_target[2 * o + 1] = a.rec[2 * in + 1];
  g.score[o] = g.node_score[in];
}

struct Layout {
  int nx, ny, n, nb;
  size_t gray, rec, keep, counts, total;
};

static bool layout(int64_t W, int64_t H, int64_t D, int64_t stride, Layout* l) {
  if (W < PATCH || H < PATCH || W * H > ((int64_t)1 << 26) || D < 2 || D > (1 << 16) || stride < 1) return false;
  l->nx = (int)((W - PATCH) / stride + 1);
  l->ny = (int)((H - PATCH) / stride + 1);
  l->n = l->nx * l->ny;
  l->nb = (l->n + CTPB - 1) / CTPB;
  size_t at = 0;
  l->gray = at, at += align256((size_t)2 * W * H);
  l->rec = at, at += align256((size_t)2 * l->n * 2 * sizeof(float));
  l->keep = at, at += align256((size_t)2 * l->n);
  l->counts = at, at += align256((size_t)2 * (l->nb + 1) * sizeof(int32_t));
  l->total = at;
  return true;
}

}  // namespace

extern "C" size_t b3gs_sweep_workspace_bytes(int32_t W, int32_t H, int32_t D, int32_t stride) {
  Layout l;
  return layout(W, H, D, stride, &l) ? l.total : 0;
}

extern "C" int b3gs_sweep_match_pair(const B3gsSweepPair* io, b3gs_stream_t stream) {
  static const char* what = "b3gs_sweep_match_pair";
  if (!io) return b3gs_fail(B3GS_ERR_ARG, what, "io is NULL");
  const B3gsSweepPair& g = *io;
  if (g.radius != RADIUS) return b3gs_fail(B3GS_ERR_ARG, what, "radius=3 (a 7x7 patch) is the only supported patch");
  if (g.W < PATCH || g.H < PATCH || (int64_t)g.W * g.H > ((int64_t)1 << 26))
    return b3gs_fail(B3GS_ERR_ARG, what, "the images are at least 7 x 7 and at most 2^26 pixels");
  if (g.D < 2 || g.D > (1 << 16)) return b3gs_fail(B3GS_ERR_ARG, what, "2 .. 65536 hypotheses (D)");
  if (g.stride < 1) return b3gs_fail(B3GS_ERR_ARG, what, "the node stride is at least 1");
  if (!(g.near > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "near is positive");
  if (!(g.near < g.far)) return b3gs_fail(B3GS_ERR_ARG, what, "near is smaller than far");
  if (!(g.step > 0.f) || !(g.inv_far > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "inv_far = 1 / far and step = (1 / near - 1 / far) / (D - 1) are positive");
  if (!(g.cyc_steps >= 0.f) || !(g.margin >= 0.f) || !(g.min_var >= 0.f))
    return b3gs_fail(B3GS_ERR_ARG, what, "cyc_steps, margin and min_var are not negative");
  if (!g.image_a || !g.image_b || !g.homographies || !g.proj || !g.kp_source || !g.kp_target || !g.score || !g.count || !g.node_invd ||
      !g.node_score || !g.node_k)
    return b3gs_fail(B3GS_ERR_ARG, what, "NULL pointer");
  if (!g.workspace || ((uintptr_t)g.workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  Layout l;
  if (!layout(g.W, g.H, g.D, g.stride, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "bad sizes");
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(g.workspace);
  Args a = {g, l.nx, l.ny, l.n, reinterpret_cast<uint8_t*>(ws + l.gray), reinterpret_cast<float*>(ws + l.rec),
            reinterpret_cast<uint8_t*>(ws + l.keep), reinterpret_cast<int32_t*>(ws + l.counts), l.nb};
  hipLaunchKernelGGL(gray_kernel, dim3((unsigned)((g.W * g.H + CTPB - 1) / CTPB), 2), dim3(CTPB), 0, s, a);
  hipLaunchKernelGGL(score_kernel, dim3((unsigned)((l.n + TPB - 1) / TPB), 2), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(check_kernel, dim3((unsigned)l.nb, 2), dim3(CTPB), 0, s, a);
  hipLaunchKernelGGL(scan_kernel, dim3(2), dim3(B3GS_SCAN_TPB), 0, s, a);
  hipLaunchKernelGGL(compact_kernel, dim3((unsigned)l.nb, 2), dim3(CTPB), 0, s, a);
  return b3gs_launch_status(what);
}
