// Baseline JPEG on the device (ABI 16): the entropy-coded scan of up to 8 uint8 [H,W,3] images of one W x H per call -- the
// images b3gs_encode_frames_batch writes -- without a host read.  YCbCr 4:2:0, one interleaved scan, the Annex K Huffman
// tables, no restart markers; header and EOI are the caller's (binocular3dgs_amd/frames.py).  All arithmetic is integer (the
// IJG "slow integer" definitions) and restated in tests/jpeg_ref.py, against which the output is compared byte for byte.
// Launches (all views in each):
//   1 transform  one wave per 16 x 16 MCU: edge-replicated load, colour conversion, 2 x 2 chroma average through LDS, the
//                8 x 8 forward DCT of the 6 blocks (rows, then columns), quantisation; int16 coefficients in zigzag order
//   2 size       one wave per MCU, lane k = zigzag coefficient k: the codes of the 6 blocks (a ballot of the non-zero lanes
//                gives every run length), their bit count
//   3 scan       one workgroup per view: exclusive scan of the MCU bit counts; zeroes the words the scan will occupy
//   4 emit       one wave per MCU: every code at its bit offset, MSB first (32-bit atomic OR into the zeroed words), and
//                the 1-bits that fill the last byte
//   5 stuffscan  one workgroup per view: 0xFF bytes per 64-byte chunk, exclusive scan, the frame's length (-1: no room)
//   6 stuff      one thread per chunk: the bytes with 0x00 behind every 0xFF, to the caller's buffer
#include "b3gs_internal.h"

namespace {

constexpr int JV = B3GS_MAX_FRAME_VIEWS;
constexpr int TPB = 256;                 // 4 waves = 4 MCUs per workgroup (transform, size, emit)
constexpr int SCAN_TPB = 1024;
constexpr int MCU_COEFS = 6 * 64;
// bits of one MCU at most: per coefficient a code of <= 16 bits and <= 11 magnitude bits (a ZRL costs less than one bit per
// zero it covers, an EOB stands for at least one zero)
constexpr int MCU_WORDS = MCU_COEFS * 27 / 32;   // 324
constexpr int CHUNK = 64;                // bytes per thread of the stuffing passes

struct HuffSpec {
  uint8_t bits[16];
  uint8_t vals[162];
  int n;
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUMA = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}, 162};
constexpr HuffSpec AC_CHROMA = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}, 162};

// code << 5 | length of every symbol (Annex C: codes of one length count up, a longer length starts at twice the next code);
// dc[table][size], ac[table][run << 4 | size]
constexpr int HUFF_DC = 0, HUFF_AC = 32, HUFF_WORDS = 32 + 512;
struct HuffTable {
  uint32_t e[HUFF_WORDS];
};
constexpr void huff_fill(HuffTable& t, int base, const HuffSpec& s) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; len++) {
    for (int i = 0; i < s.bits[len - 1]; i++, k++, code++) t.e[base + s.vals[k]] = code << 5 | (uint32_t)len;
    code <<= 1;
  }
}
constexpr HuffTable huff_build() {
  HuffTable t = {};
  huff_fill(t, HUFF_DC, DC_LUMA);
  huff_fill(t, HUFF_DC + 16, DC_CHROMA);
  huff_fill(t, HUFF_AC, AC_LUMA);
  huff_fill(t, HUFF_AC + 256, AC_CHROMA);
  return t;
}
__constant__ HuffTable g_huff = huff_build();

__constant__ uint8_t g_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegViews {
  const uint8_t* img[JV];
};

struct JpegWork {
  int16_t* coef;                   // [nv][nm][6][64] quantised, zigzag order
  uint32_t* mbits;                 // [nv][nm] bits of every MCU
  unsigned long long* moff;        // [nv][nm] bit offset of every MCU
  unsigned long long* tot;         // [nv][2]  bits of the scan (before the fill bits), bytes before stuffing
  uint32_t* words;                 // [nv][words_per_view] the scan before stuffing: stream bit i = bit 31 - i % 32 of word i / 32
  unsigned long long* ffoff;       // [nv][chunks_per_view] 0xFF bytes before every 64-byte chunk
  size_t words_per_view, chunks_per_view;
};

static size_t carve(int nv, int64_t nm, JpegWork* w, char* base) {
  char* cur = base;
  JpegWork t;
  t.words_per_view = (((size_t)nm * MCU_WORDS + 15) / 16 + 1) * 16;       // whole chunks
  t.chunks_per_view = t.words_per_view * 4 / CHUNK;
  t.coef = b3gs_carve<int16_t>(cur, (size_t)nv * nm * MCU_COEFS);
  t.mbits = b3gs_carve<uint32_t>(cur, (size_t)nv * nm);
  t.moff = b3gs_carve<unsigned long long>(cur, (size_t)nv * nm);
  t.tot = b3gs_carve<unsigned long long>(cur, (size_t)nv * 2);
  t.words = b3gs_carve<uint32_t>(cur, (size_t)nv * t.words_per_view);
  t.ffoff = b3gs_carve<unsigned long long>(cur, (size_t)nv * t.chunks_per_view);
  if (w) *w = t;
  return (size_t)(cur - base);
}

// ---- transform -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of the 13-bit Loeffler-Ligtenberg-Moschytz transform over 8 values `stride` apart.  FIRST: rows, results carry 2
// extra bits; else columns, which remove them again and leave the coefficients scaled by 8.
template <bool FIRST>
__device__ __forceinline__ void dct_pass(int* p, int stride) {
  const int d0 = p[0], d1 = p[stride], d2 = p[2 * stride], d3 = p[3 * stride], d4 = p[4 * stride], d5 = p[5 * stride],
            d6 = p[6 * stride], d7 = p[7 * stride];
  const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = FIRST ? 11 : 15;
  p[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  p[4 * stride] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  const int e = (t12 + t13) * 4433;
  p[2 * stride] = descale(e + t13 * 6270, N);
  p[6 * stride] = descale(e - t12 * 15137, N);
  const int z5 = (t4 + t6 + t5 + t7) * 9633;
  const int z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
  p[7 * stride] = descale(t4 * 2446 + z1 + z3, N);
  p[5 * stride] = descale(t5 * 16819 + z2 + z4, N);
  p[3 * stride] = descale(t6 * 25172 + z2 + z3, N);
  p[stride] = descale(t7 * 12299 + z1 + z4, N);
}

constexpr int BS = 9;                    // row stride of a block in LDS (8 + 1: the column pass reads down a column)
constexpr int CS = 17;                   // row stride of the full-resolution chroma planes

// grid (ceil(nm / 4), nv).  qt: the two tables, row-major, 64 entries each
__global__ void __launch_bounds__(TPB) jpeg_transform_kernel(JpegViews t, int W, int H, int mw, int nm,
                                                             const uint16_t* __restrict__ qt, int16_t* __restrict__ coef) {
  __shared__ int chroma[TPB / 64][2][16 * CS];
  __shared__ int blk[TPB / 64][6][8 * BS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, v = blockIdx.y;
  const int m_raw = blockIdx.x * (TPB / 64) + wave;
  const bool live = m_raw < nm;
  const int m = live ? m_raw : nm - 1;   // idle waves of the last workgroup repeat its last MCU (they reach every barrier)
  const int my = m / mw, mx = m - my * mw;
  {
    const int row = lane >> 2, c0 = (lane & 3) * 4;
    const int y = min(my * 16 + row, H - 1);
    const uint8_t* __restrict__ src = t.img[v] + (size_t)y * W * 3;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int col = c0 + i;
      const int x = min(mx * 16 + col, W - 1);
      const int r = src[3 * x], g = src[3 * x + 1], b = src[3 * x + 2];
      const int yy = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
      const int cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
      const int cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
      blk[wave][(row >> 3) * 2 + (col >> 3)][(row & 7) * BS + (col & 7)] = yy - 128;
      chroma[wave][0][row * CS + col] = cb;
      chroma[wave][1][row * CS + col] = cr;
    }
  }
  __syncthreads();
  {
    const int cy = lane >> 3, cx = lane & 7;
    const int bias = 1 + (cx & 1);       // 1, 2, 1, 2 along the row (an MCU starts at an even chroma column)
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const int* p = &chroma[wave][c][2 * cy * CS + 2 * cx];
      blk[wave][4 + c][cy * BS + cx] = ((p[0] + p[1] + p[CS] + p[CS + 1] + bias) >> 2) - 128;
    }
  }
  __syncthreads();
  if (lane < 48) dct_pass<true>(&blk[wave][lane >> 3][(lane & 7) * BS], 1);
  __syncthreads();
  if (lane < 48) dct_pass<false>(&blk[wave][lane >> 3][lane & 7], BS);
  __syncthreads();
  if (!live) return;
  const int nat = g_zigzag[lane];
  const int pos = (nat >> 3) * BS + (nat & 7);
  const int q8[2] = {8 * (int)qt[nat], 8 * (int)qt[64 + nat]};
  int16_t* __restrict__ out = coef + ((size_t)v * nm + m) * MCU_COEFS;
#pragma unroll
  for (int b = 0; b < 6; b++) {
    const int c = blk[wave][b][pos];
    const int q = q8[b >> 2];
    const int a = (abs(c) + (q >> 1)) / q;
    out[b * 64 + lane] = (int16_t)(c < 0 ? -a : a);
  }
}

// ---- entropy coding ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_huff(uint32_t* hs) {
  for (int i = threadIdx.x; i < HUFF_WORDS; i += blockDim.x) hs[i] = g_huff.e[i];
  __syncthreads();
}

__device__ __forceinline__ int size_of(int a) { return 32 - __clz(a); }   // 0 for 0

// The bits lane `lane` (= zigzag position) of a block contributes, MSB first in the low `len` bits of `val`: lane 0 the DC
// difference; a non-zero AC lane the ZRLs of its zero run, its (run, size) code and its magnitude bits; lane 63, when its
// coefficient is zero, the EOB.  At most 3 * 11 + 16 + 10 = 59 bits.  Every lane of the wave calls this.
__device__ __forceinline__ void lane_code(int c, int lane, int tab, int prev_dc, const uint32_t* hs, unsigned long long& val,
                                          int& len) {
  const unsigned long long nz = __ballot(c != 0) | 1ull;       // position 0 ends every run
  val = 0;
  len = 0;
  if (lane == 0) {
    const int d = c - prev_dc;
    const int nb = size_of(abs(d));
    const uint32_t e = hs[HUFF_DC + tab * 16 + nb];
    const uint32_t extra = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << nb) - 1u);
    val = ((unsigned long long)(e >> 5) << nb) | extra;
    len = (int)(e & 31u) + nb;
  } else if (c != 0) {
    const unsigned long long below = nz & ((1ull << lane) - 1ull);
    const int run = lane - (63 - __clzll((long long)below)) - 1;
    const int nb = size_of(abs(c));
    const uint32_t* ac = hs + HUFF_AC + tab * 256;
    const uint32_t z = ac[0xF0], e = ac[(run & 15) << 4 | nb];
    for (int i = 0; i < (run >> 4); i++) val = val << (z & 31u) | (z >> 5);
    len = (run >> 4) * (int)(z & 31u) + (int)(e & 31u) + nb;
    const uint32_t extra = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << nb) - 1u);
    val = ((val << (e & 31u) | (e >> 5)) << nb) | extra;
  } else if (lane == 63) {
    const uint32_t e = hs[HUFF_AC + tab * 256];
    val = e >> 5;
    len = (int)(e & 31u);
  }
}

// DC of the previous block of the same component (0 at the start of the scan); `mc` = this MCU's coefficients
__device__ __forceinline__ int prev_dc(const int16_t* mc, int m, int b) {
  if (b >= 1 && b <= 3) return mc[(b - 1) * 64];
  if (m == 0) return 0;
  return mc[-MCU_COEFS + (b == 0 ? 3 : b) * 64];
}

// grid (ceil(nm / 4), nv)
__global__ void __launch_bounds__(TPB) jpeg_size_kernel(int nm, JpegWork w) {
  __shared__ uint32_t hs[HUFF_WORDS];
  load_huff(hs);
  const int lane = threadIdx.x & 63, v = blockIdx.y;
  const int m = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (m >= nm) return;
  const int16_t* __restrict__ mc = w.coef + ((size_t)v * nm + m) * MCU_COEFS;
  int bits = 0;
#pragma unroll
  for (int b = 0; b < 6; b++) {
    unsigned long long val;
    int len;
    lane_code(mc[b * 64 + lane], lane, b >> 2, lane == 0 ? prev_dc(mc, m, b) : 0, hs, val, len);
    bits += len;
  }
  bits = b3gs_wave_sum(bits);
  if (lane == 0) w.mbits[(size_t)v * nm + m] = (uint32_t)bits;
}

// grid (nv): bit offsets of the MCUs; zeroes the words of the scan (whole 64-byte chunks)
__global__ void __launch_bounds__(SCAN_TPB) jpeg_scan_kernel(int nm, JpegWork w) {
  __shared__ unsigned long long wave_n[SCAN_TPB / B3GS_WAVE];
  const int v = blockIdx.x;
  const uint32_t* __restrict__ mb = w.mbits + (size_t)v * nm;
  unsigned long long* __restrict__ mo = w.moff + (size_t)v * nm;
  unsigned long long carry = 0;
  for (int base = 0; base < nm; base += SCAN_TPB) {
    const int i = base + (int)threadIdx.x;
    unsigned long long tile;
    const unsigned long long ex = b3gs_block_exscan<SCAN_TPB>((unsigned long long)(i < nm ? mb[i] : 0u), wave_n, &tile);
    if (i < nm) mo[i] = carry + ex;
    carry += tile;
  }
  const unsigned long long nbytes = (carry + 7) >> 3;
  if (threadIdx.x == 0) {
    w.tot[2 * v] = carry;
    w.tot[2 * v + 1] = nbytes;
  }
  size_t nw = (size_t)((nbytes + CHUNK - 1) / CHUNK) * (CHUNK / 4);
  nw = nw < w.words_per_view ? nw : w.words_per_view;
  uint4* __restrict__ z = reinterpret_cast<uint4*>(w.words + (size_t)v * w.words_per_view);
  for (size_t i = threadIdx.x; i < nw / 4; i += SCAN_TPB) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ORs the low `len` (1..64) bits of val into the stream at bit `pos`
__device__ __forceinline__ void put_bits(uint32_t* words, size_t nwords, unsigned long long pos, unsigned long long val, int len) {
  const size_t wi = (size_t)(pos >> 5);
  const int sh = (int)(pos & 31u);
  const unsigned long long x = val << (64 - len);                 // left-aligned
  const unsigned long long hi = x >> sh, lo = sh ? x << (64 - sh) : 0ull;
  const uint32_t w0 = (uint32_t)(hi >> 32), w1 = (uint32_t)hi, w2 = (uint32_t)(lo >> 32);
  if (w0 && wi < nwords) atomicOr(&words[wi], w0);
  if (w1 && wi + 1 < nwords) atomicOr(&words[wi + 1], w1);
  if (w2 && wi + 2 < nwords) atomicOr(&words[wi + 2], w2);
}

// grid (ceil(nm / 4), nv)
__global__ void __launch_bounds__(TPB) jpeg_emit_kernel(int nm, JpegWork w) {
  __shared__ uint32_t hs[HUFF_WORDS];
  load_huff(hs);
  const int lane = threadIdx.x & 63, v = blockIdx.y;
  const int m = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
  if (m >= nm) return;
  const int16_t* __restrict__ mc = w.coef + ((size_t)v * nm + m) * MCU_COEFS;
  uint32_t* __restrict__ words = w.words + (size_t)v * w.words_per_view;
  unsigned long long off = w.moff[(size_t)v * nm + m];
#pragma unroll
  for (int b = 0; b < 6; b++) {
    unsigned long long val;
    int len;
    lane_code(mc[b * 64 + lane], lane, b >> 2, lane == 0 ? prev_dc(mc, m, b) : 0, hs, val, len);
    const int inc = b3gs_wave_scan(len, lane);
    if (len) put_bits(words, w.words_per_view, off + (unsigned long long)(inc - len), val, len);
    off += (unsigned long long)__shfl(inc, 63, 64);
  }
  if (m == nm - 1 && lane == 0) {        // the last byte is filled with 1-bits
    const int pad = (int)((8u - (uint32_t)(off & 7u)) & 7u);
    if (pad) put_bits(words, w.words_per_view, off, (1ull << pad) - 1ull, pad);
  }
}

// ---- byte stuffing -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t stream_byte(uint32_t word, int k) { return (word >> (24 - 8 * k)) & 0xFFu; }

// grid (nv): 0xFF bytes before every chunk; lengths[v] = bytes of the stuffed scan, or -1 when they exceed the capacity
__global__ void __launch_bounds__(SCAN_TPB) jpeg_stuffscan_kernel(JpegWork w, long long capacity, long long* __restrict__ lengths) {
  __shared__ unsigned long long wave_n[SCAN_TPB / B3GS_WAVE];
  const int v = blockIdx.x;
  const unsigned long long nbytes = w.tot[2 * v + 1];
  const size_t nchunks = (size_t)((nbytes + CHUNK - 1) / CHUNK);
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(w.words + (size_t)v * w.words_per_view);
  unsigned long long* __restrict__ fo = w.ffoff + (size_t)v * w.chunks_per_view;
  unsigned long long carry = 0;
  for (size_t base = 0; base < nchunks; base += SCAN_TPB) {
    const size_t c = base + threadIdx.x;
    uint32_t n = 0;
    if (c < nchunks) {
      const unsigned long long left = nbytes - (unsigned long long)c * CHUNK;     // bytes of this chunk that belong to the scan
      const int valid = left < (unsigned long long)CHUNK ? (int)left : CHUNK;
#pragma unroll
      for (int q = 0; q < CHUNK / 16; q++) {
        const uint4 x = src[c * (CHUNK / 16) + q];
        const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
          for (int k = 0; k < 4; k++) n += (q * 16 + j * 4 + k < valid && stream_byte(xs[j], k) == 0xFFu) ? 1u : 0u;
      }
    }
    unsigned long long tile;
    const unsigned long long ex = b3gs_block_exscan<SCAN_TPB>((unsigned long long)n, wave_n, &tile);
    if (c < nchunks) fo[c] = carry + ex;
    carry += tile;
  }
  if (threadIdx.x == 0) {
    const unsigned long long total = nbytes + carry;
    lengths[v] = total <= (unsigned long long)capacity ? (long long)total : -1ll;
  }
}

// grid (ceil(chunks_per_view / TPB), nv): a frame that does not fit is not written at all
__global__ void __launch_bounds__(TPB) jpeg_stuff_kernel(JpegWork w, long long capacity, const long long* __restrict__ lengths,
                                                         uint8_t* __restrict__ out) {
  const int v = blockIdx.y;
  const long long total = lengths[v];
  if (total < 0) return;
  const unsigned long long nbytes = w.tot[2 * v + 1];
  const size_t c = (size_t)blockIdx.x * TPB + threadIdx.x;
  if ((unsigned long long)c * CHUNK >= nbytes) return;
  const unsigned long long left = nbytes - (unsigned long long)c * CHUNK;
  const int valid = left < (unsigned long long)CHUNK ? (int)left : CHUNK;
  const uint4* __restrict__ src = reinterpret_cast<const uint4*>(w.words + (size_t)v * w.words_per_view) + c * (CHUNK / 16);
  unsigned long long o = (unsigned long long)c * CHUNK + w.ffoff[(size_t)v * w.chunks_per_view + c];
  uint8_t* __restrict__ dst = out + (size_t)v * (size_t)capacity;
  for (int q = 0; q < CHUNK / 16; q++) {
    const uint4 x = src[q];
    const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (q * 16 + j * 4 + k >= valid) continue;
        const uint32_t byte = stream_byte(xs[j], k);
        if (o < (unsigned long long)total) dst[o] = (uint8_t)byte;
        o++;
        if (byte == 0xFFu) {
          if (o < (unsigned long long)total) dst[o] = 0;
          o++;
        }
      }
  }
}

static bool sides_ok(int32_t nviews, int32_t H, int32_t W) {
  return nviews >= 1 && nviews <= JV && H >= 1 && H <= 65535 && W >= 1 && W <= 65535;
}

}  // namespace

extern "C" size_t b3gs_jpeg_workspace_bytes(int32_t nviews, int32_t H, int32_t W) {
  if (!sides_ok(nviews, H, W)) return 0;
  return carve(nviews, (int64_t)((W + 15) / 16) * ((H + 15) / 16), nullptr, nullptr);
}

extern "C" int b3gs_jpeg_encode_batch(int32_t nviews, const uint8_t* const* images, int32_t H, int32_t W, const uint16_t* qtables,
                                      uint8_t* out, int64_t capacity, int64_t* lengths, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_jpeg_encode_batch";
  if (!sides_ok(nviews, H, W)) return b3gs_fail(B3GS_ERR_ARG, what, "1..8 views of 1..65535 pixels per side are needed");
  if (!images || !qtables || !out || !lengths || !workspace) return b3gs_fail(B3GS_ERR_ARG, what, "null pointer");
  if (capacity < 1) return b3gs_fail(B3GS_ERR_ARG, what, "capacity must be at least 1 byte per frame");
  if ((uintptr_t)workspace & 255) return b3gs_fail(B3GS_ERR_ARG, what, "workspace must be 256-byte aligned");
  JpegViews t = {};
  for (int i = 0; i < nviews; i++) {
    if (!images[i]) return b3gs_fail(B3GS_ERR_ARG, what, "null image");
    t.img[i] = images[i];
  }
  const int mw = (W + 15) / 16, mh = (H + 15) / 16;
  const int64_t nm64 = (int64_t)mw * mh;
  if (nm64 > (int64_t)0x7fffffff - SCAN_TPB) return b3gs_fail(B3GS_ERR_ARG, what, "too many MCUs");
  const int nm = (int)nm64;
  JpegWork w;
  carve(nviews, nm, &w, static_cast<char*>(workspace));
  hipStream_t s = (hipStream_t)stream;
  const dim3 per_mcu((unsigned)((nm + TPB / 64 - 1) / (TPB / 64)), (unsigned)nviews);
  hipLaunchKernelGGL(jpeg_transform_kernel, per_mcu, dim3(TPB), 0, s, t, (int)W, (int)H, mw, nm, qtables, w.coef);
  hipLaunchKernelGGL(jpeg_size_kernel, per_mcu, dim3(TPB), 0, s, nm, w);
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)nviews), dim3(SCAN_TPB), 0, s, nm, w);
  hipLaunchKernelGGL(jpeg_emit_kernel, per_mcu, dim3(TPB), 0, s, nm, w);
  hipLaunchKernelGGL(jpeg_stuffscan_kernel, dim3((unsigned)nviews), dim3(SCAN_TPB), 0, s, w, (long long)capacity,
                     reinterpret_cast<long long*>(lengths));
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)((w.chunks_per_view + TPB - 1) / TPB), (unsigned)nviews), dim3(TPB), 0, s, w,
                     (long long)capacity, reinterpret_cast<const long long*>(lengths), out);
  return b3gs_launch_status(what);
}
