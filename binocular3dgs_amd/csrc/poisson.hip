// Screened Poisson surface reconstruction (added to ABI 18; binocular3dgs_amd/poisson.py): oriented
// samples from depth maps, their splat onto the node grid of a B3gsTsdfVolume, the right-hand side, conjugate gradients on the
// screened Laplacian, and the level / support planes the marching-tetrahedra extractor of mesh.hip reads.
// include/b3gs_raster.h states the arithmetic statement by statement; tests/poisson_ref.py restates it.  Every float statement is
// ONE correctly rounded operation (+ - * / sqrt; the Makefile compiles with -ffp-contract=off), a node owns its words, sums across
// threads are fixed-order fp64 folds: no floating-point atomic, no vendor library, one result whatever the launch geometry.
//   points    count   thread = pixel in (view, py, px) order: keep flag -> block sums; scan -> the total, one device word
//             emit    the same flag again, rank = block offset + ballot rank -> the sample's row
//   splat     keys    thread = sample: grid coordinate, base cell key (NO_KEY when its 8 nodes are not all inside: counted)
//             sort    the project's stable radix sort: members of a cell stay in sample order
//             ranges  thread = sorted position: first / last position of every cell
//             gather  thread = node: its 8 cells in (dz, dy, dx) order, members in order, fp64 sums, rounded once
//   solve     rhs     thread = node: b = -div V; x = 0, r = p = b; partial of b.b          fold: r.r = b.b, the stop test
//             per iteration TWO launches, thread = node, 256 consecutive nodes per partial (a wave = 64 consecutive nodes: with
//             nx a multiple of 64 one row segment, so the +-y / +-z reads are whole coalesced rows; the +-x values come from
//             the neighbouring lanes):
//               stencil  p = r + beta p (from the second iteration on; written once, read at the 7 points), Ap, partial of p.Ap
//               update   x += alpha p, r -= alpha Ap, partial of r.r
//             the LAST workgroup to finish a launch (an arrival counter: release / acquire at agent scope, no workgroup waits
//             for another) folds the partials in linear order and writes the step scalars for the next launch.
//   volume    iso     partials of D x and D, fold -> iso;   tsdf = x - iso;   three box passes of D -> weight;   rgb = 0
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int NV = B3GS_MAX_TSDF_VIEWS;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
constexpr int DEFAULT_BLOCKS = 2048;           // workgroups of a solver launch when the caller names none: 8 per CU

static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

// ---- oriented samples --------------------------------------------------------------------------------------------------
struct PointArgs {
  int32_t n, W, H, stride, median;
  float alpha_min, rel_jump, min_cos;
  int64_t npix;                     // n * W * H
  int64_t* total;
  uint32_t* bsum;
  int64_t npoints;                  // emit: rows of the outputs
  float *points, *normals, *weights, *colours;
  B3gsTsdfView v[NV];
};

struct Sample {
  float p[3], n[3], w, c[3];
};

__device__ __forceinline__ bool oriented_sample(const PointArgs& a, int64_t g, Sample* out) {
  const int64_t plane = (int64_t)a.W * a.H;
  const int v = (int)(g / plane);
  const int64_t pix = g - (int64_t)v * plane;
  const int py = (int)(pix / a.W), px = (int)(pix - (int64_t)py * a.W);
  if (px % a.stride || py % a.stride) return false;
  if (px < 1 || py < 1 || px > a.W - 2 || py > a.H - 2) return false;
  const B3gsTsdfView& c = a.v[v];
  const int64_t q[5] = {pix, pix - 1, pix + 1, pix - a.W, pix + a.W};
  float z[5];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const float al = c.alpha[q[k]];
    if (!(al >= a.alpha_min)) return false;
    z[k] = a.median ? c.depth[q[k]] : c.depth[q[k]] / al;
  }
  const float lim = a.rel_jump * z[0];
#pragma unroll
  for (int k = 1; k < 5; k++) {
    const float d = z[k] - z[0];
    if (!(fabsf(d) <= lim)) return false;
  }
  const float cx = 0.5f * (float)a.W - 0.5f, cy = 0.5f * (float)a.H - 0.5f;
  const int ox[5] = {0, -1, 1, 0, 0}, oy[5] = {0, 0, 0, -1, 1};
  float P[5][3];
#pragma unroll
  for (int k = 0; k < 5; k++) {
    const float u = ((float)(px + ox[k]) - cx) / c.fx, w = ((float)(py + oy[k]) - cy) / c.fy;
    P[k][0] = u * z[k];
    P[k][1] = w * z[k];
    P[k][2] = z[k];
  }
  float e[3], f[3];
#pragma unroll
  for (int x = 0; x < 3; x++) {
    e[x] = P[2][x] - P[1][x];
    f[x] = P[4][x] - P[3][x];
  }
  const float n0 = f[1] * e[2] - f[2] * e[1], n1 = f[2] * e[0] - f[0] * e[2], n2 = f[0] * e[1] - f[1] * e[0];   // f x e
  const float nn = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
  if (!(nn > 0.0f)) return false;
  const float pn = sqrtf((P[0][0] * P[0][0] + P[0][1] * P[0][1]) + P[0][2] * P[0][2]);
  const float d0 = (n0 * P[0][0] + n1 * P[0][1]) + n2 * P[0][2];
  const float cs = (0.0f - d0) / (nn * pn);
  if (!(cs > a.min_cos)) return false;
  const float u[3] = {n0 / nn, n1 / nn, n2 / nn};
  const float t[3] = {P[0][0] - c.trans[0], P[0][1] - c.trans[1], P[0][2] - c.trans[2]};
#pragma unroll
  for (int x = 0; x < 3; x++) {                                       // R^T: column x of the row-major rotation
    out->p[x] = (c.rot[x] * t[0] + c.rot[3 + x] * t[1]) + c.rot[6 + x] * t[2];
    out->n[x] = (c.rot[x] * u[0] + c.rot[3 + x] * u[1]) + c.rot[6 + x] * u[2];
    out->c[x] = c.colour[(int64_t)x * plane + pix];
  }
  out->w = cs;
  return true;
}

__global__ void __launch_bounds__(TPB) points_count_kernel(PointArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
  Sample s;
  const int keep = g < a.npix && oriented_sample(a, g, &s);
  int total;
  b3gs_block_rank<TPB, 1>(keep, wave_n, &total);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(SCAN_TPB) points_scan_kernel(uint32_t* bsum, int nb, int64_t* total) { b3gs_scan_block_sums(bsum, nb, total); }

__global__ void __launch_bounds__(TPB) points_emit_kernel(PointArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
  Sample s;
  const int keep = g < a.npix && oriented_sample(a, g, &s);
  int total;
  const int64_t row = (int64_t)a.bsum[blockIdx.x] + b3gs_block_rank<TPB, 1>(keep, wave_n, &total);
  if (!keep || row >= a.npoints) return;                              // (the outputs hold npoints rows)
#pragma unroll
  for (int x = 0; x < 3; x++) {
    a.points[3 * row + x] = s.p[x];
    a.normals[3 * row + x] = s.n[x];
    a.colours[3 * row + x] = s.c[x];
  }
  a.weights[row] = s.w;
}

static bool points_layout(int32_t nviews, int32_t W, int32_t H, int64_t* npix, size_t* total) {
  if (nviews < 1 || nviews > NV || W < 1 || H < 1 || (int64_t)W * H > ((int64_t)1 << 27)) return false;
  *npix = (int64_t)nviews * W * H;
  *total = 256 + b3gs_align256((size_t)blocks_of(*npix) * sizeof(uint32_t));
  return true;
}

static int points_args(const char* what, int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H, int32_t stride, float alpha_min,
                       float rel_jump, float min_cos, int32_t median, void* workspace, PointArgs* a) {
  if (nviews < 1 || nviews > NV) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views per call");
  if (!views) return b3gs_fail(B3GS_ERR_ARG, what, "views is NULL");
  size_t bytes;
  int64_t npix;
  if (!points_layout(nviews, W, H, &npix, &bytes)) return b3gs_fail(B3GS_ERR_ARG, what, "the images hold 1 .. 2^27 pixels");
  if (stride < 1) return b3gs_fail(B3GS_ERR_ARG, what, "the stride is at least 1");
  if (!(alpha_min > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "alpha_min is positive");
  if (!(rel_jump >= 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "rel_jump is not negative");
  if (min_cos != min_cos) return b3gs_fail(B3GS_ERR_ARG, what, "min_cos is NaN");
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  *a = PointArgs{};
  a->n = nviews, a->W = W, a->H = H, a->stride = stride, a->median = median != 0;
  a->alpha_min = alpha_min, a->rel_jump = rel_jump, a->min_cos = min_cos;
  a->npix = npix;
  a->total = reinterpret_cast<int64_t*>(workspace);
  a->bsum = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + 256);
  for (int v = 0; v < nviews; v++) {
    if (!views[v].depth || !views[v].alpha || !views[v].colour) return b3gs_fail(B3GS_ERR_ARG, what, "NULL image pointer");
    a->v[v] = views[v];
  }
  return B3GS_OK;
}

// ---- the grid ----------------------------------------------------------------------------------------------------------
struct Grid {
  int32_t nx, ny, nz;
  uint32_t n, nxy;                  // nodes (<= 2^30), nodes of one z plane
  uint32_t nb;                      // partials: 256 consecutive nodes each
  float o[3], voxel;
};

// the scalars of a solve, at the head of the workspace (one 256-byte block)
struct Head {
  int64_t dropped;                  // samples whose 8 nodes are not all inside the grid
  int64_t nsamples;                 // of the latest splat
  int64_t status;                   // bit 0: no surviving sample
  int64_t iterations;               // CG iterations done
  int64_t done;                     // the stop flag
  double rr, bb, pap, thr;          // r.r, b.b, p.Ap, tol^2 b.b
  double alpha, beta, num, den;     // the step scalars; sum(D x), sum(D)
  float af, bf, iso, pad;           // alpha, beta and iso rounded to float32
  uint32_t ticket;                  // arrivals of the running launch (zero between launches)
};
static_assert(sizeof(Head) <= 256, "one 256-byte head");

struct Ws {
  Head* head;
  uint32_t* skey[2];
  uint32_t* sval[2];
  uint32_t* hist;
  uint32_t* vkey;                   // [ns]
  float* frac;                      // [ns, 3] the sample's position inside its cell
  uint32_t *cstart, *cend;          // [n] sorted positions of every cell's members
  float *r, *p[2], *ap;             // [n]
  double* part;                     // [nb] (volume: [2][nb])
};

static size_t ws_carve(char* base, int64_t n, int64_t ns, Ws* w) {
  char* cur = base;
  const size_t nn = (size_t)(n > 0 ? n : 1), s = (size_t)(ns > 0 ? ns : 1);
  Ws t;
  // the node arrays come first: solve and volume find them without the sample count
  t.head = b3gs_carve<Head>(cur, 1);
  t.cstart = b3gs_carve<uint32_t>(cur, nn);
  t.cend = b3gs_carve<uint32_t>(cur, nn);
  t.r = b3gs_carve<float>(cur, nn);
  for (int k = 0; k < 2; k++) t.p[k] = b3gs_carve<float>(cur, nn);
  t.ap = b3gs_carve<float>(cur, nn);
  t.part = b3gs_carve<double>(cur, 2 * (size_t)blocks_of((int64_t)nn));
  for (int k = 0; k < 2; k++) t.skey[k] = b3gs_carve<uint32_t>(cur, s);
  for (int k = 0; k < 2; k++) t.sval[k] = b3gs_carve<uint32_t>(cur, s);
  t.hist = b3gs_carve<uint32_t>(cur, b3gs_sort_scratch_words((int64_t)s));
  t.vkey = b3gs_carve<uint32_t>(cur, s);
  t.frac = b3gs_carve<float>(cur, 3 * s);
  if (w) *w = t;
  return (size_t)(cur - base);
}

static bool grid_sizes(int64_t nx, int64_t ny, int64_t nz, int64_t ns) {
  return nx >= 1 && ny >= 1 && nz >= 1 && nx <= B3GS_MAX_TSDF_DIM && ny <= B3GS_MAX_TSDF_DIM && nz <= B3GS_MAX_TSDF_DIM && ns >= 0 &&
         ns < ((int64_t)1 << 31);
}

static int grid_of(const B3gsTsdfVolume* g, const char* what, Grid* out) {
  if (!g) return b3gs_fail(B3GS_ERR_ARG, what, "the grid is NULL");
  if (!grid_sizes(g->nx, g->ny, g->nz, 0)) return b3gs_fail(B3GS_ERR_ARG, what, "every dimension of the grid is 1 .. 1024");
  if (!(g->voxel > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the voxel size is positive");
  out->nx = g->nx, out->ny = g->ny, out->nz = g->nz;
  out->nxy = (uint32_t)g->nx * (uint32_t)g->ny;
  out->n = out->nxy * (uint32_t)g->nz;
  out->nb = blocks_of((int64_t)out->n);
  for (int k = 0; k < 3; k++) out->o[k] = g->origin[k];
  out->voxel = g->voxel;
  return B3GS_OK;
}

static int check_ws(const void* workspace, const char* what) {
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  return B3GS_OK;
}

// ---- splat -------------------------------------------------------------------------------------------------------------
__global__ void head_samples_kernel(Head* h, int64_t ns) { h->nsamples = ns; }

__global__ void __launch_bounds__(TPB) splat_key_kernel(Grid g, int64_t ns, const float* __restrict__ pos, uint32_t* __restrict__ vkey,
                                                        float* __restrict__ frac, Head* head) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool drop = false;
  if (i < ns) {
    const int dim[3] = {g.nx, g.ny, g.nz};
    uint32_t cell[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float s = (pos[3 * i + k] - g.o[k]) / g.voxel;
      const float c = s - 0.5f;                                       // nodes sit at the voxel centres
      const float b = floorf(c);
      const bool ok = b >= 0.0f && b <= (float)(dim[k] - 2);          // (false for NaN)
      drop = drop || !ok;
      cell[k] = ok ? (uint32_t)b : 0u;
      frac[3 * i + k] = c - b;
    }
    vkey[i] = drop ? NO_KEY : (cell[2] * (uint32_t)g.ny + cell[1]) * (uint32_t)g.nx + cell[0];
  }
  const unsigned long long m = __ballot(drop);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0 && m) atomicAdd(reinterpret_cast<unsigned long long*>(&head->dropped), (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(TPB) splat_range_kernel(int64_t ns, const uint32_t* __restrict__ skey, uint32_t* __restrict__ cstart,
                                                          uint32_t* __restrict__ cend) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= ns) return;
  const uint32_t k = skey[i];
  if (k == NO_KEY) return;
  if (i == 0 || skey[i - 1] != k) cstart[k] = (uint32_t)i;
  if (i == ns - 1 || skey[i + 1] != k) cend[k] = (uint32_t)(i + 1);
}

__global__ void __launch_bounds__(TPB) splat_gather_kernel(Grid g, const uint32_t* __restrict__ sval, const uint32_t* __restrict__ cstart,
                                                           const uint32_t* __restrict__ cend, const float* __restrict__ frac,
                                                           const float* __restrict__ nrm, const float* __restrict__ wgt,
                                                           float* __restrict__ density, float* __restrict__ vec) {
  const uint32_t idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= g.n) return;
  const int i = (int)(idx % (uint32_t)g.nx), j = (int)(idx / (uint32_t)g.nx % (uint32_t)g.ny), k = (int)(idx / g.nxy);
  double D = 0.0, V0 = 0.0, V1 = 0.0, V2 = 0.0;
  for (int c = 0; c < 8; c++) {                                       // (dz, dy, dx), dx fastest
    const int dx = c & 1, dy = c >> 1 & 1, dz = c >> 2;
    const int bx = i - dx, by = j - dy, bz = k - dz;                  // the cell whose corner (dx, dy, dz) this node is
    if (bx < 0 || by < 0 || bz < 0 || bx > g.nx - 2 || by > g.ny - 2 || bz > g.nz - 2) continue;
    const uint32_t cell = ((uint32_t)bz * (uint32_t)g.ny + (uint32_t)by) * (uint32_t)g.nx + (uint32_t)bx;
    const uint32_t end = cend[cell];
    for (uint32_t q = cstart[cell]; q < end; q++) {
      const uint32_t s = sval[q];
      const float fx = frac[3 * (size_t)s], fy = frac[3 * (size_t)s + 1], fz = frac[3 * (size_t)s + 2];
      const float tx = dx ? fx : 1.0f - fx, ty = dy ? fy : 1.0f - fy, tz = dz ? fz : 1.0f - fz;
      const float t = (tx * ty) * tz;
      const double wt = (double)wgt[s] * (double)t;
      D = D + wt;
      V0 = V0 + wt * (double)nrm[3 * (size_t)s];
      V1 = V1 + wt * (double)nrm[3 * (size_t)s + 1];
      V2 = V2 + wt * (double)nrm[3 * (size_t)s + 2];
    }
  }
  density[idx] = (float)D;
  vec[idx] = (float)V0;
  vec[(size_t)g.n + idx] = (float)V1;
  vec[2 * (size_t)g.n + idx] = (float)V2;
}

// ---- fixed-order sums --------------------------------------------------------------------------------------------------
// The partial of 256 consecutive nodes: the butterfly of every wave, then (wave 0 + wave 1) + (wave 2 + wave 3); thread 0 stores
// it write-through.  red: 4 doubles of LDS; the caller puts a barrier between two calls.
__device__ __forceinline__ void store_partial(double q, double* red, double* slot) {
  const double s = b3gs_wave_sum(q);
  if ((threadIdx.x & (B3GS_WAVE - 1)) == 0) red[threadIdx.x / B3GS_WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double v = (red[0] + red[1]) + (red[2] + red[3]);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}
// Every thread of every workgroup of the launch calls this once, after its partials: true in every thread of the workgroup that
// arrives last (all partials of the launch are then visible to it).  No workgroup waits for another.
__device__ __forceinline__ bool last_arrival(uint32_t* ticket, uint32_t* flag) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);   // releases thread 0's partials
    *flag = t == gridDim.x - 1u;
  }
  __syncthreads();
  return *flag != 0u;
}
// ONE wave: lane l adds the partials l, l + 64, .. in order from +0, then the butterfly (b3gs_wave_fold_f64, on words that
// other workgroups of this launch wrote: loaded past the L1)
__device__ __forceinline__ double fold_partials(const double* part, uint32_t n) {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  constexpr int BATCH = 16;                                           // loads in flight per lane: the adds stay in order
  double s = 0.0;
  for (uint32_t b0 = threadIdx.x; b0 < n; b0 += BATCH * B3GS_WAVE) {
    double v[BATCH];
#pragma unroll
    for (int k = 0; k < BATCH; k++) {
      const uint32_t b = b0 + (uint32_t)k * B3GS_WAVE;
      v[k] = b < n ? __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(part + b), __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT))
                   : 0.0;
    }
#pragma unroll
    for (int k = 0; k < BATCH; k++)
      if (b0 + (uint32_t)k * B3GS_WAVE < n) s += v[k];
  }
  return b3gs_wave_sum(s);
}

// ---- right-hand side and operator ----------------------------------------------------------------------------------------
struct CgArgs {
  Grid g;
  Head* head;
  const float* density;
  float screen;
  const float* pin;                 // stencil: the direction as stored (mode 2: the previous one)
  float* pout;                      // mode 2: the new direction
  float* out;                       // A p
  float *x, *r;
  const float* vec;                 // rhs
  float* rhs;
  double* part;
};

__global__ void __launch_bounds__(TPB) rhs_kernel(CgArgs a) {
  __shared__ double red[TPB / B3GS_WAVE];
  const Grid& g = a.g;
  const uint32_t idx = blockIdx.x * TPB + threadIdx.x;
  double q = 0.0;
  if (idx < g.n) {
    const int i = (int)(idx % (uint32_t)g.nx), j = (int)(idx / (uint32_t)g.nx % (uint32_t)g.ny), k = (int)(idx / g.nxy);
    const float* vx = a.vec;
    const float* vy = a.vec + g.n;
    const float* vz = a.vec + 2 * (size_t)g.n;
    const float xp = i < g.nx - 1 ? vx[idx + 1] : 0.0f, xm = i > 0 ? vx[idx - 1] : 0.0f;
    const float yp = j < g.ny - 1 ? vy[idx + g.nx] : 0.0f, ym = j > 0 ? vy[idx - g.nx] : 0.0f;
    const float zp = k < g.nz - 1 ? vz[idx + g.nxy] : 0.0f, zm = k > 0 ? vz[idx - g.nxy] : 0.0f;
    const float div = ((xp - xm) + (yp - ym)) + (zp - zm);
    const float b = 0.0f - 0.5f * div;
    a.rhs[idx] = b;
    a.x[idx] = 0.0f;
    a.r[idx] = b;
    a.pout[idx] = b;
    q = (double)b * (double)b;
  }
  store_partial(q, red, a.part + blockIdx.x);
}

// one wave after the right-hand side: r.r = b.b, the threshold, the stop test of iteration 0
__global__ void __launch_bounds__(B3GS_WAVE) start_kernel(Head* h, const double* part, uint32_t nb, double tol2) {
  const double bb = fold_partials(part, nb);
  if (threadIdx.x) return;
  const bool empty = h->nsamples - h->dropped <= 0;
  h->status = empty ? 1 : 0;
  h->rr = bb, h->bb = bb, h->pap = 0.0, h->alpha = 0.0, h->beta = 0.0;
  h->thr = tol2 * bb;
  h->af = 0.0f, h->bf = 0.0f;
  h->iterations = 0;
  h->done = (empty || bb <= h->thr) ? 1 : 0;
  h->ticket = 0u;
}

// MODE 0: out = A pin (no sum, no stop flag).  MODE 1: the first iteration, p = pin as stored.  MODE 2: p = r + beta pin first,
// stored to pout.  A workgroup walks the chunks blockIdx.x, blockIdx.x + gridDim.x, ..: a chunk's partial does not depend on which
// workgroup made it.
template <int MODE>
__global__ void __launch_bounds__(TPB) stencil_kernel(CgArgs a) {
  __shared__ double red[TPB / B3GS_WAVE];
  __shared__ uint32_t last;
  const Grid& g = a.g;
  Head* h = a.head;
  if (MODE != 0 && h->done) return;
  const float bf = MODE == 2 ? h->bf : 0.0f;
  const int lane = threadIdx.x & (B3GS_WAVE - 1);
  auto value = [&](uint32_t q) -> float {
    if (MODE != 2) return a.pin[q];
    const float t = bf * a.pin[q];
    return a.r[q] + t;
  };
  for (uint32_t chunk = blockIdx.x; chunk < g.nb; chunk += gridDim.x) {
    const uint32_t idx = chunk * TPB + threadIdx.x;
    const bool valid = idx < g.n;
    const float pc = valid ? value(idx) : 0.0f;
    float xm = __shfl_up(pc, 1, B3GS_WAVE), xp = __shfl_down(pc, 1, B3GS_WAVE);
    double q = 0.0;
    if (valid) {
      const int i = (int)(idx % (uint32_t)g.nx), j = (int)(idx / (uint32_t)g.nx % (uint32_t)g.ny), k = (int)(idx / g.nxy);
      if (i == 0) xm = pc;                                            // beyond the grid: the node itself
      else if (lane == 0) xm = value(idx - 1);
      if (i == g.nx - 1) xp = pc;
      else if (lane == B3GS_WAVE - 1) xp = value(idx + 1);
      const float ym = j == 0 ? pc : value(idx - g.nx), yp = j == g.ny - 1 ? pc : value(idx + g.nx);
      const float zm = k == 0 ? pc : value(idx - g.nxy), zp = k == g.nz - 1 ? pc : value(idx + g.nxy);
      const float s = (((pc - xm) + (pc - xp)) + ((pc - ym) + (pc - yp))) + ((pc - zm) + (pc - zp));
      const float sd = a.screen * a.density[idx];
      const float ap = s + sd * pc;
      a.out[idx] = ap;
      if (MODE == 2) a.pout[idx] = pc;
      q = (double)pc * (double)ap;
    }
    if (MODE != 0) {
      store_partial(q, red, a.part + chunk);
      __syncthreads();
    }
  }
  if (MODE == 0) return;
  if (!last_arrival(&h->ticket, &last)) return;
  if (threadIdx.x >= B3GS_WAVE) return;
  const double pap = fold_partials(a.part, g.nb);
  if (threadIdx.x) return;
  h->pap = pap;
  if (pap == 0.0) {
    h->done = 1;
  } else {
    const double alpha = h->rr / pap;
    h->alpha = alpha;
    h->af = (float)alpha;
  }
  __hip_atomic_store(&h->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TPB) update_kernel(CgArgs a) {
  __shared__ double red[TPB / B3GS_WAVE];
  __shared__ uint32_t last;
  const Grid& g = a.g;
  Head* h = a.head;
  if (h->done) return;
  const float af = h->af;
  for (uint32_t chunk = blockIdx.x; chunk < g.nb; chunk += gridDim.x) {
    const uint32_t idx = chunk * TPB + threadIdx.x;
    double q = 0.0;
    if (idx < g.n) {
      const float t = af * a.pin[idx];
      a.x[idx] = a.x[idx] + t;
      const float u = af * a.out[idx];
      const float rn = a.r[idx] - u;
      a.r[idx] = rn;
      q = (double)rn * (double)rn;
    }
    store_partial(q, red, a.part + chunk);
    __syncthreads();
  }
  if (!last_arrival(&h->ticket, &last)) return;
  if (threadIdx.x >= B3GS_WAVE) return;
  const double rn = fold_partials(a.part, g.nb);
  if (threadIdx.x) return;
  const double beta = rn / h->rr;
  h->beta = beta;
  h->bf = (float)beta;
  h->rr = rn;
  h->iterations = h->iterations + 1;
  if (rn <= h->thr) h->done = 1;
  __hip_atomic_store(&h->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- level and volume --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) iso_part_kernel(Grid g, const float* __restrict__ density, const float* __restrict__ x, double* part) {
  __shared__ double red[TPB / B3GS_WAVE];
  const uint32_t idx = blockIdx.x * TPB + threadIdx.x;
  const double d = idx < g.n ? (double)density[idx] : 0.0;
  const double dx = idx < g.n ? d * (double)x[idx] : 0.0;
  store_partial(dx, red, part + blockIdx.x);
  __syncthreads();
  store_partial(d, red, part + g.nb + blockIdx.x);
}

__global__ void __launch_bounds__(B3GS_WAVE) iso_kernel(Head* h, const double* part, uint32_t nb) {
  const double num = fold_partials(part, nb), den = fold_partials(part + nb, nb);
  if (threadIdx.x) return;
  h->num = num, h->den = den;
  h->iso = (float)(num / den);
}

__global__ void __launch_bounds__(TPB) level_kernel(Grid g, const Head* h, const float* __restrict__ x, float* __restrict__ tsdf) {
  const uint32_t idx = blockIdx.x * TPB + threadIdx.x;
  if (idx < g.n) tsdf[idx] = x[idx] - h->iso;
}

// out = the sum of in over [c - spread, c + spread] along one axis (stride `step` nodes, `len` nodes long), clipped to the grid,
// in index order from +0
__global__ void __launch_bounds__(TPB) box_kernel(uint32_t n, uint32_t step, int32_t len, int32_t spread, const float* __restrict__ in,
                                                  float* __restrict__ out) {
  const uint32_t idx = blockIdx.x * TPB + threadIdx.x;
  if (idx >= n) return;
  const int c = (int)(idx / step % (uint32_t)len);
  const int lo = c - spread < 0 ? 0 : c - spread, hi = c + spread > len - 1 ? len - 1 : c + spread;
  float acc = 0.0f;
  for (int q = lo; q <= hi; q++) acc = acc + in[(int64_t)idx + (int64_t)(q - c) * (int64_t)step];
  out[idx] = acc;
}

}  // namespace

// ---- entry points ------------------------------------------------------------------------------------------------------
extern "C" size_t b3gs_oriented_points_workspace_bytes(int32_t nviews, int32_t W, int32_t H) {
  int64_t npix;
  size_t total;
  return points_layout(nviews, W, H, &npix, &total) ? total : 0;
}

extern "C" int b3gs_oriented_points_batch(int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H, int32_t stride, float alpha_min,
                                          float rel_jump, float min_cos, int32_t median, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_oriented_points_batch";
  PointArgs a;
  if (int rc = points_args(what, nviews, views, W, H, stride, alpha_min, rel_jump, min_cos, median, workspace, &a)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = blocks_of(a.npix);
  hipLaunchKernelGGL(points_count_kernel, dim3(nb), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(points_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, s, a.bsum, (int)nb, a.total);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_oriented_points_emit(int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H, int32_t stride, float alpha_min,
                                         float rel_jump, float min_cos, int32_t median, void* workspace, int64_t npoints, float* points,
                                         float* normals, float* weights, float* colours, b3gs_stream_t stream) {
  static const char* what = "b3gs_oriented_points_emit";
  PointArgs a;
  if (int rc = points_args(what, nviews, views, W, H, stride, alpha_min, rel_jump, min_cos, median, workspace, &a)) return rc;
  if (npoints < 0 || npoints > a.npix) return b3gs_fail(B3GS_ERR_ARG, what, "the count is 0 .. the number of pixels");
  if (npoints == 0) return B3GS_OK;
  if (!points || !normals || !weights || !colours) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output");
  a.npoints = npoints;
  a.points = points, a.normals = normals, a.weights = weights, a.colours = colours;
  hipLaunchKernelGGL(points_emit_kernel, dim3(blocks_of(a.npix)), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_poisson_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t nsamples) {
  if (!grid_sizes(nx, ny, nz, nsamples)) return 0;
  return ws_carve(nullptr, (int64_t)nx * ny * nz, nsamples, nullptr);
}

extern "C" int b3gs_poisson_splat(const B3gsTsdfVolume* grid, int64_t nsamples, const float* points, const float* normals,
                                  const float* weights, float* density, float* vector, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_poisson_splat";
  Grid g;
  if (int rc = grid_of(grid, what, &g)) return rc;
  if (nsamples < 0 || nsamples >= ((int64_t)1 << 31)) return b3gs_fail(B3GS_ERR_ARG, what, "0 .. 2^31 - 1 samples");
  if (nsamples > 0 && (!points || !normals || !weights)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL sample pointer");
  if (!density || !vector) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output");
  if (int rc = check_ws(workspace, what)) return rc;
  Ws w;
  ws_carve(static_cast<char*>(workspace), g.n, nsamples, &w);
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(workspace, 0, 256, s);
  hipLaunchKernelGGL(head_samples_kernel, dim3(1), dim3(1), 0, s, w.head, nsamples);
  (void)hipMemsetAsync(w.cstart, 0, (size_t)g.n * sizeof(uint32_t), s);
  (void)hipMemsetAsync(w.cend, 0, (size_t)g.n * sizeof(uint32_t), s);
  if (nsamples > 0) {
    const unsigned nbs = blocks_of(nsamples);
    hipLaunchKernelGGL(splat_key_kernel, dim3(nbs), dim3(TPB), 0, s, g, nsamples, points, w.vkey, w.frac, w.head);
    b3gs_launch_sort_u32_index(w.vkey, w.skey, w.sval, (uint32_t)nsamples, w.hist, s);
    hipLaunchKernelGGL(splat_range_kernel, dim3(nbs), dim3(TPB), 0, s, nsamples, (const uint32_t*)w.skey[0], w.cstart, w.cend);
  }
  hipLaunchKernelGGL(splat_gather_kernel, dim3(g.nb), dim3(TPB), 0, s, g, (const uint32_t*)w.sval[0], (const uint32_t*)w.cstart,
                     (const uint32_t*)w.cend, (const float*)w.frac, normals, weights, density, vector);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_poisson_apply(const B3gsTsdfVolume* grid, const float* density, float screen, const float* x, float* out,
                                  b3gs_stream_t stream) {
  static const char* what = "b3gs_poisson_apply";
  Grid g;
  if (int rc = grid_of(grid, what, &g)) return rc;
  if (!(screen > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the screening weight is positive");
  if (!density || !x || !out || x == out) return b3gs_fail(B3GS_ERR_ARG, what, "density, x and a separate out are needed");
  CgArgs a = {};
  a.g = g, a.density = density, a.screen = screen, a.pin = x, a.out = out;
  hipLaunchKernelGGL(stencil_kernel<0>, dim3(g.nb), dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_poisson_solve(const B3gsTsdfVolume* grid, const float* density, const float* vector, float screen, int32_t iters,
                                  float tol, int32_t max_blocks, float* rhs, float* x, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_poisson_solve";
  Grid g;
  if (int rc = grid_of(grid, what, &g)) return rc;
  if (!(screen > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the screening weight is positive");
  if (iters < 0) return b3gs_fail(B3GS_ERR_ARG, what, "the iteration count is not negative");
  if (!(tol >= 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the tolerance is not negative");
  if (max_blocks < 0) return b3gs_fail(B3GS_ERR_ARG, what, "max_blocks is not negative");
  if (!density || !vector || !rhs || !x) return b3gs_fail(B3GS_ERR_ARG, what, "NULL array");
  if (int rc = check_ws(workspace, what)) return rc;
  Ws w;
  ws_carve(static_cast<char*>(workspace), g.n, 0, &w);
  hipStream_t s = (hipStream_t)stream;
  CgArgs a = {};
  a.g = g, a.head = w.head, a.density = density, a.screen = screen;
  a.x = x, a.r = w.r, a.vec = vector, a.rhs = rhs, a.part = w.part, a.out = w.ap;
  a.pout = w.p[0];
  hipLaunchKernelGGL(rhs_kernel, dim3(g.nb), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(start_kernel, dim3(1), dim3(B3GS_WAVE), 0, s, w.head, (const double*)w.part, g.nb, (double)tol * (double)tol);
  // fewer workgroups than chunks: fewer arrivals to count, the same partials (a workgroup walks chunks b, b + launch, ..)
  const unsigned cap = max_blocks > 0 ? (unsigned)max_blocks : (unsigned)DEFAULT_BLOCKS;
  const unsigned launch = cap < g.nb ? cap : g.nb;
  int cur = 0;                                                        // the buffer that holds the direction
  for (int it = 0; it < iters; it++) {
    a.pin = w.p[cur];
    if (it == 0) {
      hipLaunchKernelGGL(stencil_kernel<1>, dim3(launch), dim3(TPB), 0, s, a);
    } else {
      a.pout = w.p[cur ^ 1];
      hipLaunchKernelGGL(stencil_kernel<2>, dim3(launch), dim3(TPB), 0, s, a);
      cur ^= 1;
      a.pin = w.p[cur];
    }
    hipLaunchKernelGGL(update_kernel, dim3(launch), dim3(TPB), 0, s, a);
  }
  return b3gs_launch_status(what);
}

extern "C" int b3gs_poisson_volume(const B3gsTsdfVolume* volume, const float* density, const float* x, int32_t spread, void* workspace,
                                   b3gs_stream_t stream) {
  static const char* what = "b3gs_poisson_volume";
  Grid g;
  if (int rc = grid_of(volume, what, &g)) return rc;
  if (!volume->tsdf || !volume->weight || !volume->rgb) return b3gs_fail(B3GS_ERR_ARG, what, "NULL volume pointer");
  if (!density || !x) return b3gs_fail(B3GS_ERR_ARG, what, "NULL array");
  if (spread < 0 || spread > B3GS_MAX_TSDF_DIM) return b3gs_fail(B3GS_ERR_ARG, what, "the spread is 0 .. 1024");
  if (int rc = check_ws(workspace, what)) return rc;
  Ws w;
  ws_carve(static_cast<char*>(workspace), g.n, 0, &w);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(iso_part_kernel, dim3(g.nb), dim3(TPB), 0, s, g, density, x, w.part);
  hipLaunchKernelGGL(iso_kernel, dim3(1), dim3(B3GS_WAVE), 0, s, w.head, (const double*)w.part, g.nb);
  hipLaunchKernelGGL(level_kernel, dim3(g.nb), dim3(TPB), 0, s, g, (const Head*)w.head, x, volume->tsdf);
  // the support of the samples: x, then y, then z (the direction arrays of the solver are free now)
  hipLaunchKernelGGL(box_kernel, dim3(g.nb), dim3(TPB), 0, s, g.n, 1u, g.nx, spread, density, w.p[0]);
  hipLaunchKernelGGL(box_kernel, dim3(g.nb), dim3(TPB), 0, s, g.n, (uint32_t)g.nx, g.ny, spread, (const float*)w.p[0], w.p[1]);
  hipLaunchKernelGGL(box_kernel, dim3(g.nb), dim3(TPB), 0, s, g.n, g.nxy, g.nz, spread, (const float*)w.p[1], volume->weight);
  (void)hipMemsetAsync(volume->rgb, 0, (size_t)g.n * 3 * sizeof(float), s);
  return b3gs_launch_status(what);
}
