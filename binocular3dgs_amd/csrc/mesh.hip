// A triangle mesh of a trained scene (ABI 17; binocular3dgs_amd/mesh.py): TSDF fusion of rendered
// depth, marching tetrahedra with welded vertices.  include/b3gs_raster.h states the arithmetic; tests/mesh_ref.py restates it.
//   integrate   grid (x blocks, ny, nz), 256 threads along x: a thread owns one voxel, keeps its five floats in registers and
//               walks the (up to 8) views of the call in index order -- per view 12 multiply-adds of wave-uniform camera words,
//               two divisions, and two gathers (alpha, depth; three more for a voxel inside the band).  The camera table is a
//               kernel argument: scalar registers, no load.  A voxel no view reached is not written back.
//   cells       thread = voxel = the cell whose corner (0,0,0) it is: 8 weights and signs -> valid bit | triangle count (a byte)
//   edges       thread = voxel: which of its 7 edges changes sign AND lies in a valid cell (a byte).  Both write block sums,
//               from wave ballots of the count bits and popcounts.
//   scan        two blocks (vertices, triangles): exclusive scan of the block sums in place, 1024 at a time (one scan chunk =
//               1024 blocks = 2^18 voxels), int64 totals to the head of the workspace
//   vertices    thread = voxel: global rank = block offset + ballot rank -> the voxel's first vertex id (kept per voxel for the
//               triangles), positions and colours of its slots
//   triangles   thread = cell: rank likewise; per tetrahedron the case table names, per triangle corner, the owning corner of
//               the cell and the edge slot: id = first id of that voxel + popcount(mask below the slot)
// The 6 x 16 case table is built at compile time from the orientation rule (below) and lives in constant memory.
// Every float statement is one operation, in the order of tests/mesh_ref.py (the Makefile compiles with -ffp-contract=off).
#include "b3gs_internal.h"

namespace {

constexpr int TPB = 256;
constexpr int SCAN_TPB = B3GS_SCAN_TPB;
constexpr int NV = B3GS_MAX_TSDF_VIEWS;

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the case table ----------------------------------------------------------------------------------------------------
// Corner c of a cell is (c & 1, c >> 1 & 1, c >> 2).  Tetrahedron t belongs to the t-th permutation (a, b, c) of the axes and
// has the corners 0, e_a, e_a + e_b, 7.  Case bit p: corner p of the tetrahedron is inside.  One inside (or one outside)
// corner p with the others q < r < s gives the triangle (pq, pr, ps); two inside a < b and two outside c < d give the quad
// ac, ad, bd, bc as (ac, ad, bd), (ac, bd, bc).  With the vertices at the edge midpoints, the normal of the first triangle is
// held against (centroid of the outside corners - centroid of the inside corners); when it points the other way, the second
// and third vertex of every triangle of the case change places.  A triangle corner is stored as the cell corner at the
// lower end of its edge (bits 0-2) and the slot of the edge's direction (bits 3-5).
struct Tables {
  uint8_t corner[6][4];
  uint8_t ntri[6][16];
  uint8_t vert[6][16][6];
};

constexpr int slot_of(int dir) { return dir == 1 ? 0 : dir == 2 ? 1 : dir == 4 ? 2 : dir == 3 ? 3 : dir == 5 ? 4 : dir == 6 ? 5 : 6; }

constexpr Tables make_tables() {
  Tables T{};
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int t = 0; t < 6; t++) {
    int cn[4] = {0, 1 << perm[t][0], (1 << perm[t][0]) | (1 << perm[t][1]), 7};
    for (int p = 0; p < 4; p++) T.corner[t][p] = (uint8_t)cn[p];
    for (int cs = 1; cs < 15; cs++) {
      int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
      for (int p = 0; p < 4; p++) {
        if (cs >> p & 1) in[ni++] = p;
        else out[no++] = p;
      }
      int e[6][2] = {};   // triangle corners as pairs of tetrahedron corners
      int n = 0;
      if (ni == 1 || no == 1) {
        const int p = ni == 1 ? in[0] : out[0];
        const int* o = ni == 1 ? out : in;
        for (int q = 0; q < 3; q++) e[q][0] = p, e[q][1] = o[q];
        n = 1;
      } else {
        const int a = in[0], b = in[1], c = out[0], d = out[1];
        const int quad[6][2] = {{a, c}, {a, d}, {b, d}, {a, c}, {b, d}, {b, c}};
        for (int q = 0; q < 6; q++) e[q][0] = quad[q][0], e[q][1] = quad[q][1];
        n = 2;
      }
      // orientation of the first triangle, in integers (midpoints times 2)
      int m[3][3] = {};
      for (int q = 0; q < 3; q++)
        for (int x = 0; x < 3; x++) m[q][x] = (cn[e[q][0]] >> x & 1) + (cn[e[q][1]] >> x & 1);
      const int ux = m[1][0] - m[0][0], uy = m[1][1] - m[0][1], uz = m[1][2] - m[0][2];
      const int vx = m[2][0] - m[0][0], vy = m[2][1] - m[0][1], vz = m[2][2] - m[0][2];
      const int nrm[3] = {uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx};
      int dot = 0;
      for (int x = 0; x < 3; x++) {
        int so = 0, si = 0;
        for (int q = 0; q < no; q++) so += cn[out[q]] >> x & 1;
        for (int q = 0; q < ni; q++) si += cn[in[q]] >> x & 1;
        dot += nrm[x] * (ni * so - no * si);
      }
      T.ntri[t][cs] = (uint8_t)n;
      for (int k = 0; k < n; k++)
        for (int q = 0; q < 3; q++) {
          const int src = 3 * k + (dot < 0 ? (q == 0 ? 0 : 3 - q) : q);
          const int lo = cn[e[src][0] < e[src][1] ? e[src][0] : e[src][1]], hi = cn[e[src][0] < e[src][1] ? e[src][1] : e[src][0]];
          T.vert[t][cs][3 * k + q] = (uint8_t)(lo | (slot_of(hi & ~lo) << 3));
        }
    }
  }
  return T;
}

__constant__ Tables TAB = make_tables();

// direction bits of the 7 slots: x, y, z, xy, xz, yz, xyz
__constant__ uint8_t SLOT_DIR[7] = {1, 2, 4, 3, 5, 6, 7};

// ---- integration -------------------------------------------------------------------------------------------------------
struct IntegrateArgs {
  B3gsTsdfVolume vol;
  int32_t n, W, H;
  float truncation, near, alpha_min;
  B3gsTsdfView v[NV];
};

__global__ void __launch_bounds__(TPB) integrate_kernel(IntegrateArgs a) {
  const B3gsTsdfVolume& g = a.vol;
  const int i = blockIdx.x * TPB + threadIdx.x, j = blockIdx.y, k = blockIdx.z;
  if (i >= g.nx) return;
  const size_t idx = ((size_t)k * g.ny + j) * g.nx + i;
  const float px = g.origin[0] + ((float)i + 0.5f) * g.voxel;
  const float py = g.origin[1] + ((float)j + 0.5f) * g.voxel;
  const float pz = g.origin[2] + ((float)k + 0.5f) * g.voxel;
  float tsdf = g.tsdf[idx], w = g.weight[idx];
  float r = g.rgb[3 * idx], gr = g.rgb[3 * idx + 1], b = g.rgb[3 * idx + 2];
  const float w_in = w;
  const float cx = 0.5f * (float)a.W - 0.5f, cy = 0.5f * (float)a.H - 0.5f;
  const float xmax = (float)(a.W - 1), ymax = (float)(a.H - 1);
  const size_t plane = (size_t)a.W * a.H;
  for (int v = 0; v < a.n; v++) {
    const B3gsTsdfView& c = a.v[v];
    const float x = ((c.rot[0] * px + c.rot[1] * py) + c.rot[2] * pz) + c.trans[0];
    const float y = ((c.rot[3] * px + c.rot[4] * py) + c.rot[5] * pz) + c.trans[1];
    const float z = ((c.rot[6] * px + c.rot[7] * py) + c.rot[8] * pz) + c.trans[2];
    if (!(z > a.near)) continue;
    const float un = x / z, vn = y / z;
    const float uf = rintf(c.fx * un + cx), vf = rintf(c.fy * vn + cy);
    if (!(uf >= 0.0f && uf <= xmax && vf >= 0.0f && vf <= ymax)) continue;          // (NaN: skipped)
    const size_t pix = (size_t)(int)vf * a.W + (int)uf;
    const float al = c.alpha[pix];
    if (!(al >= a.alpha_min)) continue;
    const float d = c.depth[pix] / al;
    const float sdf = d - z;
    if (!(sdf >= -a.truncation)) continue;
    const float val = fminf(1.0f, sdf / a.truncation);
    const float wn = w + 1.0f;
    tsdf = (tsdf * w + val) / wn;
    r = (r * w + c.colour[pix]) / wn;
    gr = (gr * w + c.colour[plane + pix]) / wn;
    b = (b * w + c.colour[2 * plane + pix]) / wn;
    w = wn;
  }
  if (w != w_in) {
    g.tsdf[idx] = tsdf;
    g.weight[idx] = w;
    g.rgb[3 * idx] = r;
    g.rgb[3 * idx + 1] = gr;
    g.rgb[3 * idx + 2] = b;
  }
}

// ---- extraction --------------------------------------------------------------------------------------------------------
struct MeshArgs {
  B3gsTsdfVolume vol;
  float min_weight;
  int64_t n;                        // voxels
  int32_t nb;                       // blocks of TPB voxels
  int64_t* totals;                  // [2] vertices, triangles
  uint8_t* cell;                    // [n] bit 7: valid cell; bits 0-3: its triangles
  uint8_t* vmask;                   // [n] bit s: slot s holds a vertex
  int32_t* vbase;                   // [n] id of the voxel's first vertex (written by emit)
  uint32_t* bsum;                   // [2][nb] block sums, then their exclusive scan (vertices, triangles)
  int64_t nverts, ntris;            // emit: rows of the outputs
  float* vertices;
  uint8_t* colours;
  int32_t* faces;
};

// (the ranks inside a block and the scan of the block sums: b3gs_internal.h, shared with meshtools.hip)
__device__ __forceinline__ int block_rank(int cnt, int* wave_n, int* total) { return b3gs_block_rank<TPB, 4>(cnt, wave_n, total); }

__device__ __forceinline__ size_t corner_offset(const B3gsTsdfVolume& g, int c) {
  return (size_t)(c & 1) + (size_t)(c >> 1 & 1) * g.nx + (size_t)(c >> 2) * g.nx * g.ny;
}

__global__ void __launch_bounds__(TPB) cells_kernel(MeshArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const B3gsTsdfVolume& g = a.vol;
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int cnt = 0;
  if (v < a.n) {
    const int i = (int)(v % g.nx), j = (int)(v / g.nx % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
    uint8_t out = 0;
    if (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) {
      bool valid = true;
      int bits = 0;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const size_t at = (size_t)v + corner_offset(g, c);
        valid = valid && g.weight[at] >= a.min_weight;
        bits |= (g.tsdf[at] < 0.0f ? 1 : 0) << c;
      }
      if (valid) {
        for (int t = 0; t < 6; t++) {
          int cs = 0;
#pragma unroll
          for (int p = 0; p < 4; p++) cs |= (bits >> TAB.corner[t][p] & 1) << p;
          cnt += TAB.ntri[t][cs];
        }
        out = (uint8_t)(0x80 | cnt);
      }
    }
    a.cell[v] = out;
  }
  int total;
  block_rank(cnt, wave_n, &total);
  if (threadIdx.x == 0) a.bsum[(size_t)a.nb + blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(TPB) edges_kernel(MeshArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const B3gsTsdfVolume& g = a.vol;
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  int mask = 0;
  if (v < a.n) {
    const int i = (int)(v % g.nx), j = (int)(v / g.nx % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
    const bool in0 = g.tsdf[v] < 0.0f;
    for (int s = 0; s < 7; s++) {
      const int dir = SLOT_DIR[s];
      const int dx = dir & 1, dy = dir >> 1 & 1, dz = dir >> 2;
      if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz) continue;
      if ((g.tsdf[(size_t)v + corner_offset(g, dir)] < 0.0f) == in0) continue;
      // the cells around the edge: along an axis the edge does not move on, the cell at this index and the one below it
      bool used = false;
      for (int c = 0; c < 8; c++) {
        if (c & dir) continue;
        const int ci = i - (c & 1), cj = j - (c >> 1 & 1), ck = k - (c >> 2);
        if (ci < 0 || cj < 0 || ck < 0 || ci >= g.nx - 1 || cj >= g.ny - 1 || ck >= g.nz - 1) continue;
        used = used || (a.cell[(size_t)v - corner_offset(g, c)] & 0x80);
      }
      if (used) mask |= 1 << s;
    }
    a.vmask[v] = (uint8_t)mask;
  }
  int total;
  block_rank(__popc(mask), wave_n, &total);
  if (threadIdx.x == 0) a.bsum[blockIdx.x] = (uint32_t)total;
}

// block 0: vertices, block 1: triangles.  The scanned offsets are 32-bit words: they wrap only when the total does not fit
// int32, which the caller refuses before anything is emitted.
__global__ void __launch_bounds__(SCAN_TPB) scan_kernel(MeshArgs a) {
  b3gs_scan_block_sums(a.bsum + (size_t)blockIdx.x * a.nb, a.nb, a.totals + blockIdx.x);
}

__global__ void __launch_bounds__(TPB) vertices_kernel(MeshArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const B3gsTsdfVolume& g = a.vol;
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int mask = v < a.n ? a.vmask[v] : 0;
  int total;
  int64_t id = (int64_t)a.bsum[blockIdx.x] + block_rank(__popc(mask), wave_n, &total);
  if (v >= a.n) return;
  a.vbase[v] = (int32_t)id;
  if (!mask) return;
  const int i = (int)(v % g.nx), j = (int)(v / g.nx % g.ny), k = (int)(v / ((int64_t)g.nx * g.ny));
  const float p0[3] = {g.origin[0] + ((float)i + 0.5f) * g.voxel, g.origin[1] + ((float)j + 0.5f) * g.voxel,
                       g.origin[2] + ((float)k + 0.5f) * g.voxel};
  const float d0 = g.tsdf[v];
  const float c0[3] = {g.rgb[3 * (size_t)v], g.rgb[3 * (size_t)v + 1], g.rgb[3 * (size_t)v + 2]};
  for (int s = 0; s < 7; s++) {
    if (!(mask >> s & 1)) continue;
    if (id >= a.nverts) return;                                                     // (the outputs hold nverts rows)
    const int dir = SLOT_DIR[s];
    const size_t at = (size_t)v + corner_offset(g, dir);
    const float p1[3] = {g.origin[0] + ((float)(i + (dir & 1)) + 0.5f) * g.voxel, g.origin[1] + ((float)(j + (dir >> 1 & 1)) + 0.5f) * g.voxel,
                         g.origin[2] + ((float)(k + (dir >> 2)) + 0.5f) * g.voxel};
    const float d1 = g.tsdf[at];
    const float t = d0 / (d0 - d1);
#pragma unroll
    for (int x = 0; x < 3; x++) {
      a.vertices[3 * id + x] = p0[x] + t * (p1[x] - p0[x]);
      const float c1 = g.rgb[3 * at + x];
      const float col = (c0[x] + t * (c1 - c0[x])) * 255.0f;
      a.colours[3 * id + x] = (uint8_t)rintf(fminf(fmaxf(col, 0.0f), 255.0f));
    }
    id++;
  }
}

__global__ void __launch_bounds__(TPB) triangles_kernel(MeshArgs a) {
  __shared__ int wave_n[TPB / B3GS_WAVE];
  const B3gsTsdfVolume& g = a.vol;
  const int64_t v = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const int cnt = v < a.n ? (a.cell[v] & 0x0f) : 0;
  int total;
  int64_t tri = (int64_t)a.bsum[(size_t)a.nb + blockIdx.x] + block_rank(cnt, wave_n, &total);
  if (!cnt) return;
  int bits = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) bits |= (g.tsdf[(size_t)v + corner_offset(g, c)] < 0.0f ? 1 : 0) << c;
  for (int t = 0; t < 6; t++) {
    int cs = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) cs |= (bits >> TAB.corner[t][p] & 1) << p;
    const int n = TAB.ntri[t][cs];
    for (int q = 0; q < 3 * n; q++) {
      if (q % 3 == 0 && tri + q / 3 >= a.ntris) return;                             // (the output holds ntris rows)
      const int code = TAB.vert[t][cs][q];
      const size_t owner = (size_t)v + corner_offset(g, code & 7);
      const int slot = code >> 3;
      a.faces[3 * tri + q] = a.vbase[owner] + __popc(a.vmask[owner] & ((1 << slot) - 1));
    }
    tri += n;
  }
}

struct Layout {
  int64_t n;
  int32_t nb;
  size_t cell, vmask, vbase, bsum, total;
};

static bool layout(int64_t nx, int64_t ny, int64_t nz, Layout* l) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > B3GS_MAX_TSDF_DIM || ny > B3GS_MAX_TSDF_DIM || nz > B3GS_MAX_TSDF_DIM) return false;
  l->n = nx * ny * nz;
  l->nb = (int32_t)((l->n + TPB - 1) / TPB);
  size_t at = 256;                                                                  // the two totals
  l->cell = at, at += align256((size_t)l->n);
  l->vmask = at, at += align256((size_t)l->n);
  l->vbase = at, at += align256((size_t)l->n * sizeof(int32_t));
  l->bsum = at, at += align256((size_t)2 * l->nb * sizeof(uint32_t));
  l->total = at;
  return true;
}

static int check_volume(const B3gsTsdfVolume* g, const char* what) {
  if (!g) return b3gs_fail(B3GS_ERR_ARG, what, "volume is NULL");
  if (g->nx < 1 || g->ny < 1 || g->nz < 1 || g->nx > B3GS_MAX_TSDF_DIM || g->ny > B3GS_MAX_TSDF_DIM || g->nz > B3GS_MAX_TSDF_DIM)
    return b3gs_fail(B3GS_ERR_ARG, what, "every dimension of the volume is 1 .. 1024");
  if (!(g->voxel > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the voxel size is positive");
  if (!g->tsdf || !g->weight || !g->rgb) return b3gs_fail(B3GS_ERR_ARG, what, "NULL volume pointer");
  return B3GS_OK;
}

static MeshArgs mesh_args(const B3gsTsdfVolume& g, const Layout& l, void* workspace) {
  char* ws = static_cast<char*>(workspace);
  MeshArgs a = {};
  a.vol = g;
  a.n = l.n;
  a.nb = l.nb;
  a.totals = reinterpret_cast<int64_t*>(ws);
  a.cell = reinterpret_cast<uint8_t*>(ws + l.cell);
  a.vmask = reinterpret_cast<uint8_t*>(ws + l.vmask);
  a.vbase = reinterpret_cast<int32_t*>(ws + l.vbase);
  a.bsum = reinterpret_cast<uint32_t*>(ws + l.bsum);
  return a;
}

}  // namespace

extern "C" int b3gs_tsdf_integrate_batch(const B3gsTsdfVolume* volume, int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H,
                                         float truncation, float near, float alpha_min, b3gs_stream_t stream) {
  static const char* what = "b3gs_tsdf_integrate_batch";
  if (int rc = check_volume(volume, what)) return rc;
  if (nviews < 1 || nviews > NV) return b3gs_fail(B3GS_ERR_ARG, what, "1 .. 8 views per call");
  if (!views) return b3gs_fail(B3GS_ERR_ARG, what, "views is NULL");
  if (W < 1 || H < 1 || (int64_t)W * H > ((int64_t)1 << 30)) return b3gs_fail(B3GS_ERR_ARG, what, "the images hold 1 .. 2^30 pixels");
  if (!(truncation > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "the truncation is positive");
  if (!(near >= 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "near is not negative");
  if (!(alpha_min > 0.f)) return b3gs_fail(B3GS_ERR_ARG, what, "alpha_min is positive");
  IntegrateArgs a = {};
  a.vol = *volume;
  a.n = nviews, a.W = W, a.H = H;
  a.truncation = truncation, a.near = near, a.alpha_min = alpha_min;
  for (int v = 0; v < nviews; v++) {
    if (!views[v].depth || !views[v].alpha || !views[v].colour) return b3gs_fail(B3GS_ERR_ARG, what, "NULL image pointer");
    a.v[v] = views[v];
  }
  const dim3 grid((unsigned)((volume->nx + TPB - 1) / TPB), (unsigned)volume->ny, (unsigned)volume->nz);
  hipLaunchKernelGGL(integrate_kernel, grid, dim3(TPB), 0, (hipStream_t)stream, a);
  return b3gs_launch_status(what);
}

extern "C" size_t b3gs_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  Layout l;
  return layout(nx, ny, nz, &l) ? l.total : 0;
}

extern "C" int b3gs_mesh_count(const B3gsTsdfVolume* volume, float min_weight, void* workspace, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_count";
  if (int rc = check_volume(volume, what)) return rc;
  if (min_weight != min_weight) return b3gs_fail(B3GS_ERR_ARG, what, "min_weight is NaN");
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  Layout l;
  if (!layout(volume->nx, volume->ny, volume->nz, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "bad sizes");
  MeshArgs a = mesh_args(*volume, l, workspace);
  a.min_weight = min_weight;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cells_kernel, dim3((unsigned)l.nb), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(edges_kernel, dim3((unsigned)l.nb), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(scan_kernel, dim3(2), dim3(SCAN_TPB), 0, s, a);
  return b3gs_launch_status(what);
}

extern "C" int b3gs_mesh_emit(const B3gsTsdfVolume* volume, void* workspace, int64_t nverts, int64_t ntris, float* vertices,
                              uint8_t* colours, int32_t* faces, b3gs_stream_t stream) {
  static const char* what = "b3gs_mesh_emit";
  if (int rc = check_volume(volume, what)) return rc;
  if (!workspace || ((uintptr_t)workspace & 255)) return b3gs_fail(B3GS_ERR_ARG, what, "a 256-byte aligned workspace is needed");
  if (nverts < 0 || ntris < 0) return b3gs_fail(B3GS_ERR_ARG, what, "negative count");
  if (nverts > INT32_MAX || ntris > INT32_MAX) return b3gs_fail(B3GS_ERR_ARG, what, "the mesh has more than 2^31 - 1 vertices or triangles: use a coarser volume");
  if ((nverts > 0 && (!vertices || !colours)) || (ntris > 0 && !faces)) return b3gs_fail(B3GS_ERR_ARG, what, "NULL output");
  if (nverts == 0 && ntris == 0) return B3GS_OK;
  Layout l;
  if (!layout(volume->nx, volume->ny, volume->nz, &l)) return b3gs_fail(B3GS_ERR_ARG, what, "bad sizes");
  MeshArgs a = mesh_args(*volume, l, workspace);
  a.nverts = nverts, a.ntris = ntris;
  a.vertices = vertices, a.colours = colours, a.faces = faces;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(vertices_kernel, dim3((unsigned)l.nb), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(triangles_kernel, dim3((unsigned)l.nb), dim3(TPB), 0, s, a);
  return b3gs_launch_status(what);
}
