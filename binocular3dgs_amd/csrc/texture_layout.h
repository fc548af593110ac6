// The atlas of a textured mesh (include/b3gs_raster.h, section "texturing an extracted mesh", statement 1): integer arithmetic
// only, the same on the host and on the device, and restated in python (binocular3dgs_amd/mesh_texture.py) and in
// tests/texture_ref.py.  Plain C++ with no dependency, so that a stand-alone host program can include it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define B3GS_TEX_HD __host__ __device__ __forceinline__
#else
#define B3GS_TEX_HD static inline
#endif

#define B3GS_TEX_MIN_CELL 4
#define B3GS_TEX_MAX_CELL 256
#define B3GS_TEX_MAX_SIDE 16384

struct TexAtlas {
  int32_t n, Wt, Ht, cpr;                       // cell parameter, atlas size in texels, cells per row
  int64_t F;
};

// -> the atlas height for F triangles, cell parameter n and width Wt; 0 when F, n or Wt is out of range or the height would
// pass B3GS_TEX_MAX_SIDE
B3GS_TEX_HD int32_t tex_atlas_height(int64_t F, int32_t n, int32_t Wt) {
  if (F < 1 || F > INT32_MAX || n < B3GS_TEX_MIN_CELL || n > B3GS_TEX_MAX_CELL || Wt < n + 1 || Wt > B3GS_TEX_MAX_SIDE) return 0;
  const int64_t cpr = Wt / (n + 1), cells = (F + 1) / 2;
  const int64_t Ht = (int64_t)n * ((cells + cpr - 1) / cpr);
  return Ht > B3GS_TEX_MAX_SIDE ? 0 : (int32_t)Ht;
}
// the largest cell parameter whose atlas of width Wt holds F triangles; 0: none does
B3GS_TEX_HD int32_t tex_largest_cell(int64_t F, int32_t Wt) {
  for (int32_t n = B3GS_TEX_MAX_CELL; n >= B3GS_TEX_MIN_CELL; n--)
    if (tex_atlas_height(F, n, Wt)) return n;
  return 0;
}

// Texel (X, Y) of the atlas -> its triangle (-1: the texel is in no cell, or in the half of a triangle past F) and its local
// indices (i, j) in the EVEN triangle's frame: the odd half of a cell is the even half under i -> n - i, j -> n - 1 - j.
B3GS_TEX_HD int64_t tex_owner(const TexAtlas& a, int32_t X, int32_t Y, int32_t* i, int32_t* j) {
  const int32_t cx = X / (a.n + 1), li = X - cx * (a.n + 1), cy = Y / a.n, lj = Y - cy * a.n;
  if (cx >= a.cpr) return -1;
  const int32_t odd = li + lj >= a.n;
  const int64_t f = 2 * ((int64_t)cy * a.cpr + cx) + odd;
  if (f >= a.F) return -1;
  *i = odd ? a.n - li : li, *j = odd ? a.n - 1 - lj : lj;
  return f;
}
// the texel-centre coordinates of the three corners of triangle f (whole numbers)
B3GS_TEX_HD void tex_corners(const TexAtlas& a, int64_t f, float* u, float* v) {
  const int64_t c = f >> 1;
  const int32_t x0 = (int32_t)(c % a.cpr) * (a.n + 1), y0 = (int32_t)(c / a.cpr) * a.n, n = a.n;
  if (f & 1) {
    u[0] = (float)(x0 + n), u[1] = (float)(x0 + 2), u[2] = (float)(x0 + n);
    v[0] = (float)(y0 + n - 1), v[1] = (float)(y0 + n - 1), v[2] = (float)(y0 + 1);
  } else {
    u[0] = (float)x0, u[1] = (float)(x0 + n - 2), u[2] = (float)x0;
    v[0] = (float)y0, v[1] = (float)y0, v[2] = (float)(y0 + n - 2);
  }
}
