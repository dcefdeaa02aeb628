// Operator 1's sampling geometry, written once: the affine_grid / grid_sample coordinate maths, the bilinear taps and their
// accumulate, the rotation's taps and their validity, where the paste and the crop of a sample land in the global map, and the
// block order and grid size of the gather kernels.  Included by wsmg_bev.hip (index, scatter, first rotation) and wsmg_bev_map.hip
// (global map: reset, fuse, crop, final rotation, retrieval).
//
// Every route of the operator is held bit-identical to the one it replaced (torch.equal in the tests), so every expression here is
// the same IEEE float32 operation in the same order wherever it is used, with FMA contraction disabled: both includers rely on the
// pragma below reaching to the end of their translation unit, and must keep their own `#pragma clang fp contract(off)` as well.
#pragma once
#include "wsmg_common.h"

#pragma clang fp contract(off)

namespace {

// ----------------------------------------------------------------------------- sampling grid maths
// affine_grid(align_corners=False) base coordinate: linspace(-1,1,W)[j] * (W-1) / W
__device__ __forceinline__ float base_coord(int j, int W) {
  float step = 2.0f / (float)(W - 1);
  float v = (j < W / 2) ? -1.0f + step * (float)j : 1.0f - step * (float)(W - 1 - j);
  return v * (float)(W - 1) / (float)W;
}
// grid_sample(align_corners=False) un-normalisation
__device__ __forceinline__ float unnorm(float g, int W) { return ((g + 1.0f) * (float)W - 1.0f) / 2.0f; }

struct Taps {
  int x0, y0;          // north-west corner
  float w00, w01, w10, w11;  // nw, ne, sw, se
};
__device__ __forceinline__ Taps make_taps(float ix, float iy) {
  Taps t;
  float fx0 = floorf(ix), fy0 = floorf(iy);
  t.x0 = (int)fx0;
  t.y0 = (int)fy0;
  float x1 = fx0 + 1.0f, y1 = fy0 + 1.0f;
  t.w00 = (x1 - ix) * (y1 - iy);
  t.w01 = (ix - fx0) * (y1 - iy);
  t.w10 = (x1 - ix) * (iy - fy0);
  t.w11 = (ix - fx0) * (iy - fy0);
  return t;
}
// weight of tap k = 2 * (row: 0 north, 1 south) + (column: 0 west, 1 east); the tap's pixel is (y0 + (k >> 1), x0 + (k & 1))
__device__ __forceinline__ float tap_w(const Taps& t, int k) { return k == 0 ? t.w00 : k == 1 ? t.w01 : k == 2 ? t.w10 : t.w11; }
// one tap of four channels: v += q * w, a product and a sum per lane
__device__ __forceinline__ void acc4(f32x4& v, f32x4 q, float w) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] += q[j] * w;
}

struct Rot { float c, s; };
// rotation of an E x E map: gx = bx*c + by*s ; gy = -bx*s + by*c
__device__ __forceinline__ Taps rot_taps(int x, int y, int E, Rot r) {
  float bx = base_coord(x, E), by = base_coord(y, E);
  float gx = bx * r.c + by * r.s;
  float gy = bx * (-r.s) + by * r.c;
  return make_taps(unnorm(gx, E), unnorm(gy, E));
}
// which columns (x0, x0 + 1) and rows (y0, y0 + 1) of a rotation's taps lie inside the E x E map: tap k counts when its row and
// its column do (zero padding of grid_sample).  (Four references, not a struct: the compiler packs a struct of four bools into
// one register and unpacks it at every use.)
__device__ __forceinline__ void taps_in(const Taps& t, int E, bool& x0ok, bool& x1ok, bool& y0ok, bool& y1ok) {
  x0ok = t.x0 >= 0 && t.x0 < E;
  x1ok = t.x0 + 1 >= 0 && t.x0 + 1 < E;
  y0ok = t.y0 >= 0 && t.y0 < E;
  y1ok = t.y0 + 1 >= 0 && t.y0 + 1 < E;
}

// Block order of the gather kernels: hardware block b runs on XCD b % 8; logical block = a contiguous eighth of the grid per XCD,
// so that output rows that share source rows (the +1 taps) meet in one L2 instead of fetching them into several.
__device__ __forceinline__ int bev_block(int nb, int bid) {
  const int q = nb >> 3, r = nb & 7, x = bid & 7;
  return x * q + (x < r ? x : r) + (bid >> 3);
}
__device__ __forceinline__ int bev_block() { return bev_block((int)gridDim.x, (int)blockIdx.x); }

int sgrid(int64_t n, int cap = 4096) {
  int64_t g = wsmg_cdiv(n, 256);
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

// ----------------------------------------------------------------------------- a sample in the global map
struct Pose { float gx, gy; };  // integer-valued grid cell of the agent (to_grid.get_grid_coords)
__device__ __forceinline__ Pose grid_cell(const float* gps, int b, int G, float cmax, float cmin, float gsz) {
  Pose p;
  p.gx = rintf((cmax - gps[b * 2 + 0]) / gsz);
  p.gy = rintf((gps[b * 2 + 1] - cmin) / gsz);
  return p;
}

struct MapArgs {
  int C, E, G, lo;
  float cmax, cmin, gsz, halfG;
};

// where the paste of a sample lands: the translation of the fuse and the origin of its (E+4)^2 window in the global map
struct FuseGeo { float tx, ty; int wy0, wx0; };
__device__ __forceinline__ FuseGeo fuse_geo(Pose ps, const MapArgs& a) {
  FuseGeo f;
  f.tx = -(ps.gy - a.halfG) / a.halfG;
  f.ty = -(ps.gx - a.halfG) / a.halfG;
  f.wy0 = a.lo + (int)(ps.gx - a.halfG) - 2;
  f.wx0 = a.lo + (int)(ps.gy - a.halfG) - 2;
  return f;
}
// global-map pixel (Y, X) inside the sample's window (one unsigned compare per axis: below the origin wraps)
__device__ __forceinline__ bool in_window(int Y, int X, const FuseGeo& f, int E) {
  const unsigned WN = (unsigned)(E + 4);
  return (unsigned)Y - (unsigned)f.wy0 < WN && (unsigned)X - (unsigned)f.wx0 < WN;
}
// episode reset of four channels: g *= m, untouched when m == 1
__device__ __forceinline__ void reset4(f32x4& g, float m) {
  if (m != 1.0f) {
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] *= m;
  }
}

// the translation that brings the global map back to the agent (the retrieval's crop)
struct CropGeo { float tx, ty; };
__device__ __forceinline__ CropGeo crop_geo(Pose ps, const MapArgs& a) {
  CropGeo g;
  g.tx = (ps.gy - a.halfG) / a.halfG;
  g.ty = (ps.gx - a.halfG) / a.halfG;
  return g;
}
// sample coordinate in the global map of crop pixel j along one axis, translated by t
__device__ __forceinline__ float crop_coord(int j, float t, const MapArgs& a) { return unnorm(base_coord(a.lo + j, a.G) + t, a.G); }
// the four global-map taps of crop pixel (cy, cx)
__device__ __forceinline__ Taps crop_taps(int cx, int cy, float tx, float ty, const MapArgs& a) {
  return make_taps(crop_coord(cx, tx, a), crop_coord(cy, ty, a));
}
// the same per axis (the tiled retrieval meets x and y separately)
struct Axis { int p0; float a, b; };  // floor(i), (floor(i) + 1) - i, i - floor(i): one axis of make_taps
__device__ __forceinline__ Axis crop_axis(int j, float t, const MapArgs& a) {
  const float i = crop_coord(j, t, a);
  const float f0 = floorf(i);
  Axis r;
  r.p0 = (int)f0;
  r.a = (f0 + 1.0f) - i;
  r.b = i - f0;
  return r;
}

}  // namespace
