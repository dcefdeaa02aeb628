// Operator 1, global-map half (rollout path, no backward): episode reset, paste + translate + max-fuse of the rotated ego map into
// the persistent global map, and its retrieval (translate back, crop, final rotation).  Replaces, from common/rgb_mapping.py of the
// reference: Mapping.project_feat_to_map :32-72 with RotateTensor.forward :239-250 and to_grid :100-139.  wsmg_bev.hip has the
// projection half (index, scatter-max, first rotation); wsmg_bev_geom.h the sampling arithmetic both share.
//
// Everything here is NHWC (channel-contiguous, like the global map [P][G][G][C]) except the ROTATED NCHW PLANES the one-launch
// scatter + rotation hands to map_fuse_planes_kernel.  Each route is bit-identical to the launches it replaced: the same IEEE float32
// operations in the same order, with FMA contraction disabled for this file.
#include "wsmg_bev_geom.h"

#pragma clang fp contract(off)

namespace {

// full_global_map[:bs] *= masks (episode reset).  Untouched when mask == 1.
__global__ __launch_bounds__(256) void map_reset_kernel(float* gm, const float* masks, int64_t n4_per_env) {
  const int b = blockIdx.y;
  const float m = masks[b];
  if (m == 1.0f) return;
  f32x4* g = reinterpret_cast<f32x4*>(gm) + (size_t)b * n4_per_env;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4_per_env; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 v = g[i];
    reset4(v, m);
    g[i] = v;
  }
}

// the four taps of the translated paste at global-map pixel (Y, X): offset into an E x E plane (-1: zero padding of grid_sample or
// the zero border of the agent view around the paste) and weight, in k order
struct PasteTaps { int off[4]; float w[4]; };
__device__ __forceinline__ PasteTaps paste_taps(int X, int Y, bool pok, float tx, float ty, const MapArgs& a) {
  const int hi = a.lo + a.E;
  float gx = base_coord(pok ? X : 0, a.G) + tx;
  float gy = base_coord(Y, a.G) + ty;
  Taps tp = make_taps(unnorm(gx, a.G), unnorm(gy, a.G));
  PasteTaps r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = tp.y0 + (k >> 1), xx = tp.x0 + (k & 1);
    r.w[k] = tap_w(tp, k);
    const bool ok = pok && yy >= a.lo && yy < hi && xx >= a.lo && xx < hi && yy < a.G && xx < a.G;
    r.off[k] = ok ? (yy - a.lo) * a.E + (xx - a.lo) : -1;
  }
  return r;
}

// paste (centre) + translate (bilinear) + max-fuse, restricted to the (E+4)^2 window the pasted
// map can reach; outside it the translated view is exactly 0 and the map (>= 0) is unchanged.
// The ego map is NHWC here: a tap's plane offset is its pixel, and an item takes four channels of it.
__global__ __launch_bounds__(256) void map_fuse_kernel(const float* __restrict__ ego, float* __restrict__ gm,
                                                       const float* __restrict__ gps, MapArgs a) {
  const int b = blockIdx.y;
  const int WN = a.E + 4;
  const FuseGeo fg = fuse_geo(grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz), a);
  const int C4 = a.C >> 2;
  const f32x4* eb = reinterpret_cast<const f32x4*>(ego + (size_t)b * a.E * a.E * a.C);
  f32x4* gb = reinterpret_cast<f32x4*>(gm + (size_t)b * a.G * a.G * a.C);
  for (int64_t i = (int64_t)bev_block() * blockDim.x + threadIdx.x; i < (int64_t)WN * WN * C4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C4);
    int p = (int)(i / C4);
    int wy = p / WN, wx = p - wy * WN;
    int Y = fg.wy0 + wy, X = fg.wx0 + wx;
    if (Y < 0 || Y >= a.G || X < 0 || X >= a.G) continue;
    const PasteTaps pt = paste_taps(X, Y, true, fg.tx, fg.ty, a);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pt.off[k] >= 0) acc4(v, eb[(size_t)pt.off[k] * C4 + c], pt.w[k]);
    size_t o = ((size_t)Y * a.G + X) * C4 + c;
    f32x4 g = gb[o];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = v[j] > g[j] ? v[j] : g[j];
    gb[o] = g;
  }
}

// map_fuse_kernel for an ego map that arrives as ROTATED NCHW PLANES (bev_scatter_rotate_kernel).  A workgroup owns FP
// consecutive window pixels of one window row and all channels, in two phases:
//   1. work item = (channel, pixel) with the PIXEL fastest: the four taps are 4-byte loads that run along a plane row (coalesced,
//      independent — several items in flight per thread), the translated value goes to LDS as t[pixel][channel];
//   2. work item = (pixel, 4 channels) with the channel quad fastest, as in map_fuse_kernel: the value comes back from LDS as one
//      16-byte read and the global map is read-modify-written in 16-byte pieces of consecutive addresses.
// Same arithmetic per element (taps in k order).  (First form of this kernel: the (FR + 2) x (FC + 4) patch of every plane in LDS,
// then gathers out of it — 65 KB per workgroup, two workgroups per CU, load and compute phases that could not overlap: 334 us at
// cfg4 against 144 us of map_fuse_kernel.)
constexpr int FP = 64;
// RESET: the episode reset of the window's pixels rides in the read-modify-write (g * m before the max, as map_reset_kernel then
// this kernel leave it) — map_fuse_retrieve_kernel, where no reset launch runs in front
template <bool RESET>
__device__ __forceinline__ void fuse_planes_block(const float* __restrict__ ego, float* __restrict__ gm, const float* __restrict__ gps,
                                                  const MapArgs& a, int tiles_x, int blk, int b, float m) {
  extern __shared__ float tl[];           // [FP][C + 1]... pitch C + 4 keeps the 16-byte reads aligned
  const int wy = blk / tiles_x, tx_ = blk - wy * tiles_x;
  const int WN = a.E + 4;
  Pose ps = grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz);
  const FuseGeo fg = fuse_geo(ps, a);
  const float tx = fg.tx, ty = fg.ty;
  const int wy0 = fg.wy0, wx0 = fg.wx0;
  const int C4 = a.C >> 2;
  const int E2 = a.E * a.E;
  const int pitch = a.C + 4;
  const int Y = wy0 + wy;
  if (Y < 0 || Y >= a.G) return;          // (whole workgroup: the row is outside the global map)
  const float* eb = ego + (size_t)b * a.C * E2;
  // ---- phase 1
  {
    const int p = threadIdx.x & (FP - 1), cq = threadIdx.x >> 6;     // pixel of the tile, channel phase (256 / FP = 4)
    const int wx = tx_ * FP + p, X = wx0 + wx;
    const bool pok = wx < WN && X >= 0 && X < a.G;
    const PasteTaps pt = paste_taps(X, Y, pok, tx, ty, a);
    const int* off = pt.off;
    const float* w = pt.w;
    constexpr int U = 4;
    for (int c0 = cq; c0 < a.C; c0 += 4 * U) {
      float q[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + 4 * u;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[u][k] = (c < a.C && off[k] >= 0) ? eb[(size_t)c * E2 + off[k]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + 4 * u;
        if (c >= a.C) break;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (off[k] >= 0) v += q[u][k] * w[k];
        tl[p * pitch + c] = v;
      }
    }
  }
  __syncthreads();
  // ---- phase 2
  f32x4* gb = reinterpret_cast<f32x4*>(gm + (size_t)b * a.G * a.G * a.C);
  constexpr int V = 4;
  const int nitems = FP * C4;
  for (int i0 = threadIdx.x; i0 < nitems; i0 += 256 * V) {
    bool ok[V];
    size_t o[V];
    f32x4 g[V];
    int li[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      const int i = i0 + 256 * u;
      const int c = i % C4, p = i / C4;
      const int wx = tx_ * FP + p, X = wx0 + wx;
      ok[u] = i < nitems && wx < WN && X >= 0 && X < a.G;
      o[u] = ((size_t)Y * a.G + X) * C4 + c;
      li[u] = p * pitch + 4 * c;
      if (ok[u]) g[u] = gb[o[u]];
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if (!ok[u]) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(tl + li[u]);
      f32x4 gg = g[u];
      if (RESET) reset4(gg, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) gg[j] = v[j] > gg[j] ? v[j] : gg[j];
      gb[o[u]] = gg;
    }
  }
}
__global__ __launch_bounds__(256) void map_fuse_planes_kernel(const float* __restrict__ ego, float* __restrict__ gm,
                                                              const float* __restrict__ gps, MapArgs a, int tiles_x) {
  fuse_planes_block<false>(ego, gm, gps, a, tiles_x, (int)blockIdx.x, (int)blockIdx.y, 1.0f);
}

// translate the global map back to the agent and crop the centre E x E (NHWC scratch)
__global__ __launch_bounds__(256) void map_crop_kernel(const float* __restrict__ gm, const float* __restrict__ gps,
                                                       MapArgs a, float* __restrict__ crop) {
  const int b = blockIdx.y;
  const CropGeo cg = crop_geo(grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz), a);
  const int C4 = a.C >> 2;
  const f32x4* gb = reinterpret_cast<const f32x4*>(gm + (size_t)b * a.G * a.G * a.C);
  f32x4* cb = reinterpret_cast<f32x4*>(crop + (size_t)b * a.E * a.E * a.C);
  for (int64_t i = (int64_t)bev_block() * blockDim.x + threadIdx.x; i < (int64_t)a.E * a.E * C4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C4);
    int p = (int)(i / C4);
    int y = p / a.E, x = p - y * a.E;
    const Taps tp = crop_taps(x, y, cg.tx, cg.ty, a);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int yy = tp.y0 + (k >> 1), xx = tp.x0 + (k & 1);
      if (yy >= 0 && yy < a.G && xx >= 0 && xx < a.G) acc4(v, gb[((size_t)yy * a.G + xx) * C4 + c], tap_w(tp, k));
    }
    cb[i] = v;
  }
}

// final rotation: NHWC in, NHWC out (thread = (pixel, 4 channels): the tap geometry is computed once per
// 16 bytes instead of once per float, and every access is a 16-byte one; per-element arithmetic order unchanged)
__global__ __launch_bounds__(256) void rotate_nhwc_kernel(const float* __restrict__ in, const float* __restrict__ heading,
                                                          float sign, int C, int E, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int E2 = E * E, C4 = C >> 2;
  float t = sign * heading[b];
  Rot r{cosf(t), sinf(t)};
  const f32x4* ib = reinterpret_cast<const f32x4*>(in + (size_t)b * E2 * C);
  f32x4* ob = reinterpret_cast<f32x4*>(out + (size_t)b * E2 * C);
  for (int64_t i = (int64_t)bev_block() * blockDim.x + threadIdx.x; i < (int64_t)E2 * C4;
       i += (int64_t)gridDim.x * blockDim.x) {
    int c = (int)(i % C4);
    int p = (int)(i / C4);
    int y = p / E, x = p - y * E;
    Taps tp = rot_taps(x, y, E, r);
    bool x0ok, x1ok, y0ok, y1ok;
    taps_in(tp, E, x0ok, x1ok, y0ok, y1ok);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (y0ok && x0ok) acc4(v, ib[((size_t)tp.y0 * E + tp.x0) * C4 + c], tp.w00);
    if (y0ok && x1ok) acc4(v, ib[((size_t)tp.y0 * E + tp.x0 + 1) * C4 + c], tp.w01);
    if (y1ok && x0ok) acc4(v, ib[((size_t)(tp.y0 + 1) * E + tp.x0) * C4 + c], tp.w10);
    if (y1ok && x1ok) acc4(v, ib[((size_t)(tp.y0 + 1) * E + tp.x0 + 1) * C4 + c], tp.w11);
    ob[i] = v;
  }
}

// map_crop_kernel + rotate_nhwc_kernel in one pass (round 3): a rotation tap needs the cropped map at an integer pixel, which is
// itself four taps of the global map — the item (output pixel, 4 channels) computes its four crop values in registers (16 loads of
// 16 bytes, all independent, neighbours' loads hitting the same lines in L1 / L2) instead of the crop going to memory (205 MB out,
// 205 MB back at cfg4) between two launches.  Same arithmetic per value as the two kernels: crop = sum over k of q_k w_k, output =
// sum over the rotation taps (nw, ne, sw, se) of crop w.
__device__ __forceinline__ f32x4 retrieve_item_regs(const f32x4* __restrict__ gb, const MapArgs& a, float tx, float ty, Rot r,
                                                    int x, int y, int c) {
  const int C4 = a.C >> 2, E = a.E;
  const Taps rt = rot_taps(x, y, E, r);
  f32x4 q[4][4];
  float w[4][4];
  bool rok[4], cok[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {          // rotation tap k = crop pixel (cy, cx)
    const int cy = rt.y0 + (k >> 1), cx = rt.x0 + (k & 1);
    rok[k] = cy >= 0 && cy < E && cx >= 0 && cx < E;
    const Taps tp = crop_taps(rok[k] ? cx : 0, rok[k] ? cy : 0, tx, ty, a);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int yy = tp.y0 + (m >> 1), xx = tp.x0 + (m & 1);
      w[k][m] = tap_w(tp, m);
      cok[k][m] = rok[k] && yy >= 0 && yy < a.G && xx >= 0 && xx < a.G;
      if (cok[k][m]) q[k][m] = gb[((size_t)yy * a.G + xx) * C4 + c];
    }
  }
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!rok[k]) continue;
    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; ++m)
      if (cok[k][m]) acc4(cv, q[k][m], w[k][m]);
    acc4(v, cv, tap_w(rt, k));
  }
  return v;
}

// One f32x4 of the global map as this step's fuse leaves it, from the value `g` read before or after the fuse stored it (see
// map_fuse_retrieve_kernel): reset, then max with the translated paste inside the sample's window — the expressions of
// map_reset_kernel and map_fuse_planes_kernel.  The rare route's form: 16 plane loads per call.  A tile takes that route only when a
// gps coordinate is not finite (a finite pose's box always fits RBOX): an infinite one puts every tap outside the map and this is not
// called; a NaN one lands the taps on rows / columns 0 and 1 with NaN weights, so this runs (inside the window when G - E < 8) but the
// ego map is NaN whatever it returns.  Its values are therefore not observable through the ego map; the test
// (test_fuse_retrieve_rare_route_with_a_non_finite_gps) holds the route to the two launches' NaN pattern, zeros and global map.
__device__ __noinline__ f32x4 fuse_quad(f32x4 g, const float* __restrict__ eb, const MapArgs& a, const FuseGeo& fg, float m, int Y, int X,
                                        int c) {
  reset4(g, m);
  if (!in_window(Y, X, fg, a.E)) return g;
  const PasteTaps pt = paste_taps(X, Y, true, fg.tx, fg.ty, a);
  const int E2 = a.E * a.E;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (pt.off[k] >= 0) v += eb[(size_t)(4 * c + j) * E2 + pt.off[k]] * pt.w[k];
    g[j] = v > g[j] ? v : g[j];
  }
  return g;
}

// the same value, one rotation tap at a time (4 loads in flight instead of 16: the tiled kernel's rare route, few registers)
// MAPV: what a loaded global-map value stands for — itself (AsStored: no state, no argument registers) or this step's fuse of it
struct AsStored {
  __device__ __forceinline__ f32x4 operator()(f32x4 q, const MapArgs&, int, int, int) const { return q; }
};
struct AsFused {
  const float* eb;      // the sample's rotated planes
  FuseGeo fg;
  float m;
  __device__ __forceinline__ f32x4 operator()(f32x4 q, const MapArgs& a, int Y, int X, int c) const { return fuse_quad(q, eb, a, fg, m, Y, X, c); }
};
template <class MAPV>
__device__ __noinline__ f32x4 retrieve_item_seq(const f32x4* __restrict__ gb, const MapArgs& a, float tx, float ty, Rot r, int x, int y,
                                                int c, MAPV mapv) {
  const int C4 = a.C >> 2, E = a.E;
  const Taps rt = rot_taps(x, y, E, r);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int cy = rt.y0 + (k >> 1), cx = rt.x0 + (k & 1);
    if (!(cy >= 0 && cy < E && cx >= 0 && cx < E)) continue;
    const Taps tp = crop_taps(cx, cy, tx, ty, a);
    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int yy = tp.y0 + (m >> 1), xx = tp.x0 + (m & 1);
      if (yy >= 0 && yy < a.G && xx >= 0 && xx < a.G) acc4(cv, mapv(gb[((size_t)yy * a.G + xx) * C4 + c], a, yy, xx, c), tap_w(tp, m));
    }
    acc4(v, cv, tap_w(rt, k));
  }
  return v;
}

__global__ __launch_bounds__(256) void map_retrieve_fused_kernel(const float* __restrict__ gm, const float* __restrict__ gps,
                                                                 const float* __restrict__ heading, MapArgs a,
                                                                 float* __restrict__ out) {
  const int b = blockIdx.y;
  const CropGeo cg = crop_geo(grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz), a);
  const int C4 = a.C >> 2, E = a.E;
  const float t = heading[b];
  const Rot r{cosf(t), sinf(t)};
  const f32x4* gb = reinterpret_cast<const f32x4*>(gm + (size_t)b * a.G * a.G * a.C);
  f32x4* ob = reinterpret_cast<f32x4*>(out + (size_t)b * E * E * a.C);
  for (int64_t i = (int64_t)bev_block() * blockDim.x + threadIdx.x; i < (int64_t)E * E * C4; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const int p = (int)(i / C4);
    const int y = p / E, x = p - y * E;
    ob[i] = retrieve_item_regs(gb, a, cg.tx, cg.ty, r, x, y, c);
  }
}

// map_crop_kernel + rotate_nhwc_kernel in one pass through LDS (round 5).  The register form above pays 16 gathers of 16 bytes per
// item through the texture path (cfg4: 311 us against 219 for the two launches, which is why it only ran at small batches); here a
// workgroup owns an 8 x 8 tile of output pixels (and a slice of <= 40 channels), works out which global-map pixels the crop pixels
// under its rotation taps touch (<= 14 x 14: 7 sqrt 2 + 2 crop pixels, one more for their own taps, one for a floor that slips),
// stages that box once — rows of the box, pixels outside the map as zeros — and takes all 16 taps of an item from LDS.  The
// tap geometry is computed once per (pixel, rotation tap) — 256 records, one per thread: box offset, four crop weights, rotation
// weight — instead of once per (pixel, 4 channels) item (base_coord's IEEE divisions were the VALU time of the gather kernels),
// from the same expressions, and each value keeps the two kernels' summation order: bit-identical.  Where the two kernels SKIP a
// tap (outside the map, outside the crop) the record points at zeros with zero weights: an accumulator that starts at +0 is never
// -0, so adding +-0 leaves it unchanged.  A tile whose geometry does not fit the box (cannot happen for finite inputs: the spans
// above are bounds; an infinite gps does it) runs the register form instead.
// Latency: a tile is little work behind a chain of dependent steps (pose -> taps -> box extents -> box -> taps from LDS), and LDS
// holds few tiles per CU, so the chain is kept short: every thread derives its record from the pose alone (no tables, no LDS
// round trips), the extents meet through one wave reduction (DPP) and 16 words of LDS — LDS atomics from 64 lanes on one word
// took 20 000 of a workgroup's 32 000 cycles — and the box's loads are all in flight before the first LDS store.
// Where a workgroup's cycles go at cfg4 (since it started; profiles/r05_map_retrieve.txt): records 3 850, extents met 4 100, box
// issued 8 300, box in LDS 8 450, end 12 300.
constexpr int RT = 8, RBOX = 14, RBIG = 0x10000000;
// min / max over the lane's row of 16 (DPP: no LDS crossbar), in every lane of the row
template <bool MAX>
__device__ __forceinline__ int row_ext(int v) {
#define WSMG_EXT_STEP(ctrl)                                                      \
  {                                                                              \
    const int o = __builtin_amdgcn_update_dpp(v, v, ctrl, 0xf, 0xf, false);      \
    v = MAX ? (o > v ? o : v) : (o < v ? o : v);                                 \
  }
  WSMG_EXT_STEP(0xB1)    // quad_perm [1, 0, 3, 2]
  WSMG_EXT_STEP(0x4E)    // quad_perm [2, 3, 0, 1]
  WSMG_EXT_STEP(0x141)   // row_half_mirror
  WSMG_EXT_STEP(0x140)   // row_mirror
#undef WSMG_EXT_STEP
  return v;
}
// lane K of the caller's quad, in every lane of the quad
template <int K>
__device__ __forceinline__ int quad_get(int v) { return __builtin_amdgcn_update_dpp(v, v, K * 0x55, 0xf, 0xf, false); }
template <int K>
__device__ __forceinline__ float quad_getf(float v) { return __int_as_float(quad_get<K>(__float_as_int(v))); }

// FUSE (map_fuse_retrieve_kernel): the box holds the map AS THIS STEP'S FUSE LEAVES IT — every staged value is reset (g * m) on
// its way into LDS, and box pixel p < 196 then belongs to thread p, which max-fuses the translated paste of its pixel into the
// slice's channels in place (the taps once per pixel; per channel four 4-byte plane loads that run along a plane row across the
// lanes of a box row) when the pixel lies inside the sample's window.  gm is only read.  `blk`: the tile-and-slice number.
template <bool FUSE>
__device__ __forceinline__ void retrieve_tile(const float* __restrict__ gm, const float* __restrict__ gps,
                                              const float* __restrict__ heading, const MapArgs& a, int tiles_x, int nsplit, int S4,
                                              unsigned magicS4, float* __restrict__ out, int blk, int b,
                                              const float* __restrict__ ego, float m) {
  extern __shared__ float boxf[];  // [bh][bw][4 S4] floats: the box; then bw + 2 pixels of zeros
  __shared__ int s_ext[16][4];
  const int tid = threadIdx.x;
  const int tile = blk / nsplit, cs0 = (blk - tile * nsplit) * S4;   // first f32x4 of this workgroup's channel slice
  const int tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
  Pose ps = grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz);
  const CropGeo cg = crop_geo(ps, a);
  const float tx = cg.tx, ty = cg.ty;
  const int C4 = a.C >> 2, E = a.E, G = a.G;
  const FuseGeo fg = FUSE ? fuse_geo(ps, a) : FuseGeo{0.f, 0.f, 0, 0};
  const float* eb = FUSE ? ego + (size_t)b * a.C * E * E : nullptr;
  const f32x4* gb = reinterpret_cast<const f32x4*>(gm + (size_t)b * G * G * a.C);
  f32x4* ob = reinterpret_cast<f32x4*>(out + (size_t)b * E * E * a.C);
  f32x4* box = reinterpret_cast<f32x4*>(boxf);
  const float th = heading[b];
  const Rot r{cosf(th), sinf(th)};

  // ---- this thread's record: pixel tid / 4 of the tile, rotation tap tid % 4 = crop pixel (cy, cx)
  const int pl_r = tid >> 2, k_r = tid & 3;
  const int ry = tyi * RT + (pl_r >> 3), rx = txi * RT + (pl_r & 7);
  const bool live = ry < E && rx < E;
  const Taps rt = rot_taps(live ? rx : 0, live ? ry : 0, E, r);
  const int cy = rt.y0 + (k_r >> 1), cx = rt.x0 + (k_r & 1);
  const bool rok = live && cy >= 0 && cy < E && cx >= 0 && cx < E;
  const Axis ax = crop_axis(rok ? cx : 0, tx, a), ay = crop_axis(rok ? cy : 0, ty, a);
  // a coordinate that is not finite and small (an infinite / NaN gps): the floors saturate and the weights are NaN while the two
  // kernels skip the taps — not this route's case
  const bool sane = fabsf(ax.a) <= 2.0f && fabsf(ax.b) <= 2.0f && fabsf(ay.a) <= 2.0f && fabsf(ay.b) <= 2.0f && ax.p0 > -RBIG &&
                    ax.p0 < RBIG && ay.p0 > -RBIG && ay.p0 < RBIG;
  const bool use = rok && sane;
  {  // (a record that is not sane stretches the box beyond RBOX: the tile takes the register form)
    const int xlo = row_ext<false>(use ? ax.p0 : (rok ? -2 * RBIG : RBIG)), xhi = row_ext<true>(use ? ax.p0 + 1 : -RBIG);
    const int ylo = row_ext<false>(use ? ay.p0 : RBIG), yhi = row_ext<true>(use ? ay.p0 + 1 : -RBIG);
    if ((tid & 15) == 0) {
      int* e = s_ext[tid >> 4];
      e[0] = xlo; e[1] = xhi; e[2] = ylo; e[3] = yhi;
    }
  }
  __syncthreads();
  int gx_lo = RBIG, gx_hi = -RBIG, gy_lo = RBIG, gy_hi = -RBIG;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    gx_lo = s_ext[w][0] < gx_lo ? s_ext[w][0] : gx_lo; gx_hi = s_ext[w][1] > gx_hi ? s_ext[w][1] : gx_hi;
    gy_lo = s_ext[w][2] < gy_lo ? s_ext[w][2] : gy_lo; gy_hi = s_ext[w][3] > gy_hi ? s_ext[w][3] : gy_hi;
  }
  int bw = 2, bh = 0;                         // no tap of the tile lands in the crop: zeros only
  bool slow = false;                          // uniform
  if (gx_lo != RBIG) {
    slow = gx_lo < -RBIG || gx_hi - gx_lo + 1 > RBOX || gy_hi - gy_lo + 1 > RBOX;
    bw = gx_hi - gx_lo + 1; bh = gy_hi - gy_lo + 1;
  } else {
    gx_lo = gy_lo = 0;
  }
  if (slow) {  // the register form for this tile
    for (int i = tid; i < RT * RT * S4; i += 256) {
      const int pl = (int)__umulhi((unsigned)i, magicS4), c = cs0 + i - pl * S4;
      const int qy = tyi * RT + (pl >> 3), qx = txi * RT + (pl & 7);
      if (qy < E && qx < E) {
        if constexpr (FUSE) ob[((size_t)qy * E + qx) * C4 + c] = retrieve_item_seq(gb, a, tx, ty, r, qx, qy, c, AsFused{eb, fg, m});
        else ob[((size_t)qy * E + qx) * C4 + c] = retrieve_item_seq(gb, a, tx, ty, r, qx, qy, c, AsStored{});
      }
    }
    return;
  }
  // the record stays in registers: the four records of a pixel sit in one quad
  int off = bh * bw;
  f32x4 w = {0.f, 0.f, 0.f, 0.f};
  float wr = 0.f;
  if (use) {
    off = (ay.p0 - gy_lo) * bw + (ax.p0 - gx_lo);
    w[0] = ax.a * ay.a; w[1] = ax.b * ay.a; w[2] = ax.a * ay.b; w[3] = ax.b * ay.b;
    wr = tap_w(rt, k_r);
  }
  // ---- stage the box: rows of the box (this slice's channels of each pixel), out-of-map pixels and the tail as zeros; a batch's
  // loads all before its LDS stores (one load, one store per trip paid the memory latency per trip), branch-free
  {
    const unsigned rowq = (unsigned)(bw * S4), mrow = 0xFFFFFFFFu / rowq + 1u;
    const unsigned nbox = (unsigned)bh * rowq, nq = nbox + (unsigned)(bw + 2) * S4;
    constexpr int UB = 9;   // (14 x 14 + 16) pixels x 10 / 256 = 8.3: one batch
    for (unsigned i0 = tid; i0 < nq; i0 += 256 * UB) {
      f32x4 q[UB];
      bool ok[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const unsigned i = i0 + 256 * u;
        const unsigned row = __umulhi(i, mrow), rem = i - row * rowq;
        const unsigned px = __umulhi(rem, magicS4), c = rem - px * S4;
        const int yy = gy_lo + (int)row, xx = gx_lo + (int)px;
        ok[u] = i < nbox && yy >= 0 && yy < G && xx >= 0 && xx < G;
        q[u] = gb[ok[u] ? ((size_t)yy * G + xx) * C4 + cs0 + c : (size_t)0];
      }
      if constexpr (FUSE) {
#pragma unroll
        for (int u = 0; u < UB; ++u) reset4(q[u], m);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (i0 + 256 * u < nq) box[i0 + 256 * u] = ok[u] ? q[u] : z;
      }
    }
  }
  __syncthreads();
  if constexpr (FUSE) {
    if (tid < bh * bw) {
      const int row = tid / bw, px = tid - row * bw;
      const int Y = gy_lo + row, X = gx_lo + px;
      // a pixel outside the window is not the fuse's: its map value stays (a paste value of 0 there would still beat a negative one)
      const bool inw = Y >= 0 && Y < G && X >= 0 && X < G && in_window(Y, X, fg, E);
      if (inw) {
        const PasteTaps pt = paste_taps(X, Y, true, fg.tx, fg.ty, a);
        const float* ep = eb + (size_t)(4 * cs0) * (E * E);
        f32x4* const bp = box + tid * S4;
#pragma unroll 2
        for (int c = 0; c < S4; ++c) {
          float pq[4][4];
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) pq[j][k] = pt.off[k] >= 0 ? ep[(size_t)(4 * c + j) * (E * E) + pt.off[k]] : 0.f;
          f32x4 g = bp[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (pt.off[k] >= 0) v += pq[j][k] * pt.w[k];
            g[j] = v > g[j] ? v : g[j];
          }
          bp[c] = g;
        }
      }
    }
    __syncthreads();
  }
  // ---- thread = (its record's pixel, channel groups tid % 4, + 4, ...): the pixel's four records come from the quad (DPP, as
  // they are used: held for the whole loop they cost 24 registers and the kernel its fourth workgroup per CU)
  const int dn = bw * S4;
  const int offS = off * S4;
  for (int c = k_r; c < S4 + k_r; c += 4) {   // (uniform trip count: the quad broadcasts need the whole quad)
    const bool on = live && c < S4;
    const int cc = c < S4 ? c : 0;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#define WSMG_TAP(K)                                                                                                        \
    {                                                                                                                        \
      const f32x4* p = box + quad_get<K>(offS) + cc;                                                                         \
      const f32x4 q0 = p[0], q1 = p[S4], q2 = p[dn], q3 = p[dn + S4];                                                        \
      const float w0 = quad_getf<K>(w[0]), w1 = quad_getf<K>(w[1]), w2 = quad_getf<K>(w[2]), w3 = quad_getf<K>(w[3]);        \
      const float wk = quad_getf<K>(wr);                                                                                     \
      f32x4 cv = {0.f, 0.f, 0.f, 0.f};                                                                                       \
      acc4(cv, q0, w0); acc4(cv, q1, w1); acc4(cv, q2, w2); acc4(cv, q3, w3);                                                \
      acc4(v, cv, wk);                                                                                                       \
    }
    WSMG_TAP(0) WSMG_TAP(1) WSMG_TAP(2) WSMG_TAP(3)
#undef WSMG_TAP
    if (on) ob[((size_t)ry * E + rx) * C4 + cs0 + c] = v;
  }
}
__global__ __launch_bounds__(256, 4) void map_retrieve_tiled_kernel(const float* __restrict__ gm, const float* __restrict__ gps,
                                                                 const float* __restrict__ heading, MapArgs a, int tiles_x,
                                                                 int nsplit, int S4, unsigned magicS4, float* __restrict__ out) {
  retrieve_tile<false>(gm, gps, heading, a, tiles_x, nsplit, S4, magicS4, out, bev_block(), (int)blockIdx.y, nullptr, 1.0f);
}

// Episode reset of what the fuse window does not cover: global[b] *= m outside the sample's (E+4)^2 window (whose pixels the fuse
// workgroups reset as they read-modify-write them).  Nothing to do for m == 1.
constexpr int ZU = 4;
__device__ __forceinline__ void reset_rest_block(float* __restrict__ gm, const float* __restrict__ gps, const MapArgs& a, int blk, int nblk,
                                                 int b, float m) {
  if (m == 1.0f) return;
  const FuseGeo fg = fuse_geo(grid_cell(gps, b, a.G, a.cmax, a.cmin, a.gsz), a);
  const int C4 = a.C >> 2;
  const int64_t n4 = (int64_t)a.G * a.G * C4;
  f32x4* g = reinterpret_cast<f32x4*>(gm) + (size_t)b * n4;
  // ZU elements a stride apart per trip, their loads all before their stores: a quarter of the workgroups (which every sample
  // launches and a sample that is not reset only exits) keeps the loads in flight of four times as many
  const int64_t stride = (int64_t)nblk * 256;
  for (int64_t i0 = (int64_t)blk * 256 + threadIdx.x; i0 < n4; i0 += ZU * stride) {
    f32x4 v[ZU];
    bool own[ZU];
#pragma unroll
    for (int u = 0; u < ZU; ++u) {
      const int64_t i = i0 + u * stride;
      own[u] = false;
      if (i < n4) {
        const int p = (int)(i / C4), Y = p / a.G, X = p - Y * a.G;
        own[u] = !in_window(Y, X, fg, a.E);
      }
      if (own[u]) v[u] = g[i];
    }
#pragma unroll
    for (int u = 0; u < ZU; ++u) {
      if (!own[u]) continue;
      reset4(v[u], m);
      g[i0 + u * stride] = v[u];
    }
  }
}

// map_reset_kernel + map_fuse_planes_kernel + map_retrieve_tiled_kernel in ONE launch: three kinds of workgroup by blockIdx.x.
//   [0, nR)            retrieve_tile<true>: the retrieval.  They only READ the global map, and fuse what they read on the way into
//                      LDS, so that the values under the taps are this step's whatever the stores of the others have done yet.
//   [nR, nR + nF)      fuse_planes_block<true>: the fuse, with the reset of the window's pixels in its read-modify-write.
//   [nR + nF, ...)     reset_rest_block: the reset of the rest of the sample's map (only for a sample whose mask is not 1).
// OWNERSHIP.  Every element of the global map has ONE writer in this launch, and it is written at most once: an element inside
// the sample's window by the fuse workgroup of its window row and 64-pixel run, an element outside it by the reset workgroup whose
// grid-stride loop reaches it; retrieval workgroups never write the map.  No workgroup waits for another (no barrier across
// workgroups, no spin): the launch cannot hang on residency.
// THE HAZARD.  A retrieval workgroup may read an element before or after its owner's store.  Every read of the map is an aligned
// vector load whose dwords are each read once and whole, so each float it sees is either the value g before the step or the
// owner's result F(g) — and the reader applies F itself:  F(x) = max'(x * m, p), with x * m skipped when m == 1 (as
// map_reset_kernel skips it), p the translated paste (the same expressions and plane loads as the owner's, so the same bits) and
// max'(x, p) = p > x ? p : x; outside the window F(x) = x * m.  It needs F(F(g)) == F(g) bit for bit, which holds for masks in
// {0, 1} and a finite paste:
//   m == 1:  F(g) is g or p.  p > p is false and p > g was false where g stayed: F(F(g)) == F(g).  NaN: p > NaN and NaN > x are
//            false, so a NaN in the map stays and a NaN paste never enters — both times.
//   m == 0:  x * 0 is +0, -0 (x negative or -0) or NaN (x infinite / NaN).  F(g) is p (then p > +-0, so p > 0 is finite and
//            p * 0 == +0, p > +0: p again) or g * 0 (a zero keeps its sign under * 0, NaN stays NaN, and the comparison with p
//            comes out as before: +0 == -0 compare equal).  The -0 case: g = -3, m = 0, p = +0 gives -0 both times, never +0.
// A mask that is neither 0 nor 1 scales twice where a reader comes second, and an infinite paste turns to NaN under * 0: both are
// outside the contract (masks are the reference's not-done flags; features are finite).  tests: test_gpu_map_fuse_retrieve.py (signed
// zeros, negative features), test_map_fuse_retrieve_cpu.py (the same property on the oracle).
__global__ __launch_bounds__(256, 4) void map_fuse_retrieve_kernel(const float* __restrict__ ego, float* __restrict__ gm,
                                                                 const float* __restrict__ gps, const float* __restrict__ heading,
                                                                 const float* __restrict__ masks, MapArgs a, int tiles_x, int nsplit,
                                                                 int S4, unsigned magicS4, int nR, int ftiles_x, int nF, int nZ,
                                                                 float* __restrict__ out) {
  const int b = blockIdx.y, bid = blockIdx.x;
  const float m = masks[b];
  if (bid < nR) retrieve_tile<true>(gm, gps, heading, a, tiles_x, nsplit, S4, magicS4, out, bev_block(nR, bid), b, ego, m);
  else if (bid < nR + nF) fuse_planes_block<true>(ego, gm, gps, a, ftiles_x, bid - nR, b, m);
  else reset_rest_block(gm, gps, a, bid - nR - nF, nZ, b, m);
}

// what every global-map entry point asks of its shapes (grid.y = B; channel quads; a rotation needs E > 1)
bool map_shape_ok(int B, int C, int E, int G) { return !(B <= 0 || C <= 0 || C % 4 || E <= 1 || G < E || B > 65535); }

MapArgs map_args(int C, int E, int G, float resolution) {
  MapArgs a;
  a.C = C; a.E = E; a.G = G;
  a.lo = G / 2 - E / 2;  // G//2 - floor(E/2)
  double cmin = -(double)G * (double)resolution / 2, cmax = (double)G * (double)resolution / 2;
  a.cmax = (float)cmax;
  a.cmin = (float)cmin;
  a.gsz = (float)((cmax - cmin) / G);
  a.halfG = (float)(G / 2);
  return a;
}

// how the tiled retrieval cuts its work (wsmg_map_retrieve_tiled, wsmg_map_fuse_retrieve: the same slices, tiles and magic number,
// or the two would not give the same bits).  nsplit: the fewest channel slices that keep a slice at <= 40 channels and divide C / 4
// (a box of 14 x 14 + 16 pixels x 40 channels and the records are 40 KB: four workgroups per CU); 0: none does with a box that fits
// LDS.  S4: f32x4 per pixel and slice; tiles: 8 x 8 output tiles per axis.
struct RetrievePlan { int nsplit, S4, tiles; size_t lds; unsigned magic; };
RetrievePlan retrieve_plan(int C, int E) {
  RetrievePlan p{};
  const int C4 = C / 4;
  for (int n = 1; n <= C4 && !p.nsplit; ++n)
    if (C4 % n == 0 && C4 / n <= 10) p.nsplit = n;
  if (!p.nsplit) return p;
  p.S4 = C4 / p.nsplit;
  p.tiles = (E + RT - 1) / RT;
  p.lds = (size_t)(RBOX * RBOX + RBOX + 2) * p.S4 * 16;
  p.magic = 0xFFFFFFFFu / (unsigned)p.S4 + 1u;       // i / S4 as a multiply-high: exact while i * S4 < 2^32 (i < 16 * 14 * S4)
  return p;
}

}  // namespace

extern "C" int wsmg_map_fuse(const float* ego_rot, float* global_map, const float* gps, const float* masks, int B,
                             int C, int E, int G, float resolution, wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G)) return WSMG_EINVAL;
  MapArgs a = map_args(C, E, G, resolution);
  int64_t n4 = (int64_t)G * G * C / 4;
  hipLaunchKernelGGL(map_reset_kernel, dim3(sgrid(n4, 1024), B), dim3(256), 0, wsmg_s(stream), global_map, masks, n4);
  int64_t n = (int64_t)(E + 4) * (E + 4) * (C / 4);
  hipLaunchKernelGGL(map_fuse_kernel, dim3(sgrid(n), B), dim3(256), 0, wsmg_s(stream), ego_rot, global_map, gps, a);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_map_fuse_planes(const float* ego_rot_planes, float* global_map, const float* gps, const float* masks, int B,
                                    int C, int E, int G, float resolution, wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G) || C > 64) return WSMG_EINVAL;
  MapArgs a = map_args(C, E, G, resolution);
  int64_t n4 = (int64_t)G * G * C / 4;
  hipLaunchKernelGGL(map_reset_kernel, dim3(sgrid(n4, 1024), B), dim3(256), 0, wsmg_s(stream), global_map, masks, n4);
  const int tiles_x = wsmg_cdiv(E + 4, FP), tiles_y = E + 4;
  const size_t lds = (size_t)FP * (C + 4) * sizeof(float);
  hipLaunchKernelGGL(map_fuse_planes_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)B), dim3(256), lds, wsmg_s(stream),
                     ego_rot_planes, global_map, gps, a, tiles_x);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_map_retrieve(const float* global_map, const float* gps, const float* compass, int B, int C, int E,
                                 int G, float resolution, float* scratch, float* out, wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G)) return WSMG_EINVAL;
  MapArgs a = map_args(C, E, G, resolution);
  int64_t n = (int64_t)E * E * (C / 4);
  hipLaunchKernelGGL(map_crop_kernel, dim3(sgrid(n), B), dim3(256), 0, wsmg_s(stream), global_map, gps, a, scratch);
  hipLaunchKernelGGL(rotate_nhwc_kernel, dim3(sgrid(n), B), dim3(256), 0, wsmg_s(stream), scratch, compass, 1.0f, C, E,
                     out);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_map_retrieve_fused(const float* global_map, const float* gps, const float* compass, int B, int C, int E, int G,
                                       float resolution, float* out, wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G)) return WSMG_EINVAL;
  MapArgs a = map_args(C, E, G, resolution);
  int64_t n = (int64_t)E * E * (C / 4);
  hipLaunchKernelGGL(map_retrieve_fused_kernel, dim3(sgrid(n), B), dim3(256), 0, wsmg_s(stream), global_map, gps, compass, a, out);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_map_retrieve_tiled(const float* global_map, const float* gps, const float* compass, int B, int C, int E, int G,
                                       float resolution, float* out, wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G)) return WSMG_EINVAL;
  const RetrievePlan p = retrieve_plan(C, E);
  if (p.nsplit <= 0) return WSMG_EINVAL;
  if ((int64_t)p.tiles * p.tiles * p.nsplit > 0x7fffffff) return WSMG_EINVAL;
  MapArgs a = map_args(C, E, G, resolution);
  hipLaunchKernelGGL(map_retrieve_tiled_kernel, dim3((unsigned)(p.tiles * p.tiles * p.nsplit), (unsigned)B), dim3(256), p.lds,
                     wsmg_s(stream), global_map, gps, compass, a, p.tiles, p.nsplit, p.S4, p.magic, out);
  WSMG_RETURN_LAUNCH();
}

// wsmg_map_fuse_planes + wsmg_map_retrieve_tiled in one launch (map_fuse_retrieve_kernel has the ownership rule and why a read
// that races its owner's store is admissible); bit-identical to the two for masks in {0, 1} and finite features
extern "C" int wsmg_map_fuse_retrieve(const float* ego_rot_planes, float* global_map, const float* gps, const float* compass,
                                      const float* masks, int B, int C, int E, int G, float resolution, float* out,
                                      wsmg_stream_t stream) {
  if (!map_shape_ok(B, C, E, G) || C > 64 || (size_t)E * E * 4 > 160 * 1024) return WSMG_EINVAL;
  const RetrievePlan p = retrieve_plan(C, E);
  if (p.nsplit <= 0) return WSMG_EINVAL;
  const size_t lds_f = (size_t)FP * (C + 4) * sizeof(float);
  MapArgs a = map_args(C, E, G, resolution);
  const int nR = p.tiles * p.tiles * p.nsplit;                 // E <= 202: < 2^31
  const int ftiles_x = wsmg_cdiv(E + 4, FP), nF = ftiles_x * (E + 4);
  const int nZ = sgrid(wsmg_cdiv((int64_t)G * G * C / 4, ZU), 64);         // reset workgroups: ZU elements per thread and trip
  hipLaunchKernelGGL(map_fuse_retrieve_kernel, dim3((unsigned)(nR + nF + nZ), (unsigned)B), dim3(256), p.lds > lds_f ? p.lds : lds_f,
                     wsmg_s(stream), ego_rot_planes, global_map, gps, compass, masks, a, p.tiles, p.nsplit, p.S4, p.magic, nR, ftiles_x, nF,
                     nZ, out);
  WSMG_RETURN_LAUNCH();
}
