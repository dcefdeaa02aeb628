// Operator 1: RGB-D -> egocentric bird's-eye-view map (rollout path, no backward).
// Replaces, from common/rgb_mapping.py of the reference:
//   ComputeSpatialLocs.forward :153-176, ProjectToGroundPlane.forward :184-232 (incl. the
//   third-party torch_scatter.scatter_max CUDA kernel), RotateTensor.forward :239-250,
//   to_grid.get_grid_coords :100-103, get_grid :106-139 and Mapping.project_feat_to_map :32-72.
//
// Integer part is bit-exact with the reference's float32 arithmetic: every operation below is
// the same IEEE float32 operation in the same order, with FMA contraction disabled for this
// file.  Sources the reference funnels to cell 0 with -1e16 (invalid depth / height filter /
// out of range) are skipped instead, cells are initialised "empty" and emitted as 0 — the
// same result without the cell-0 hot spot.
//
// HBM layout: features NCHW in (as the frozen UNet produces them), one E x E channel plane per
// workgroup lives in LDS for the scatter; everything downstream of the first rotation is NHWC
// (channel-contiguous, like the persistent global map [P][G][G][C]) so that the bilinear
// gathers and the max-fuse read-modify-write are fully coalesced 256-B channel runs.
//
// This file: index, compacted index, the scatter family, the one-launch projection and the first rotation.  The global-map half
// (reset, fuse, crop, final rotation, retrieval) is wsmg_bev_map.hip; the sampling arithmetic both use is wsmg_bev_geom.h.
#include "wsmg_bev_geom.h"

#pragma clang fp contract(off)

namespace {

// ----------------------------------------------------------------------------- index
struct IndexArgs {
  const float* depth;
  int32_t* lin;
  int B, Hd, Wd, Hf, Wf, E;
  float depth_scale, local_scale, half, cx, cy, fx, fy, K;
};

// (grid.y = sample, 32-bit index arithmetic inside it: the flat 64-bit form spent three 64-bit divisions per element — most of its
//  12.6 us at cfg4 — on finding (b, hf, wf))
__global__ __launch_bounds__(256) void bev_index_kernel(IndexArgs a) {
  const unsigned per = (unsigned)(a.Hf * a.Wf);
  const int b = blockIdx.y;
  for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < per; p += gridDim.x * blockDim.x) {
    const unsigned hfu = p / (unsigned)a.Wf;
    const int hf = (int)hfu, wf = (int)(p - hfu * (unsigned)a.Wf);
    const size_t i = (size_t)b * per + p;
    // (arange * K).long(): int64 * python float -> float32 product, truncated
    int ih = (int)((float)hf * a.K);
    int iw = (int)((float)wf * a.K);
    float z = a.depth[((size_t)b * a.Hd + ih) * a.Wd + iw] * a.depth_scale;
    float xx = ((float)iw - a.cx) / a.fx;
    float yy = ((float)(a.Hd - ih) - a.cy) / a.fy;
    float X = xx * z;
    float Y = yy * z;
    bool valid = (z != 0.f) && (Y > -1.5f) && (Y < 0.1f);
    float xg = rintf(X / a.local_scale + a.half);
    float yg = rintf(-(z / a.local_scale) + a.half);
    float Ef = (float)a.E;
    bool inr = (yg < Ef) && (yg >= 0.f) && (xg < Ef) && (xg >= 0.f);
    a.lin[i] = (valid && inr) ? (int)yg * a.E + (int)xg : -1;
  }
}

// Round 6 — the index launch also COMPACTS the valid sources.  75-80 % of the sources of a frame are invalid (no depth, above the
// horizon, outside the map: SURVEY section 7), and every (sample, channel) plane workgroup of the scatter walked all Hf x Wf index
// entries to find the rest — 40 times per sample at cfg4, eight dependent trips of index -> feature -> LDS atomic each.  Here a
// workgroup owns a block of CB = 8192 consecutive sources, writes their index entries as before, and packs the valid ones —
// (source << 16) | cell, both < 65 536 — to the front of ITS block of `clist`, count in cnt[sample][block]: no global atomics,
// nothing to zero, any order inside a block (the scatter is a max: order-independent, bit-exact).  The scatter then walks
// sum(cnt) entries instead of Hf x Wf.
constexpr int CB = 8192;
__device__ __forceinline__ int index_of(const IndexArgs& a, int b, unsigned p) {
  const unsigned hfu = p / (unsigned)a.Wf;
  const int hf = (int)hfu, wf = (int)(p - hfu * (unsigned)a.Wf);
  int ih = (int)((float)hf * a.K);
  int iw = (int)((float)wf * a.K);
  float z = a.depth[((size_t)b * a.Hd + ih) * a.Wd + iw] * a.depth_scale;
  float xx = ((float)iw - a.cx) / a.fx;
  float yy = ((float)(a.Hd - ih) - a.cy) / a.fy;
  float X = xx * z;
  float Y = yy * z;
  bool valid = (z != 0.f) && (Y > -1.5f) && (Y < 0.1f);
  float xg = rintf(X / a.local_scale + a.half);
  float yg = rintf(-(z / a.local_scale) + a.half);
  float Ef = (float)a.E;
  bool inr = (yg < Ef) && (yg >= 0.f) && (xg < Ef) && (xg >= 0.f);
  return (valid && inr) ? (int)yg * a.E + (int)xg : -1;
}
// the index row of sample b, computed where it is read (bev_project_kernel: no index launch in front of the scatter)
struct DepthCells {
  IndexArgs a;
  int b;
  __device__ __forceinline__ int operator[](int s) const { return index_of(a, b, (unsigned)s); }
};
__global__ __launch_bounds__(1024) void bev_index_compact_kernel(IndexArgs a, unsigned* __restrict__ clist, int* __restrict__ cnt) {
  __shared__ int lcount;
  const unsigned per = (unsigned)(a.Hf * a.Wf);
  const int b = blockIdx.y, k = blockIdx.x;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) lcount = 0;
  __syncthreads();
  unsigned* const mine = clist + (size_t)b * per + (size_t)k * CB;
#pragma unroll 1
  for (int u = 0; u < CB / 1024; ++u) {
    const unsigned p = (unsigned)k * CB + threadIdx.x + 1024u * u;
    int v = -1;
    if (p < per) {
      v = index_of(a, b, p);
      a.lin[(size_t)b * per + p] = v;
    }
    const bool ok = v >= 0;
    const unsigned long long m = __ballot(ok);
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      int base = 0;
      if (lane == leader) base = atomicAdd(&lcount, __popcll(m));
      base = __shfl(base, leader, 64);
      if (ok) mine[base + __popcll(m & ((1ull << lane) - 1ull))] = (p << 16) | (unsigned)v;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) cnt[b * (int)gridDim.x + k] = lcount;
}

// ----------------------------------------------------------------------------- scatter-max
__device__ __forceinline__ unsigned f2key(float v) {
  unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
  unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  return __uint_as_float(u);
}

// Scatter-max of one (sample, map channel) into its LDS plane `tg` (keys; 0 = empty), by the 1024 threads of a workgroup.
// adaptive_max_pool1d window of output channel c over the Cf feature channels: [ws, we).
// Memory-level parallelism is the whole game here: the plane leaves room for ONE workgroup per CU at E = 200 (16 waves), and a
// trip is index -> feature -> atomic.  Round 2 went from one source per thread and trip (14 GB/s per CU: pure latency) to eight
// with their loads issued together (16 GB/s per CU x 256); round 3 also issues the (up to four) window channels of all eight
// sources together instead of one channel per dependent loop trip, and fetches the NEXT trip's indices before this trip's
// features are used, so that an index round trip is never exposed.
// WU: window channels fetched together (the launcher picks the widest window of the geometry, up to 4; at Cf == C it is 1, and
// the 40 VGPRs of that form keep two workgroups per CU at E = 100, which the 78 of WU = 4 do not).
// CELLS: lb[s] = cell of source s or -1 — the index launch's row (const int32_t*, passed __restrict__ as before) or DepthCells,
// which derives it from the depth.
template <class T> struct CellArg { using type = const T; };
template <class T> struct CellArg<T*> { using type = T* __restrict__; };
template <int WU, class CELLS>
__device__ __forceinline__ void scatter_plane(const float* __restrict__ feat, typename CellArg<CELLS>::type lb, int b, int c, int Cf,
                                              int HW, int C, unsigned* tg, int tid) {
  const int ws = (int)(((int64_t)c * Cf) / C);
  const int we = (int)((((int64_t)(c + 1)) * Cf + C - 1) / C);
  const float* fb = feat + ((size_t)b * Cf + ws) * HW;
  constexpr int U = 8;
  const int nwin = we - ws;
  if constexpr (WU == 1) {
    // Cf == C (the rollout geometry, one feature channel per map channel): the round-2 loop, which at B = 8 already runs at
    // 6.6 TB/s — the pipelined form below measured 30.6 instead of 23.8 us there (56 instead of 34 VGPRs)
    for (int s0 = tid; s0 < HW; s0 += 1024 * U) {
      int cell[U];
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int s = s0 + 1024 * u;
        cell[u] = s < HW ? lb[s] : -1;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = cell[u] >= 0 ? fb[s0 + 1024 * u] : 0.f;
      for (int w = 1; w < nwin; ++w) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (cell[u] >= 0) v[u] = fmaxf(v[u], fb[(size_t)w * HW + s0 + 1024 * u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (cell[u] >= 0) atomicMax(&tg[cell[u]], f2key(v[u]));
    }
    return;
  }
  int nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int s = tid + 1024 * u;
    nxt[u] = s < HW ? lb[s] : -1;
  }
  for (int s0 = tid; s0 < HW; s0 += 1024 * U) {
    int cell[U];
    float f[U][WU];
#pragma unroll
    for (int u = 0; u < U; ++u) cell[u] = nxt[u];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int w = 0; w < WU; ++w) f[u][w] = (cell[u] >= 0 && w < nwin) ? fb[(size_t)w * HW + s0 + 1024 * u] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + 1024 * (U + u);
      nxt[u] = s < HW ? lb[s] : -1;
    }
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = f[u][0];
#pragma unroll
      for (int w = 1; w < WU; ++w)
        if (w < nwin) v[u] = fmaxf(v[u], f[u][w]);
    }
    for (int w = WU; w < nwin; ++w) {       // wider windows (Cf > 4 C): the rest one channel per trip
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (cell[u] >= 0) v[u] = fmaxf(v[u], fb[(size_t)w * HW + s0 + 1024 * u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (cell[u] >= 0) atomicMax(&tg[cell[u]], f2key(v[u]));
  }
}

// The same scatter from the compacted source list of bev_index_compact_kernel: `nblk` blocks of CB entries, cnt[k] valid at the
// front of block k.  The flat entry index i in [0, sum cnt) is mapped to (block, offset) against the prefix sums in registers.
template <int WU>
__device__ __forceinline__ void scatter_plane_compact(const float* __restrict__ feat, const unsigned* __restrict__ cl, const int* __restrict__ cnt,
                                                      int nblk, int b, int c, int Cf, int HW, int C, unsigned* tg, int tid) {
  const int ws = (int)(((int64_t)c * Cf) / C);
  const int we = (int)((((int64_t)(c + 1)) * Cf + C - 1) / C);
  const float* fb = feat + ((size_t)b * Cf + ws) * HW;
  const int nwin = we - ws;
  // (the list is short — ~16 k entries per sample at cfg4, 16 per thread — and every entry is a dependent chain entry -> feature ->
  //  LDS atomic: eight of them in flight per thread — 16 spilled at WU = 2 and cost the E = 100 geometry its second workgroup per CU)
  constexpr int U = 8;
  int off[9];            // prefix sums of the (up to 8) block counts
  off[0] = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) off[k + 1] = off[k] + (k < nblk ? cnt[k] : 0);
  const int N = off[8];
  auto entry = [&](int i) -> unsigned {
    if (i >= N) return 0xffffffffu;
    int k = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) k += (i >= off[j]) ? 1 : 0;
    return cl[(size_t)k * CB + (i - off[k])];
  };
  unsigned nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) nxt[u] = entry(tid + 1024 * u);
  for (int i0 = tid; i0 < N; i0 += 1024 * U) {
    unsigned e[U];
    float f[U][WU];
#pragma unroll
    for (int u = 0; u < U; ++u) e[u] = nxt[u];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int w = 0; w < WU; ++w) f[u][w] = (e[u] != 0xffffffffu && w < nwin) ? fb[(size_t)w * HW + (e[u] >> 16)] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) nxt[u] = entry(i0 + 1024 * (U + u));
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = f[u][0];
#pragma unroll
      for (int w = 1; w < WU; ++w)
        if (w < nwin) v[u] = fmaxf(v[u], f[u][w]);
    }
    for (int w = WU; w < nwin; ++w) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (e[u] != 0xffffffffu) v[u] = fmaxf(v[u], fb[(size_t)w * HW + (e[u] >> 16)]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (e[u] != 0xffffffffu) atomicMax(&tg[e[u] & 0xffffu], f2key(v[u]));
  }
}

// one workgroup = (sample, CG consecutive map channels); the CG E*E planes live in LDS
template <int WU>
__global__ __launch_bounds__(1024) void bev_scatter_kernel(const float* __restrict__ feat,
                                                           const int32_t* __restrict__ lin, int Cf, int HW, int C,
                                                           int E2, int CG, float* __restrict__ out) {
  extern __shared__ unsigned tile[];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * CG;
  const int tid = threadIdx.x;
  for (int i = tid; i < CG * E2; i += 1024) tile[i] = 0u;  // 0 = empty (below every float key)
  __syncthreads();
  const int32_t* lb = lin + (size_t)b * HW;
  for (int g = 0; g < CG; ++g) {
    int c = c0 + g;
    if (c >= C) break;
    scatter_plane<WU, const int32_t*>(feat, lb, b, c, Cf, HW, C, tile + (size_t)g * E2, tid);
  }
  __syncthreads();
  for (int i = tid; i < CG * E2; i += 1024) {
    int g = i / E2;
    if (c0 + g >= C) break;
    unsigned k = tile[i];
    out[((size_t)b * C + c0) * E2 + i] = k ? key2f(k) + 0.0f : 0.0f;
  }
}

// scatter-max and the first rotation in ONE launch (round 3): the E x E plane of a channel is complete in LDS when the scatter
// ends, so the rotation samples it there (4 LDS reads per output pixel) and only the ROTATED plane goes to memory — NCHW, whole
// rows, coalesced — instead of plane out, plane in through 4-byte gathers, NHWC out.  map_fuse_planes_kernel consumes the planes.
// Same arithmetic per output pixel as rotate_nchw_to_nhwc_kernel (tap order nw, ne, sw, se).
// Round 5 — the rotation's arithmetic diet (cfg4: scatter alone 165 us, scatter + rotation 270-295: the rotation phase was VALU time,
// not LDS or HBM time — every (pixel, channel) item recomputed the tap geometry with four IEEE divisions (base_coord: 2 / (W - 1)
// and / W, twice) and an integer division p / E): the two base coordinates come from a table in the LDS left over beside the
// plane (E floats, the same function's values: bit-identical), y = p / E is a multiply-high by a host-computed magic number.
template <int WU, class CELLS>
__device__ __forceinline__ void scatter_rotate_block(const float* __restrict__ feat, typename CellArg<CELLS>::type lb,
                                                     const float* __restrict__ heading,
                                                     float sign, int Cf, int HW, int C, int E, int CG, unsigned magicE, int table,
                                                     float* __restrict__ out, const unsigned* __restrict__ clist,
                                                     const int* __restrict__ cnt, int nblk) {
  extern __shared__ unsigned tile[];
  const int b = blockIdx.y;
  const int c0 = blockIdx.x * CG;
  const int tid = threadIdx.x;
  const int E2 = E * E;
  float* const bc = reinterpret_cast<float*>(tile + (size_t)CG * E2);    // [E] base coordinates (only when `table`)
  for (int i = tid; i < CG * E2; i += 1024) tile[i] = 0u;
  if (table)
    for (int i = tid; i < E; i += 1024) bc[i] = base_coord(i, E);
  __syncthreads();
  for (int g = 0; g < CG; ++g) {
    int c = c0 + g;
    if (c >= C) break;
    if (clist) scatter_plane_compact<WU>(feat, clist + (size_t)b * HW, cnt + (size_t)b * nblk, nblk, b, c, Cf, HW, C, tile + (size_t)g * E2, tid);
    else scatter_plane<WU, CELLS>(feat, lb, b, c, Cf, HW, C, tile + (size_t)g * E2, tid);
  }
  __syncthreads();
  for (int i = tid; i < CG * E2; i += 1024) {   // keys -> the values bev_scatter_kernel writes, in place
    const unsigned k = tile[i];
    tile[i] = __float_as_uint(k ? key2f(k) + 0.0f : 0.0f);
  }
  __syncthreads();
  const float t = sign * heading[b];
  const Rot r{cosf(t), sinf(t)};
  for (int g = 0; g < CG; ++g) {
    const int c = c0 + g;
    if (c >= C) break;
    const float* pb = reinterpret_cast<const float*>(tile + (size_t)g * E2);
    float* ob = out + ((size_t)b * C + c) * E2;
    for (int p = tid; p < E2; p += 1024) {
      const int y = (int)__umulhi((unsigned)p, magicE), x = p - y * E;
      const float bx = table ? bc[x] : base_coord(x, E), by = table ? bc[y] : base_coord(y, E);
      const float gx = bx * r.c + by * r.s;
      const float gy = bx * (-r.s) + by * r.c;
      const Taps tp = make_taps(unnorm(gx, E), unnorm(gy, E));
      // branch-free (round 5, end): one unsigned compare per bound, every tap read from a clamped address, a tap outside the plane
      // dropped by a select AFTER its product (what the four branches did, without four exec-mask round trips per pixel)
      const bool x0ok = (unsigned)tp.x0 < (unsigned)E, x1ok = (unsigned)(tp.x0 + 1) < (unsigned)E;
      const bool y0ok = (unsigned)tp.y0 < (unsigned)E, y1ok = (unsigned)(tp.y0 + 1) < (unsigned)E;
      const int xa = x0ok ? tp.x0 : 0, xb = x1ok ? tp.x0 + 1 : 0;
      const int ya = y0ok ? tp.y0 * E : 0, yb = y1ok ? (tp.y0 + 1) * E : 0;
      const float q00 = pb[ya + xa], q01 = pb[ya + xb], q10 = pb[yb + xa], q11 = pb[yb + xb];
      float v = 0.f, t;
      t = v + q00 * tp.w00; v = (y0ok && x0ok) ? t : v;
      t = v + q01 * tp.w01; v = (y0ok && x1ok) ? t : v;
      t = v + q10 * tp.w10; v = (y1ok && x0ok) ? t : v;
      t = v + q11 * tp.w11; v = (y1ok && x1ok) ? t : v;
      ob[p] = v;
    }
  }
}
template <int WU>
__global__ __launch_bounds__(1024) void bev_scatter_rotate_kernel(const float* __restrict__ feat, const int32_t* __restrict__ lin,
                                                                  const float* __restrict__ heading, float sign, int Cf, int HW,
                                                                  int C, int E, int CG, unsigned magicE, int table,
                                                                  float* __restrict__ out, const unsigned* __restrict__ clist,
                                                                  const int* __restrict__ cnt, int nblk) {
  scatter_rotate_block<WU, const int32_t*>(feat, lin + (size_t)blockIdx.y * HW, heading, sign, Cf, HW, C, E, CG, magicE, table, out, clist, cnt, nblk);
}

// bev_index_kernel + bev_scatter_rotate_kernel in ONE launch, for the batches below 4 where the operator is launch latency and not
// bandwidth: a plane workgroup derives every source's cell from the depth image itself (index_of: the index kernel's expressions) —
// 256 KB per sample, re-read by the C / CG workgroups of the sample out of L2 — instead of waiting for an index launch.  The first
// workgroup of a sample also writes the index row when the caller wants it.  Same cells, same scatter, same rotation: same bits.
template <int WU>
__global__ __launch_bounds__(1024) void bev_project_kernel(const float* __restrict__ feat, IndexArgs ia, const float* __restrict__ heading,
                                                           float sign, int Cf, int C, int CG, unsigned magicE, int table,
                                                           float* __restrict__ out) {
  const int b = blockIdx.y, HW = ia.Hf * ia.Wf;
  if (ia.lin && blockIdx.x == 0)
    for (int s = threadIdx.x; s < HW; s += 1024) ia.lin[(size_t)b * HW + s] = index_of(ia, b, (unsigned)s);
  scatter_rotate_block<WU, DepthCells>(feat, DepthCells{ia, b}, heading, sign, Cf, HW, C, ia.E, CG, magicE, table, out, nullptr, nullptr, 0);
}

// first rotation: NCHW planes in (scatter output), NHWC out through an LDS transpose
__global__ __launch_bounds__(256) void rotate_nchw_to_nhwc_kernel(const float* __restrict__ in,
                                                                  const float* __restrict__ heading, float sign,
                                                                  int C, int E, float* __restrict__ out) {
  __shared__ float sh[64 * 65];
  // one workgroup = an 8 x 8 block of output pixels x all channels: the taps of a block fall into a ~12 x 12
  // source patch per channel plane (a 64 x 1 line would touch up to 64 source rows at 45 degrees)
  const int b = blockIdx.y;
  const int nbx = (E + 7) >> 3;
  const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
  const int tid = threadIdx.x;
  const int pl = tid & 63, cq = tid >> 6;
  const int E2 = E * E;
  float t = sign * heading[b];
  Rot r{cosf(t), sinf(t)};
  const int y = by * 8 + (pl >> 3), x = bx * 8 + (pl & 7);
  const bool pok = y < E && x < E;
  Taps tp = rot_taps(pok ? x : 0, pok ? y : 0, E, r);
  bool x0ok, x1ok, y0ok, y1ok;
  taps_in(tp, E, x0ok, x1ok, y0ok, y1ok);
#pragma unroll 4
  for (int c = cq; c < C; c += 4) {
    const float* pb = in + ((size_t)b * C + c) * E2;
    float v = 0.f;
    if (pok) {
      if (y0ok && x0ok) v += pb[tp.y0 * E + tp.x0] * tp.w00;
      if (y0ok && x1ok) v += pb[tp.y0 * E + tp.x0 + 1] * tp.w01;
      if (y1ok && x0ok) v += pb[(tp.y0 + 1) * E + tp.x0] * tp.w10;
      if (y1ok && x1ok) v += pb[(tp.y0 + 1) * E + tp.x0 + 1] * tp.w11;
    }
    sh[pl * 65 + c] = v;
  }
  __syncthreads();
  for (int i = tid; i < 64 * C; i += 256) {
    int q = i / C, c = i - q * C;
    const int qy = by * 8 + (q >> 3), qx = bx * 8 + (q & 7);
    if (qy < E && qx < E) out[((size_t)b * E2 + qy * E + qx) * C + c] = sh[q * 65 + c];
  }
}

// widest adaptive_max_pool1d window of Cf -> C channels, capped at 4 (scatter_plane's WU)
int scatter_window(int Cf, int C) {
  int m = 1;
  for (int c = 0; c < C; ++c) {
    const int ws = (int)(((int64_t)c * Cf) / C), we = (int)((((int64_t)(c + 1)) * Cf + C - 1) / C);
    if (we - ws > m) m = we - ws;
  }
  return m > 4 ? 4 : m;
}

// Shapes whose (source << 16) | cell entries the compacted list can hold: both ids in 16 bits, and never both products at the limit
// together — source 65 535 on cell 65 535 would be 0xffffffff, the list's "no entry" word.
bool compact_fits(int Hf, int Wf, int E) {
  const int64_t HW = (int64_t)Hf * Wf, E2 = (int64_t)E * E;
  return HW <= 65536 && E2 <= 65536 && !(HW == 65536 && E2 == 65536);
}

// the index kernels' arguments (wsmg_bev_index, wsmg_bev_index_compact, wsmg_bev_project: one set of camera constants)
IndexArgs index_args(const float* depth, int B, int Hd, int Wd, float depth_scale, int Hf, int Wf, int E, float local_scale,
                     int32_t* lin_idx) {
  IndexArgs a;
  a.depth = depth; a.lin = lin_idx;
  a.B = B; a.Hd = Hd; a.Wd = Wd; a.Hf = Hf; a.Wf = Wf; a.E = E;
  a.depth_scale = depth_scale;
  a.local_scale = local_scale;
  a.half = (float)((E - 1) / 2.0);
  // get_camera_matrix(imh, imw, 90): cx=imh/2, cy=imw/2, fx=(imh/2)/tan(45deg), fy=(imw/2)/tan(45deg) (float64 -> f32)
  const double tn = tan(45.0 * 3.14159265358979323846 / 180.0);
  a.cx = (float)(Hd / 2.0); a.cy = (float)(Wd / 2.0);
  a.fx = (float)((Hd / 2.0) / tn); a.fy = (float)((Wd / 2.0) / tn);
  a.K = (float)((double)Wd / (double)Wf);
  return a;
}

// how the scatter + rotation launches lay out their planes (bev_scatter_rotate_impl, wsmg_bev_project: the same grouping, table and
// magic number, or the two would not give the same bits)
struct PlaneLaunch { int CG, table; size_t lds; unsigned magicE; };
PlaneLaunch plane_launch(int B, int C, int E) {
  const size_t plane = (size_t)E * E * sizeof(unsigned);
  PlaneLaunch p;
  p.CG = (2 * plane <= 80 * 1024 && (int64_t)B * C >= 1024) ? 2 : 1;
  // the base-coordinate table rides in whatever LDS the planes leave (E = 200: 3 840 spare bytes of the 160 KB, 800 needed)
  p.table = plane * p.CG + (size_t)E * sizeof(float) <= 160 * 1024 ? 1 : 0;
  p.lds = plane * p.CG + (p.table ? (size_t)E * sizeof(float) : 0);
  p.magicE = (unsigned)((1ull << 32) / (unsigned)E + 1);      // p / E == umulhi(p, magicE) for p < E * E <= 40 960
  return p;
}

// The plane kernels are templates over WU (scatter_plane) and keep up to 160 KB of planes in dynamic LDS.  launch_by_window<K>
// launches K::kernel<wu>, wu = scatter_window() = 1..4, on 1024 threads; each instantiation has its dynamic-LDS limit lifted once
// per process, before its first launch.
struct ScatterKernel { template <int WU> static constexpr auto kernel = bev_scatter_kernel<WU>; };
struct ScatterRotateKernel { template <int WU> static constexpr auto kernel = bev_scatter_rotate_kernel<WU>; };
struct ProjectKernel { template <int WU> static constexpr auto kernel = bev_project_kernel<WU>; };
template <class K, int WU, class... Args>
int launch_window(dim3 grid, size_t lds, wsmg_stream_t stream, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(K::template kernel<WU>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL(K::template kernel<WU>, grid, dim3(1024), lds, wsmg_s(stream), args...);
  WSMG_RETURN_LAUNCH();
}
template <class K, class... Args>
int launch_by_window(int wu, dim3 grid, size_t lds, wsmg_stream_t stream, Args... args) {
  if (wu == 1) return launch_window<K, 1>(grid, lds, stream, args...);
  if (wu == 2) return launch_window<K, 2>(grid, lds, stream, args...);
  if (wu == 3) return launch_window<K, 3>(grid, lds, stream, args...);
  return launch_window<K, 4>(grid, lds, stream, args...);
}

}  // namespace

extern "C" int wsmg_bev_index(const float* depth, int B, int Hd, int Wd, float depth_scale, int Hf, int Wf, int E,
                              float local_scale, int32_t* lin_idx, wsmg_stream_t stream) {
  if (B <= 0 || Hd <= 0 || Wd <= 0 || Hf <= 0 || Wf <= 0 || E <= 0 || Hf > Hd || Wf > Wd) return WSMG_EINVAL;
  const IndexArgs a = index_args(depth, B, Hd, Wd, depth_scale, Hf, Wf, E, local_scale, lin_idx);
  if (B > 65535 || (int64_t)Hf * Wf >= (1ll << 31)) return WSMG_EINVAL;
  hipLaunchKernelGGL(bev_index_kernel, dim3(sgrid((int64_t)Hf * Wf, 1024), (unsigned)B), dim3(256), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}

// wsmg_bev_index + the compacted list of valid sources (round 6): clist [B][Hf*Wf] uint32, cnt [B][ceil(Hf*Wf / 8192)] int32, both
// written in full by this launch (nothing to zero); needs Hf*Wf <= 65536 and E*E <= 65536, not both at 65536 (compact_fits).
extern "C" int wsmg_bev_index_compact(const float* depth, int B, int Hd, int Wd, float depth_scale, int Hf, int Wf, int E,
                                      float local_scale, int32_t* lin_idx, uint32_t* clist, int32_t* cnt, wsmg_stream_t stream) {
  if (B <= 0 || Hd <= 0 || Wd <= 0 || Hf <= 0 || Wf <= 0 || E <= 0 || Hf > Hd || Wf > Wd || B > 65535) return WSMG_EINVAL;
  if (!compact_fits(Hf, Wf, E) || !clist || !cnt || !lin_idx) return WSMG_EINVAL;
  const IndexArgs a = index_args(depth, B, Hd, Wd, depth_scale, Hf, Wf, E, local_scale, lin_idx);
  hipLaunchKernelGGL(bev_index_compact_kernel, dim3((unsigned)wsmg_cdiv((int64_t)Hf * Wf, CB), (unsigned)B), dim3(1024), 0, wsmg_s(stream), a,
                     clist, cnt);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_bev_scatter_max(const float* feat, const int32_t* lin_idx, int B, int Cf, int Hf, int Wf, int C,
                                    int E, float* out, wsmg_stream_t stream) {
  if (B <= 0 || Cf <= 0 || C <= 0 || C > Cf || E <= 0 || B > 65535) return WSMG_EINVAL;
  const int E2 = E * E;
  const size_t plane = (size_t)E2 * sizeof(unsigned);
  if (plane > 160 * 1024) return WSMG_EINVAL;
  // two planes per workgroup when that still leaves >= 2 workgroups per CU's LDS and enough workgroups
  int CG = (2 * plane <= 80 * 1024 && (int64_t)B * C >= 1024) ? 2 : 1;
  dim3 grid((unsigned)wsmg_cdiv(C, CG), (unsigned)B);
  return launch_by_window<ScatterKernel>(scatter_window(Cf, C), grid, plane * CG, stream, feat, lin_idx, Cf, Hf * Wf, C, E2, CG, out);
}

extern "C" int wsmg_bev_rotate(const float* in, const float* heading, float sign, int B, int C, int E, float* out,
                               wsmg_stream_t stream) {
  if (B <= 0 || C <= 0 || C > 64 || E <= 1 || B > 65535) return WSMG_EINVAL;
  const int nb8 = (E + 7) / 8;
  dim3 grid((unsigned)(nb8 * nb8), (unsigned)B);
  hipLaunchKernelGGL(rotate_nchw_to_nhwc_kernel, grid, dim3(256), 0, wsmg_s(stream), in, heading, sign, C, E, out);
  WSMG_RETURN_LAUNCH();
}

static int bev_scatter_rotate_impl(const float* feat, const int32_t* lin_idx, const uint32_t* clist, const int32_t* cnt, const float* heading,
                                   float sign, int B, int Cf, int Hf, int Wf, int C, int E, float* out_planes, wsmg_stream_t stream) {
  if (B <= 0 || Cf <= 0 || C <= 0 || C > Cf || E <= 1 || B > 65535) return WSMG_EINVAL;
  if (clist && (!cnt || !compact_fits(Hf, Wf, E))) return WSMG_EINVAL;
  const int nblk = (int)wsmg_cdiv((int64_t)Hf * Wf, CB);
  if ((size_t)E * E * sizeof(unsigned) > 160 * 1024) return WSMG_EINVAL;
  const PlaneLaunch pl = plane_launch(B, C, E);
  dim3 grid((unsigned)wsmg_cdiv(C, pl.CG), (unsigned)B);
  return launch_by_window<ScatterRotateKernel>(scatter_window(Cf, C), grid, pl.lds, stream, feat, lin_idx, heading, sign, Cf, Hf * Wf, C, E,
                                               pl.CG, pl.magicE, pl.table, out_planes, clist, cnt, nblk);
}

extern "C" int wsmg_bev_scatter_rotate(const float* feat, const int32_t* lin_idx, const float* heading, float sign, int B, int Cf,
                                       int Hf, int Wf, int C, int E, float* out_planes, wsmg_stream_t stream) {
  return bev_scatter_rotate_impl(feat, lin_idx, nullptr, nullptr, heading, sign, B, Cf, Hf, Wf, C, E, out_planes, stream);
}
// the same from wsmg_bev_index_compact's list of valid sources (bit-identical planes)
extern "C" int wsmg_bev_scatter_rotate_compact(const float* feat, const uint32_t* clist, const int32_t* cnt, const float* heading, float sign,
                                               int B, int Cf, int Hf, int Wf, int C, int E, float* out_planes, wsmg_stream_t stream) {
  if (!clist || !cnt) return WSMG_EINVAL;
  return bev_scatter_rotate_impl(feat, nullptr, clist, cnt, heading, sign, B, Cf, Hf, Wf, C, E, out_planes, stream);
}

// wsmg_bev_index + wsmg_bev_scatter_rotate in one launch (bev_project_kernel); lin_idx may be NULL
extern "C" int wsmg_bev_project(const float* depth, const float* feat, const float* heading, float sign, int B, int Hd, int Wd,
                                float depth_scale, int Cf, int Hf, int Wf, int C, int E, float local_scale, int32_t* lin_idx,
                                float* out_planes, wsmg_stream_t stream) {
  if (B <= 0 || Hd <= 0 || Wd <= 0 || Hf <= 0 || Wf <= 0 || Hf > Hd || Wf > Wd || (int64_t)Hf * Wf >= (1ll << 31)) return WSMG_EINVAL;
  if (Cf <= 0 || C <= 0 || C > Cf || E <= 1 || B > 65535) return WSMG_EINVAL;
  if ((size_t)E * E * sizeof(unsigned) > 160 * 1024) return WSMG_EINVAL;
  const IndexArgs a = index_args(depth, B, Hd, Wd, depth_scale, Hf, Wf, E, local_scale, lin_idx);
  const PlaneLaunch pl = plane_launch(B, C, E);
  dim3 grid((unsigned)wsmg_cdiv(C, pl.CG), (unsigned)B);
  return launch_by_window<ProjectKernel>(scatter_window(Cf, C), grid, pl.lds, stream, feat, a, heading, sign, Cf, C, pl.CG, pl.magicE,
                                         pl.table, out_planes);
}
