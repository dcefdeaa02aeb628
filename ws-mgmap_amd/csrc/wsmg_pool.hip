// Element-wise and window kernels over NHWC activations (float32 / bf16 storage, float32 arithmetic) of the UNet-style decoders:
// ReLU in all its forms, MaxPool2d(3,2,1) with and without kept taps, avg_pool2d(2), bilinear 2x upsample (align_corners=True),
// upsample + concatenate, channel concatenation, the three-way gradient add and the token-gradient merge.
// Reference call sites: map_encoder.py:80,84,102,108; unet_encoder.py:95-109; mg_map_policy.py:89-100,217.
// All are streaming, HBM-bound kernels; backward passes are written as gathers so results are deterministic (no atomics).
// The layout changes that used to live here are in wsmg_layout.hip, the NHWC cross-entropy in wsmg_loss.hip.
#include <type_traits>

#include "wsmg_common.h"

namespace {

#define GRID_STRIDE(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

template <class T>
__global__ void relu_fwd_kernel(const T* x, T* y, int64_t n4) {
  GRID_STRIDE(i, n4) {
    f32x4 v = ld4(x + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
    st4(y + i * 4, v);
  }
}
template <class T>
__global__ void relu_bwd_kernel(const T* dy, const T* y, T* dx, int64_t n4) {
  GRID_STRIDE(i, n4) {
    f32x4 g = ld4(dy + i * 4), v = ld4(y + i * 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? g[j] : 0.f;
    st4(dx + i * 4, g);
  }
}

// All pool / upsample kernels below: one thread = 4 consecutive channels of one pixel (16-byte f32 / 8-byte bf16
// accesses; C % 4 == 0 is guaranteed by the engine's 32-channel padding), pixel geometry computed once per 4 values.
#define PIX_DECODE(i, C4, WW, HH, c, px, py, b)   \
  const int c = (int)((i) % (C4)) * 4;             \
  const int64_t p_ = (i) / (C4);                   \
  const int px = (int)(p_ % (WW));                 \
  const int py = (int)((p_ / (WW)) % (HH));        \
  const int b = (int)(p_ / ((int64_t)(WW) * (HH)));

// ---- MaxPool2d(kernel 3, stride 2, pad 1).  The one scan of the window of output (b, oy, ox), channels c .. c + 3: the four best
// values and their taps 3 ky + kx.  The first maximum in (ky, kx) scan order wins ties (ATen), a NaN wins over everything before
// it, and the first valid tap is taken whatever it holds (tap < 0), so a window of nothing but -inf names a tap too.
struct PoolBest { f32x4 v; int tap[4]; };
template <class T>
__device__ inline PoolBest maxpool_scan4(const T* x, int b, int oy, int ox, int c, int H, int W, int C) {
  PoolBest r = {{-INFINITY, -INFINITY, -INFINITY, -INFINITY}, {-1, -1, -1, -1}};
  for (int ky = 0; ky < 3; ++ky) {
    int iy = oy * 2 - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      int ix = ox * 2 - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      f32x4 v = ld4(x + (((size_t)b * H + iy) * W + ix) * C + c);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (v[j] > r.v[j] || v[j] != v[j] || r.tap[j] < 0) { r.v[j] = v[j]; r.tap[j] = 3 * ky + kx; }
    }
  }
  return r;
}
// the tap input pixel (iy, ix) has in the window of output (oy, ox); the caller knows it lies inside
__device__ __forceinline__ int maxpool_tap_of(int iy, int ix, int oy, int ox) { return 3 * (iy - (2 * oy - 1)) + (ix - (2 * ox - 1)); }

template <class T>
__global__ void maxpool_fwd_kernel(const T* x, T* y, int B, int H, int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  int64_t n = (int64_t)B * OH * OW * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, OW, OH, c, ox, oy, b)
    st4(y + i * 4, maxpool_scan4(x, b, oy, ox, c, H, W, C).v);
  }
}

// the backward that recomputes the winning tap of up to four windows per input element from x
template <class T>
__global__ void maxpool_bwd_kernel(const T* dy, const T* x, T* dx, int B, int H, int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  int64_t n = (int64_t)B * H * W * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, W, H, c, ix, iy, b)
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    int oy0 = iy / 2, oy1 = (iy + 1) / 2;  // windows [2oy-1, 2oy+1] containing iy
    int ox0 = ix / 2, ox1 = (ix + 1) / 2;
    for (int oy = oy0; oy <= oy1; ++oy) {
      if (oy >= OH) continue;
      for (int ox = ox0; ox <= ox1; ++ox) {
        if (ox >= OW) continue;
        const PoolBest r = maxpool_scan4(x, b, oy, ox, c, H, W, C);
        const int mine = maxpool_tap_of(iy, ix, oy, ox);
        const f32x4 d = ld4(dy + (((size_t)b * OH + oy) * OW + ox) * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (r.tap[j] == mine) g[j] += d[j];
      }
    }
    st4(dx + i * 4, g);
  }
}

// ---- the same pool with the winning tap of every output element kept (round 3): one byte per element.  The backward above
// recomputes the arg-max of up to four windows per input element — 36 loads and their compares for one store: 50 us for the
// decoder's 12 x 12 map at B = 512, a 9 MB tensor, on the critical chain of small launches; with the taps it is four index words
// and four gradient loads.
template <class T>
__global__ void maxpool_fwd_idx_kernel(const T* x, T* y, unsigned* idx, int B, int H, int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  int64_t n = (int64_t)B * OH * OW * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, OW, OH, c, ox, oy, b)
    const PoolBest r = maxpool_scan4(x, b, oy, ox, c, H, W, C);
    st4(y + i * 4, r.v);
    idx[i] = (unsigned)r.tap[0] | ((unsigned)r.tap[1] << 8) | ((unsigned)r.tap[2] << 16) | ((unsigned)r.tap[3] << 24);
  }
}
template <class T>
__global__ void maxpool_bwd_idx_kernel(const T* dy, const unsigned* idx, T* dx, int B, int H, int W, int C, int OH, int OW) {
  const int C4 = C / 4;
  int64_t n = (int64_t)B * H * W * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, W, H, c, ix, iy, b)
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
    const int oy0 = iy / 2, oy1 = (iy + 1) / 2, ox0 = ix / 2, ox1 = (ix + 1) / 2;   // windows [2o - 1, 2o + 1] containing (iy, ix)
    for (int oy = oy0; oy <= oy1; ++oy) {
      if (oy >= OH) continue;
      for (int ox = ox0; ox <= ox1; ++ox) {
        if (ox >= OW) continue;
        const unsigned tap = (unsigned)maxpool_tap_of(iy, ix, oy, ox);
        const size_t o = (((size_t)b * OH + oy) * OW + ox) * C4 + c / 4;
        const unsigned w = idx[o];
        const f32x4 d = ld4(dy + o * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (((w >> (8 * j)) & 0xffu) == tap) g[j] += d[j];
      }
    }
    st4(dx + i * 4, g);
  }
}

// ---- bilinear x2, align_corners=True (ATen upsample_bilinear2d: src = dst * (in-1)/(out-1))
__device__ inline void up_src(int o, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
  float s = scale * (float)o;
  i0 = (int)s;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}
// The four-tap expression stands here and in upsample_cat_bf16_kernel, not in one function: the compiler pairs its multiplies into
// packed FMAs per channel (channel 0 fma(wx0, v00, wx1 v01), channel 1 fma(wx1, v01, wx0 v00)), moving it into a function changed
// the pairing and with it float32 result bits (profiles/pool_refactor.txt).
template <class T>
__global__ void upsample_fwd_kernel(const T* x, T* y, int B, int H, int W, int C) {
  const int OH = 2 * H, OW = 2 * W, C4 = C / 4;
  const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  int64_t n = (int64_t)B * OH * OW * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, OW, OH, c, ox, oy, b)
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    up_src(oy, H, sh, y0, y1, hy0, hy1);
    up_src(ox, W, sw, x0, x1, wx0, wx1);
    const T* xb = x + (size_t)b * H * W * C + c;
    const f32x4 v00 = ld4(xb + ((size_t)y0 * W + x0) * C), v01 = ld4(xb + ((size_t)y0 * W + x1) * C);
    const f32x4 v10 = ld4(xb + ((size_t)y1 * W + x0) * C), v11 = ld4(xb + ((size_t)y1 * W + x1) * C);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = hy0 * (wx0 * v00[j] + wx1 * v01[j]) + hy1 * (wx0 * v10[j] + wx1 * v11[j]);
    st4(y + i * 4, o);
  }
}

// g += w * (N consecutive channels of a pixel as loaded: wsmg_common.h's chans_t)
template <int N>
__device__ __forceinline__ void fma_chans(float (&g)[N], float w, chans_t<N> d) {
  float v[N];
  chans_f32<N>(d, v);
#pragma unroll
  for (int j = 0; j < N; ++j) g[j] += w * v[j];
}

// The upsample's backward as a gather, N = 4 or 8 channels per thread (8: bf16 only, one 16-byte access): dx[iy][ix] = the sum over the
// output rows ascending, output columns ascending, of g += (wy wx) dy — one order for every N and dtype, so the widths agree bit
// for bit.  The row and the column weights of the (at most 6 + 6) candidate positions are worked out once per thread, not once per
// (row, column) pair (36 evaluations of the source-index arithmetic per thread were most of an earlier form's time: 61 us for the
// 151 MB layer), the candidates with weight 0 are dropped before any load, and the loads of a row (4-5 of them) are issued together.
template <class T, int N>
__global__ __launch_bounds__(256) void upsample_bwdn_kernel(const T* __restrict__ dy, T* __restrict__ dx, int B, int H, int W, int C,
                                                            int64_t ld_dy) {   // ld_dy: pixel stride of dy
  const int OH = 2 * H, OW = 2 * W, CN = C / N;
  const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  const int64_t n = (int64_t)B * H * W * CN;
  GRID_STRIDE(i, n) {
    const int c = (int)(i % CN) * N;
    const int64_t p_ = i / CN;
    const int ix = (int)(p_ % W), iy = (int)((p_ / W) % H), b = (int)(p_ / ((int64_t)W * H));
    // the output rows / columns that read this input row / column (4, sometimes 5; 6 at H = 2), ascending, with their weights
    int oys[6], oxs[6], ny = 0, nx = 0;
    float wys[6], wxs[6];
    const int oy_lo = 2 * iy - 2 < 0 ? 0 : 2 * iy - 2, oy_hi = 2 * iy + 3 > OH - 1 ? OH - 1 : 2 * iy + 3;
    const int ox_lo = 2 * ix - 2 < 0 ? 0 : 2 * ix - 2, ox_hi = 2 * ix + 3 > OW - 1 ? OW - 1 : 2 * ix + 3;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      const int oy = oy_lo + t;
      if (oy <= oy_hi) {
        int y0, y1;
        float hy0, hy1;
        up_src(oy, H, sh, y0, y1, hy0, hy1);
        const float wy = (y0 == iy ? hy0 : 0.f) + (y1 == iy ? hy1 : 0.f);
        if (wy != 0.f) { oys[ny] = oy; wys[ny] = wy; ++ny; }
      }
      const int ox = ox_lo + t;
      if (ox <= ox_hi) {
        int x0, x1;
        float wx0, wx1;
        up_src(ox, W, sw, x0, x1, wx0, wx1);
        const float wx = (x0 == ix ? wx0 : 0.f) + (x1 == ix ? wx1 : 0.f);
        if (wx != 0.f) { oxs[nx] = ox; wxs[nx] = wx; ++nx; }
      }
    }
    float g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = 0.f;
    const T* const base = dy + (size_t)b * OH * OW * ld_dy + c;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      if (a >= ny) break;
      chans_t<N> d[6];
#pragma unroll
      for (int e = 0; e < 6; ++e)
        if (e < nx) d[e] = ld_chans_raw<N>(base + ((size_t)oys[a] * OW + oxs[e]) * ld_dy);
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        if (e >= nx) break;
        fma_chans<N>(g, wys[a] * wxs[e], d[e]);
      }
    }
    st_chans<N>(dx + i * N, g);
  }
}

// ---- avg_pool2d(2,2), H and W even
template <class T>
__global__ void avgpool_fwd_kernel(const T* x, T* y, int B, int H, int W, int C) {
  const int OH = H / 2, OW = W / 2, C4 = C / 4;
  int64_t n = (int64_t)B * OH * OW * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, OW, OH, c, ox, oy, b)
    const T* xb = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * C + c;
    const f32x4 a0 = ld4(xb), a1 = ld4(xb + C), a2 = ld4(xb + (size_t)W * C), a3 = ld4(xb + (size_t)W * C + C);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (a0[j] + a1[j] + a2[j] + a3[j]) * 0.25f;
    st4(y + i * 4, o);
  }
}
template <class T>
__global__ void avgpool_bwd_kernel(const T* dy, T* dx, int B, int H, int W, int C) {
  const int OH = H / 2, OW = W / 2, C4 = C / 4;
  int64_t n = (int64_t)B * H * W * C4;
  GRID_STRIDE(i, n) {
    PIX_DECODE(i, C4, W, H, c, ix, iy, b)
    f32x4 d = ld4(dy + (((size_t)b * OH + iy / 2) * OW + ix / 2) * C + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= 0.25f;
    st4(dx + i * 4, d);
  }
}

// ---- channel concatenation of two NHWC tensors (the UNet skip connections, map_encoder.py:104,110, and
// mg_map_policy.py:99): out[p] = a[p] ++ b[p], one 16-byte chunk per thread, the pixel index computed once per chunk
__global__ void cat_channels_kernel(const u32x4* __restrict__ a, const u32x4* __restrict__ b, u32x4* __restrict__ y,
                                    int64_t rows, int ca, int cb) {
  const int cy = ca + cb;
  const int64_t n = rows * cy;
  GRID_STRIDE(i, n) {
    const int64_t p = i / cy;
    const int c = (int)(i - p * cy);
    y[i] = c < ca ? a[p * ca + c] : b[p * cb + (c - ca)];
  }
}

// Rollout route of the UNet decoders (unet_encoder.py:95-109, map_encoder.py:103-110): cat([upsample2x(a), b], channels) in one
// pass, bf16 — the upsampled tensor is never written (and read back by the concatenation); 8 channels per thread, the
// interpolation arithmetic of upsample_fwd_kernel.
__global__ void upsample_cat_bf16_kernel(const bf16_t* __restrict__ a, const u32x4* __restrict__ b, u32x4* __restrict__ y, int B,
                                         int H, int W, int ca8, int cb8) {
  const int OH = 2 * H, OW = 2 * W, cy = ca8 + cb8, C = ca8 * 8;
  const float sh = OH > 1 ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = OW > 1 ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  const int64_t n = (int64_t)B * OH * OW * cy;
  GRID_STRIDE(i, n) {
    const int64_t p = i / cy;
    const int c = (int)(i - p * cy);
    if (c >= ca8) {
      y[i] = b[p * cb8 + (c - ca8)];
      continue;
    }
    const int ox = (int)(p % OW);
    const int64_t q = p / OW;
    const int oy = (int)(q % OH), bb = (int)(q / OH);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    up_src(oy, H, sh, y0, y1, hy0, hy1);
    up_src(ox, W, sw, x0, x1, wx0, wx1);
    const bf16_t* xb = a + (size_t)bb * H * W * C + c * 8;
    u32x4 o;
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
      const f32x4 v00 = ld4(xb + ((size_t)y0 * W + x0) * C + 4 * hlf), v01 = ld4(xb + ((size_t)y0 * W + x1) * C + 4 * hlf);
      const f32x4 v10 = ld4(xb + ((size_t)y1 * W + x0) * C + 4 * hlf), v11 = ld4(xb + ((size_t)y1 * W + x1) * C + 4 * hlf);
      unsigned short r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16_t v = (bf16_t)(hy0 * (wx0 * v00[j] + wx1 * v01[j]) + hy1 * (wx0 * v10[j] + wx1 * v11[j]));
        r[j] = __builtin_bit_cast(unsigned short, v);
      }
      o[2 * hlf] = (unsigned)r[0] | ((unsigned)r[1] << 16);
      o[2 * hlf + 1] = (unsigned)r[2] | ((unsigned)r[3] << 16);
    }
    y[i] = o;
  }
}

// bf16: 8 values (one 16-byte access) per thread
__device__ __forceinline__ unsigned relu2(unsigned v) {   // two packed bf16: x > 0 ? x : 0 (NaN -> 0, like the float compare)
  const float lo = __uint_as_float(v << 16), hi = __uint_as_float(v & 0xffff0000u);
  return (lo > 0.f ? (v & 0xffffu) : 0u) | (hi > 0.f ? (v & 0xffff0000u) : 0u);
}
__device__ __forceinline__ unsigned mask2(unsigned g, unsigned y) {   // g where y > 0, else 0
  const float lo = __uint_as_float(y << 16), hi = __uint_as_float(y & 0xffff0000u);
  return (lo > 0.f ? (g & 0xffffu) : 0u) | (hi > 0.f ? (g & 0xffff0000u) : 0u);
}
// a + b + c of three bf16 tensors in one pass, float32 sums, one rounding (round 3: the gradient of a tensor with three
// consumers — the encoded map feeds the token projection, the decoder's stem and its full-resolution branch — instead of two
// add launches of six passes over 151 MB each way)
__device__ __forceinline__ unsigned add3_2(unsigned a, unsigned b, unsigned c) {
  const float lo = __uint_as_float(a << 16) + __uint_as_float(b << 16) + __uint_as_float(c << 16);
  const float hi = __uint_as_float(a & 0xffff0000u) + __uint_as_float(b & 0xffff0000u) + __uint_as_float(c & 0xffff0000u);
  const bf16_t l = (bf16_t)lo, h = (bf16_t)hi;
  return (unsigned)__builtin_bit_cast(unsigned short, l) | ((unsigned)__builtin_bit_cast(unsigned short, h) << 16);
}
__global__ void add3_bf16_kernel(const u32x4* __restrict__ a, const u32x4* __restrict__ b, const u32x4* __restrict__ c,
                                 u32x4* __restrict__ y, int64_t n8) {
  GRID_STRIDE(i, n8) {
    const u32x4 u = a[i], v = b[i], w = c[i];
    u32x4 o = {add3_2(u[0], v[0], w[0]), add3_2(u[1], v[1], w[1]), add3_2(u[2], v[2], w[2]), add3_2(u[3], v[3], w[3])};
    y[i] = o;
  }
}
__global__ void relu_fwd8_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ y, int64_t n8) {
  GRID_STRIDE(i, n8) {
    const u32x4 v = x[i];
    u32x4 o = {relu2(v[0]), relu2(v[1]), relu2(v[2]), relu2(v[3])};
    y[i] = o;
  }
}
__global__ void relu_bwd8_kernel(const u32x4* __restrict__ dy, const u32x4* __restrict__ y, u32x4* __restrict__ dx, int64_t n8) {
  GRID_STRIDE(i, n8) {
    const u32x4 g = dy[i], v = y[i];
    u32x4 o = {mask2(g[0], v[0]), mask2(g[1], v[1]), mask2(g[2], v[2]), mask2(g[3], v[3])};
    dx[i] = o;
  }
}

// the same with a row stride on dy (rows of C8 16-byte pieces, `ld8` pieces apart): a channel slice of a wider gradient read in place
__global__ void relu_bwd8_rows_kernel(const u32x4* __restrict__ dy, int64_t ld8, const u32x4* __restrict__ y, u32x4* __restrict__ dx,
                                      int C8, int64_t n8) {
  GRID_STRIDE(i, n8) {
    const int64_t r = i / C8;
    const u32x4 g = dy[r * ld8 + (i - r * C8)], v = y[i];
    u32x4 o = {mask2(g[0], v[0]), mask2(g[1], v[1]), mask2(g[2], v[2]), mask2(g[3], v[3])};
    dx[i] = o;
  }
}

// dx[b][i][c] = (dx[b][i][c] + g[b][c] * inv_I) * (x[b][i][c] > 0), in place: the gradient of the map tokens from the attention
// (already in dx) merged with the broadcast gradient of their token mean (mg_map_policy.py:217: AdaptiveAvgPool1d over the 576
// tokens) and masked by the fused ReLU of the convolution that produced the tokens (map_cated_linear, :99-100) — one pass
// instead of an add launch over a materialised broadcast plus a ReLU-mask launch.
template <class T>
__global__ void token_grad_merge_kernel(T* __restrict__ dx, const T* __restrict__ x, const float* __restrict__ g, int I, int C,
                                        float inv_I, int relu, int64_t n4) {
  const int C4 = C / 4;
  GRID_STRIDE(i, n4) {
    const int c = (int)(i % C4) * 4;
    const int64_t b = i / ((int64_t)C4 * I);
    f32x4 d = ld4(dx + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + b * C + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = fmaf(gv[j], inv_I, d[j]);
    if (relu) {
      const f32x4 xv = ld4(x + i * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = xv[j] > 0.f ? d[j] : 0.f;
    }
    st4(dx + i * 4, d);
  }
}

// ---- launch wrappers.  What every [B][H][W][C] kernel here asks of its tensor: a positive extent, channels in whole fours
bool nhwc4_ok(int B, int H, int W, int C) { return B > 0 && H > 0 && W > 0 && C > 0 && !(C & 3); }
// the pool's: OH x OW is the one output size of MaxPool2d(3, 2, 1) over H x W (which ties H and W to it; they are not asked to be
// positive on their own)
bool maxpool_geom_ok(int B, int H, int W, int C, int OH, int OW) {
  return OH == (H + 2 - 3) / 2 + 1 && OW == (W + 2 - 3) / 2 + 1 && nhwc4_ok(B, 1, 1, C);
}

template <class T>
int token_grad_merge_t(T* dx, const T* x, const float* g, int B, int I, int C, int relu, wsmg_stream_t stream) {
  if (!nhwc4_ok(B, I, 1, C)) return WSMG_EINVAL;
  const int64_t n4 = (int64_t)B * I * C / 4;
  hipLaunchKernelGGL(token_grad_merge_kernel<T>, dim3(wsmg_sgrid(n4)), dim3(256), 0, wsmg_s(stream), dx, x, g, I, C, 1.0f / (float)I, relu, n4);
  WSMG_RETURN_LAUNCH();
}

template <class T>
int relu_fwd_t(const T* x, T* y, int64_t n, wsmg_stream_t stream) {
  if (n <= 0 || n % 4) return WSMG_EINVAL;
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (n % 8 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
      hipLaunchKernelGGL(relu_fwd8_kernel, dim3(wsmg_sgrid(n / 8)), dim3(256), 0, wsmg_s(stream), (const u32x4*)x, (u32x4*)y, n / 8);
      WSMG_RETURN_LAUNCH();
    }
  }
  hipLaunchKernelGGL(relu_fwd_kernel<T>, dim3(wsmg_sgrid(n / 4)), dim3(256), 0, wsmg_s(stream), x, y, n / 4);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int relu_bwd_t(const T* dy, const T* y, T* dx, int64_t n, wsmg_stream_t stream) {
  if (n <= 0 || n % 4) return WSMG_EINVAL;
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (n % 8 == 0 && (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dx) & 15) == 0) {
      hipLaunchKernelGGL(relu_bwd8_kernel, dim3(wsmg_sgrid(n / 8)), dim3(256), 0, wsmg_s(stream), (const u32x4*)dy, (const u32x4*)y,
                         (u32x4*)dx, n / 8);
      WSMG_RETURN_LAUNCH();
    }
  }
  hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3(wsmg_sgrid(n / 4)), dim3(256), 0, wsmg_s(stream), dy, y, dx, n / 4);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int maxpool_fwd_t(const T* x, T* y, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t stream) {
  if (!maxpool_geom_ok(B, H, W, C, OH, OW)) return WSMG_EINVAL;
  hipLaunchKernelGGL(maxpool_fwd_kernel<T>, dim3(wsmg_sgrid((int64_t)B * OH * OW * C / 4)), dim3(256), 0, wsmg_s(stream), x, y, B, H, W, C, OH, OW);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int maxpool_bwd_t(const T* dy, const T* x, T* dx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t stream) {
  if (!maxpool_geom_ok(B, H, W, C, OH, OW)) return WSMG_EINVAL;
  hipLaunchKernelGGL(maxpool_bwd_kernel<T>, dim3(wsmg_sgrid((int64_t)B * H * W * C / 4)), dim3(256), 0, wsmg_s(stream), dy, x, dx, B, H, W, C, OH, OW);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int maxpool_fwd_idx_t(const T* x, T* y, uint32_t* idx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t stream) {
  if (!maxpool_geom_ok(B, H, W, C, OH, OW) || !idx) return WSMG_EINVAL;
  hipLaunchKernelGGL(maxpool_fwd_idx_kernel<T>, dim3(wsmg_sgrid((int64_t)B * OH * OW * C / 4)), dim3(256), 0, wsmg_s(stream), x, y, idx, B, H, W, C, OH, OW);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int maxpool_bwd_idx_t(const T* dy, const uint32_t* idx, T* dx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t stream) {
  if (!maxpool_geom_ok(B, H, W, C, OH, OW) || !idx) return WSMG_EINVAL;
  hipLaunchKernelGGL(maxpool_bwd_idx_kernel<T>, dim3(wsmg_sgrid((int64_t)B * H * W * C / 4)), dim3(256), 0, wsmg_s(stream), dy, idx, dx, B, H, W, C, OH, OW);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int upsample_fwd_t(const T* x, T* y, int B, int H, int W, int C, wsmg_stream_t stream) {
  if (!nhwc4_ok(B, H, W, C)) return WSMG_EINVAL;
  hipLaunchKernelGGL(upsample_fwd_kernel<T>, dim3(wsmg_sgrid((int64_t)B * H * W * C)), dim3(256), 0, wsmg_s(stream), x, y, B, H, W, C);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int upsample_bwd_t(const T* dy, T* dx, int B, int H, int W, int C, wsmg_stream_t stream, int64_t ld_dy = 0) {
  if (!nhwc4_ok(B, H, W, C)) return WSMG_EINVAL;
  if (ld_dy == 0) ld_dy = C;
  // the 4-channel kernel reads 4 elements at a time, so a pixel stride of 4 k will do (a contiguous dy of 4, 12 or 20 channels, which
  // the forward pass accepts, was refused here while this asked for 8 k); only the 8-channel kernel needs 8 k
  if (ld_dy < C || (ld_dy & 3) || ((uintptr_t)dy & 15)) return WSMG_EINVAL;
  if constexpr (std::is_same<T, bf16_t>::value) {
    if ((C & 7) == 0 && (ld_dy & 7) == 0 && ((uintptr_t)dx & 15) == 0) {
      hipLaunchKernelGGL((upsample_bwdn_kernel<T, 8>), dim3(wsmg_sgrid((int64_t)B * H * W * C / 8)), dim3(256), 0, wsmg_s(stream), dy, dx, B, H,
                         W, C, ld_dy);
      WSMG_RETURN_LAUNCH();
    }
  }
  hipLaunchKernelGGL((upsample_bwdn_kernel<T, 4>), dim3(wsmg_sgrid((int64_t)B * H * W * C / 4)), dim3(256), 0, wsmg_s(stream), dy, dx, B, H, W, C, ld_dy);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int avgpool_fwd_t(const T* x, T* y, int B, int H, int W, int C, wsmg_stream_t stream) {
  if (!nhwc4_ok(B, H, W, C) || (H & 1) || (W & 1)) return WSMG_EINVAL;
  hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(wsmg_sgrid((int64_t)B * H * W * C / 16)), dim3(256), 0, wsmg_s(stream), x, y, B, H, W, C);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int avgpool_bwd_t(const T* dy, T* dx, int B, int H, int W, int C, wsmg_stream_t stream) {
  if (!nhwc4_ok(B, H, W, C) || (H & 1) || (W & 1)) return WSMG_EINVAL;
  hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(wsmg_sgrid((int64_t)B * H * W * C / 4)), dim3(256), 0, wsmg_s(stream), dy, dx, B, H, W, C);
  WSMG_RETURN_LAUNCH();
}

}  // namespace

#define B16(p) ((bf16_t*)(p))
#define CB16(p) ((const bf16_t*)(p))
extern "C" int wsmg_cat_channels(const void* a, const void* b, void* y, int64_t rows, int bytes_a, int bytes_b, wsmg_stream_t s) {
  if (rows <= 0 || bytes_a <= 0 || bytes_b <= 0 || (bytes_a & 15) || (bytes_b & 15)) return WSMG_EINVAL;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) return WSMG_EINVAL;
  const int ca = bytes_a / 16, cb = bytes_b / 16;
  hipLaunchKernelGGL(cat_channels_kernel, dim3(wsmg_sgrid(rows * (ca + cb))), dim3(256), 0, wsmg_s(s), (const u32x4*)a, (const u32x4*)b,
                     (u32x4*)y, rows, ca, cb);
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_upsample2x_cat_bf16(const void* a, const void* b, void* y, int B, int H, int W, int Ca, int Cb, wsmg_stream_t s) {
  if (B <= 0 || H <= 0 || W <= 0 || Ca <= 0 || Cb <= 0 || (Ca & 7) || (Cb & 7)) return WSMG_EINVAL;
  if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)y) & 15) return WSMG_EINVAL;
  hipLaunchKernelGGL(upsample_cat_bf16_kernel, dim3(wsmg_sgrid((int64_t)B * 4 * H * W * (Ca + Cb) / 8)), dim3(256), 0, wsmg_s(s), CB16(a),
                     (const u32x4*)b, (u32x4*)y, B, H, W, Ca / 8, Cb / 8);
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_add3_bf16(const void* a, const void* b, const void* c, void* y, int64_t n, wsmg_stream_t s) {
  if (!a || !b || !c || !y || n <= 0 || (n & 7) || (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)y) & 15)) return WSMG_EINVAL;
  hipLaunchKernelGGL(add3_bf16_kernel, dim3(wsmg_sgrid(n / 8)), dim3(256), 0, wsmg_s(s), (const u32x4*)a, (const u32x4*)b, (const u32x4*)c,
                     (u32x4*)y, n / 8);
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_relu_fwd(const float* x, float* y, int64_t n, wsmg_stream_t s) { return relu_fwd_t<float>(x, y, n, s); }
extern "C" int wsmg_relu_fwd_bf16(const void* x, void* y, int64_t n, wsmg_stream_t s) { return relu_fwd_t<bf16_t>(CB16(x), B16(y), n, s); }
extern "C" int wsmg_token_grad_merge(float* dx, const float* x, const float* g, int B, int I, int C, int relu, wsmg_stream_t s) {
  return token_grad_merge_t<float>(dx, x, g, B, I, C, relu, s);
}
extern "C" int wsmg_token_grad_merge_bf16(void* dx, const void* x, const float* g, int B, int I, int C, int relu, wsmg_stream_t s) {
  return token_grad_merge_t<bf16_t>(B16(dx), CB16(x), g, B, I, C, relu, s);
}
extern "C" int wsmg_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, wsmg_stream_t s) { return relu_bwd_t<float>(dy, y, dx, n, s); }
extern "C" int wsmg_relu_bwd_bf16(const void* dy, const void* y, void* dx, int64_t n, wsmg_stream_t s) { return relu_bwd_t<bf16_t>(CB16(dy), CB16(y), B16(dx), n, s); }
extern "C" int wsmg_relu_bwd_rows_bf16(const void* dy, int64_t ld_dy, const void* y, void* dx, int64_t rows, int C, wsmg_stream_t s) {
  if (rows <= 0 || C <= 0 || (C & 7) || ld_dy < C || (ld_dy & 7) || (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)dx) & 15)) return WSMG_EINVAL;
  hipLaunchKernelGGL(relu_bwd8_rows_kernel, dim3(wsmg_sgrid(rows * C / 8)), dim3(256), 0, wsmg_s(s), (const u32x4*)dy, ld_dy / 8,
                     (const u32x4*)y, (u32x4*)dx, C / 8, rows * C / 8);
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_maxpool3x3s2_fwd(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_fwd_t<float>(x, y, B, H, W, C, OH, OW, s); }
extern "C" int wsmg_maxpool3x3s2_fwd_bf16(const void* x, void* y, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_fwd_t<bf16_t>(CB16(x), B16(y), B, H, W, C, OH, OW, s); }
extern "C" int wsmg_maxpool3x3s2_fwd_idx_bf16(const void* x, void* y, uint32_t* idx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_fwd_idx_t<bf16_t>(CB16(x), B16(y), idx, B, H, W, C, OH, OW, s); }
extern "C" int wsmg_maxpool3x3s2_bwd_idx_bf16(const void* dy, const uint32_t* idx, void* dx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_bwd_idx_t<bf16_t>(CB16(dy), idx, B16(dx), B, H, W, C, OH, OW, s); }
extern "C" int wsmg_maxpool3x3s2_bwd(const float* dy, const float* x, float* dx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_bwd_t<float>(dy, x, dx, B, H, W, C, OH, OW, s); }
extern "C" int wsmg_maxpool3x3s2_bwd_bf16(const void* dy, const void* x, void* dx, int B, int H, int W, int C, int OH, int OW, wsmg_stream_t s) { return maxpool_bwd_t<bf16_t>(CB16(dy), CB16(x), B16(dx), B, H, W, C, OH, OW, s); }
extern "C" int wsmg_upsample2x_fwd(const float* x, float* y, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_fwd_t<float>(x, y, B, H, W, C, s); }
extern "C" int wsmg_upsample2x_fwd_bf16(const void* x, void* y, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_fwd_t<bf16_t>(CB16(x), B16(y), B, H, W, C, s); }
extern "C" int wsmg_upsample2x_bwd(const float* dy, float* dx, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_bwd_t<float>(dy, dx, B, H, W, C, s); }
extern "C" int wsmg_upsample2x_bwd_bf16(const void* dy, void* dx, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_bwd_t<bf16_t>(CB16(dy), B16(dx), B, H, W, C, s); }
extern "C" int wsmg_upsample2x_bwd_ld(const float* dy, int64_t ld_dy, float* dx, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_bwd_t<float>(dy, dx, B, H, W, C, s, ld_dy); }
extern "C" int wsmg_upsample2x_bwd_ld_bf16(const void* dy, int64_t ld_dy, void* dx, int B, int H, int W, int C, wsmg_stream_t s) { return upsample_bwd_t<bf16_t>(CB16(dy), B16(dx), B, H, W, C, s, ld_dy); }
extern "C" int wsmg_avgpool2_fwd(const float* x, float* y, int B, int H, int W, int C, wsmg_stream_t s) { return avgpool_fwd_t<float>(x, y, B, H, W, C, s); }
extern "C" int wsmg_avgpool2_fwd_bf16(const void* x, void* y, int B, int H, int W, int C, wsmg_stream_t s) { return avgpool_fwd_t<bf16_t>(CB16(x), B16(y), B, H, W, C, s); }
extern "C" int wsmg_avgpool2_bwd(const float* dy, float* dx, int B, int H, int W, int C, wsmg_stream_t s) { return avgpool_bwd_t<float>(dy, dx, B, H, W, C, s); }
extern "C" int wsmg_avgpool2_bwd_bf16(const void* dy, void* dx, int B, int H, int W, int C, wsmg_stream_t s) { return avgpool_bwd_t<bf16_t>(CB16(dy), B16(dx), B, H, W, C, s); }
