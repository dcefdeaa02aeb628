// BatchNorm2d (+residual, +ReLU) forward/backward and per-channel column sums for NHWC
// float32 or bf16 activations viewed as a [rows][C] matrix (rows = B*H*W, C in {32,64,128,256,512}: chan_ok).
//
// Replaces nn.BatchNorm2d / F.relu (cuDNN batch-norm + elementwise kernels) at
// map_encoder.py:10-12,21-28,94-112, mg_map_policy.py:80-85 and the torchvision BasicBlock
// tail (relu(bn2(conv2) + identity)).  Train-mode BN couples the whole T*N batch, so it is a
// two-pass structure: (1) a chip-wide column reduction in float64 partials, (2) a streaming
// normalise pass.  HBM-bound: pass 1 reads x once, pass 2 reads x (+res) and writes y.
#include <stdlib.h>

#include <type_traits>

#include "wsmg_common.h"

namespace {

constexpr int RED_THREADS = 256;
constexpr int RED_MAX_BLOCKS = 1024;

__host__ __device__ inline int red_blocks(int64_t rows, int C) {
  int rows_per_iter = RED_THREADS / (C / 4);
  int64_t nb = (rows + (int64_t)rows_per_iter * 8 - 1) / ((int64_t)rows_per_iter * 8);
  if (nb < 1) nb = 1;
  if (nb > RED_MAX_BLOCKS) nb = RED_MAX_BLOCKS;
  return (int)nb;
}

// Column reductions over a [rows][C] matrix; each thread owns 4 adjacent channels (one 8/16-B load
// per tensor and row) and walks rows with a grid stride; float64 accumulation.
// MODE 0: sum(x)                      -> part[blk][0][c]
// MODE 1: sum(x), sum(x*x)            -> part[blk][0..1][c]
// MODE 2: sum(g), sum(g*xhat)  with g = dy * (relu ? y > 0 : 1), xhat = (x-mean)*invstd
template <int MODE, class T>
__global__ __launch_bounds__(RED_THREADS) void col_reduce_kernel(const T* __restrict__ x,
                                                                 const T* __restrict__ dy,
                                                                 const T* __restrict__ y,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, int relu,
                                                                 int64_t rows, int C, double* __restrict__ part,
                                                                 int64_t ld_dy = 0) {   // row stride of dy (0: C)
  __shared__ double sh[2][4][RED_THREADS];
  const int64_t ldg = ld_dy ? ld_dy : C;
  const int tid = threadIdx.x;
  const int C4 = C >> 2;
  const int c = (tid % C4) * 4;
  const int rl = tid / C4;
  const int rpi = RED_THREADS / C4;
  double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0};
  f32x4 mu = {0.f, 0.f, 0.f, 0.f}, is = {1.f, 1.f, 1.f, 1.f};
  f32x4 gm = {1.f, 1.f, 1.f, 1.f}, bt = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 2) {
    mu = *reinterpret_cast<const f32x4*>(mean + c); is = *reinterpret_cast<const f32x4*>(invstd + c);
    if (relu && !y) { gm = *reinterpret_cast<const f32x4*>(gamma + c); bt = *reinterpret_cast<const f32x4*>(beta + c); }
  }
  // four rows in flight per thread (the plain grid-stride loop compiled to ONE 8-byte load per thread and trip: 3.1-3.9
  // TB/s): the loads of a trip are issued together, then accumulated
  auto accumulate = [&](const f32x4& xv, f32x4 g, const f32x4& yv) {
    if (MODE == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s0[j] += (double)xv[j];
    } else if (MODE == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { s0[j] += (double)xv[j]; s1[j] += (double)xv[j] * (double)xv[j]; }
    } else {
      if (relu) {
        if (y) {
#pragma unroll
          for (int j = 0; j < 4; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
        } else {   // no residual: the forward value is recomputed (same expression as bn_apply_kernel) instead of read
#pragma unroll
          for (int j = 0; j < 4; ++j) g[j] = ((xv[j] - mu[j]) * is[j] * gm[j] + bt[j]) > 0.f ? g[j] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float xh = (xv[j] - mu[j]) * is[j];
        s0[j] += (double)g[j];
        s1[j] += (double)g[j] * (double)xh;
      }
    }
  };
  const int64_t S = (int64_t)gridDim.x * rpi;
  int64_t r = (int64_t)blockIdx.x * rpi + rl;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (; r + 3 * S < rows; r += 4 * S) {
    f32x4 xa[4], ga[4], ya[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t o = (size_t)(r + u * S) * C + c;
      xa[u] = ld4(x + o);
      ga[u] = MODE == 2 ? ld4(dy + (size_t)(r + u * S) * ldg + c) : zero4;
      ya[u] = (MODE == 2 && relu && y) ? ld4(y + o) : zero4;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) accumulate(xa[u], ga[u], ya[u]);
  }
  for (; r < rows; r += S) {
    const size_t o = (size_t)r * C + c;
    accumulate(ld4(x + o), MODE == 2 ? ld4(dy + (size_t)r * ldg + c) : zero4, (MODE == 2 && relu && y) ? ld4(y + o) : zero4);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { sh[0][j][tid] = s0[j]; sh[1][j][tid] = s1[j]; }
  __syncthreads();
  if (rl == 0) {
    for (int k = 1; k < rpi; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) { s0[j] += sh[0][j][k * C4 + tid]; s1[j] += sh[1][j][k * C4 + tid]; }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      part[((size_t)blockIdx.x * 2 + 0) * C + c + j] = s0[j];
      part[((size_t)blockIdx.x * 2 + 1) * C + c + j] = s1[j];
    }
  }
}

// finalize kernels: one wave per channel sums the per-block float64 partials (lane-strided, then
// a shuffle reduction) — a few microseconds instead of a 1024-iteration serial loop.
__device__ __forceinline__ void reduce_partials(const double* part, int nblk, int C, int c, double& s, double& q) {
  // four independent lane-strided loads per trip (the one-pair-per-trip loop waited out an L2 round trip 16 times for
  // 1024 partials: 7.5 us per finalize launch, 32 launches per update)
  double sv[4] = {0.0, 0.0, 0.0, 0.0}, qv[4] = {0.0, 0.0, 0.0, 0.0};
  int b = threadIdx.x;
  for (; b + 3 * WSMG_WAVE < nblk; b += 4 * WSMG_WAVE) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sv[j] += part[((size_t)(b + j * WSMG_WAVE) * 2 + 0) * C + c];
      qv[j] += part[((size_t)(b + j * WSMG_WAVE) * 2 + 1) * C + c];
    }
  }
  for (; b < nblk; b += WSMG_WAVE) {
    sv[0] += part[((size_t)b * 2 + 0) * C + c];
    qv[0] += part[((size_t)b * 2 + 1) * C + c];
  }
  s = wave_sum_d((sv[0] + sv[1]) + (sv[2] + sv[3]));
  q = wave_sum_d((qv[0] + qv[1]) + (qv[2] + qv[3]));
}

__global__ __launch_bounds__(64) void sum_finalize_kernel(const double* part, int nblk, int C, float* out) {
  const int c = blockIdx.x;
  double s, q;
  reduce_partials(part, nblk, C, c, s, q);
  if (threadIdx.x == 0) out[c] = (float)s;
}

__global__ __launch_bounds__(64) void bn_stats_finalize_kernel(double* part, int nblk, int C, int64_t rows,
                                                               float momentum, float eps, float* running_mean,
                                                               float* running_var, float* save_mean,
                                                               float* save_invstd, int clear) {
  const int c = blockIdx.x;
  double s, q;
  reduce_partials(part, nblk, C, c, s, q);
  if (clear)   // slabs filled by a convolution's epilogue: hand them back zeroed for the next forward pass
    for (int b = threadIdx.x; b < nblk; b += WSMG_WAVE) { part[((size_t)b * 2 + 0) * C + c] = 0.0; part[((size_t)b * 2 + 1) * C + c] = 0.0; }
  if (threadIdx.x != 0) return;
  double n = (double)rows;
  double mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0.0) var = 0.0;
  save_mean[c] = (float)mean;
  save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    double unb = rows > 1 ? var * n / (n - 1.0) : var;
    running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
    running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unb);
  }
}

__global__ void bn_eval_prepare_kernel(const float* running_mean, const float* running_var, float eps, int C,
                                       float* save_mean, float* save_invstd) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  save_mean[c] = running_mean[c];
  save_invstd[c] = 1.0f / sqrtf(running_var[c] + eps);
}

// y = act((x - mean) * invstd * gamma + beta (+ res)).  Each thread owns ONE channel quad for the
// whole launch (per-channel constants live in registers) and walks rows with a grid stride.
template <class T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ beta,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, int relu, int64_t rows,
                                                       int C, T* __restrict__ y) {
  const int C4 = C >> 2;
  const int c = (threadIdx.x % C4) * 4;
  const int rl = threadIdx.x / C4;
  const int rpi = 256 / C4;
  const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
  const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
  const f32x4 m = *reinterpret_cast<const f32x4*>(mean + c);
  const f32x4 s = *reinterpret_cast<const f32x4*>(invstd + c);
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const size_t o = (size_t)r * C + c;
    f32x4 v = ld4(x + o);
    f32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = (v[j] - m[j]) * s[j] * g[j] + b[j];
    if (res) {
      f32x4 rr = ld4(res + o);
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] += rr[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 4; ++j) out[j] = out[j] > 0.f ? out[j] : 0.f;
    }
    st4(y + o, out);
  }
}

// dgamma/dbeta from the reduction, then dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n)
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(const double* part, int nblk, int C, float* dgamma,
                                                             float* dbeta) {
  const int c = blockIdx.x;
  double s, q;
  reduce_partials(part, nblk, C, c, s, q);
  if (threadIdx.x == 0) {
    dbeta[c] = (float)s;
    dgamma[c] = (float)q;
  }
}

// dx = gamma*invstd*(g - dbeta/n - xhat*dgamma/n), g = dy masked by the ReLU; fixed channel quad per thread
template <class T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                           const T* __restrict__ y,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, int relu, float inv_n,
                                                           int64_t rows, int C, T* __restrict__ dx,
                                                           T* __restrict__ dres, int64_t ld_dy) {
  const int C4 = C >> 2;
  const int c = (threadIdx.x % C4) * 4;
  const int rl = threadIdx.x / C4;
  const int rpi = 256 / C4;
  const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c);
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
  const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
  const f32x4 dg = *reinterpret_cast<const f32x4*>(dgamma + c);
  const f32x4 db = *reinterpret_cast<const f32x4*>(dbeta + c);
  f32x4 bt = {0.f, 0.f, 0.f, 0.f};
  if (relu && !y) bt = *reinterpret_cast<const f32x4*>(beta + c);
  f32x4 k0, k1, k2;  // dx = k0 * (g - k1 - xhat * k2)
#pragma unroll
  for (int j = 0; j < 4; ++j) { k0[j] = gm[j] * is[j]; k1[j] = db[j] * inv_n; k2[j] = dg[j] * inv_n; }
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const size_t o = (size_t)r * C + c;
    f32x4 g = ld4(dy + (size_t)r * ld_dy + c);
    f32x4 xv = ld4(x + o);
    if (relu) {
      if (y) {
        f32x4 yv = ld4(y + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = ((xv[j] - mu[j]) * is[j] * gm[j] + bt[j]) > 0.f ? g[j] : 0.f;
      }
    }
    if (dres) st4(dres + o, g);
    f32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xh = (xv[j] - mu[j]) * is[j];
      out[j] = k0[j] * (g[j] - k1[j] - xh * k2[j]);
    }
    st4(dx + o, out);
  }
}

// ---- bf16 activations: 8 channels (one 16-byte access) per thread instead of 4 (8 bytes)
typedef unsigned int u32x4n __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void unpack8(const u32x4n raw, f32x4& lo, f32x4& hi) {
  lo[0] = __uint_as_float(raw[0] << 16); lo[1] = __uint_as_float(raw[0] & 0xffff0000u);
  lo[2] = __uint_as_float(raw[1] << 16); lo[3] = __uint_as_float(raw[1] & 0xffff0000u);
  hi[0] = __uint_as_float(raw[2] << 16); hi[1] = __uint_as_float(raw[2] & 0xffff0000u);
  hi[2] = __uint_as_float(raw[3] << 16); hi[3] = __uint_as_float(raw[3] & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
  bf16_t x = (bf16_t)a, y = (bf16_t)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ u32x4n pack8(const f32x4& lo, const f32x4& hi) {
  u32x4n r = {pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
  return r;
}

__global__ __launch_bounds__(256) void bn_apply8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        int relu, int64_t rows, int C, bf16_t* __restrict__ y) {
  const int C8 = C >> 3;
  const int c = (threadIdx.x % C8) * 8;
  const int rl = threadIdx.x / C8;
  const int rpi = 256 / C8;
  f32x4 g[2], b[2], m[2], s[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    g[k] = *reinterpret_cast<const f32x4*>(gamma + c + 4 * k); b[k] = *reinterpret_cast<const f32x4*>(beta + c + 4 * k);
    m[k] = *reinterpret_cast<const f32x4*>(mean + c + 4 * k);  s[k] = *reinterpret_cast<const f32x4*>(invstd + c + 4 * k);
  }
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const size_t o = (size_t)r * C + c;
    f32x4 v[2], rr[2], out[2];
    unpack8(*reinterpret_cast<const u32x4n*>(x + o), v[0], v[1]);
    if (res) unpack8(*reinterpret_cast<const u32x4n*>(res + o), rr[0], rr[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = (v[k][j] - m[k][j]) * s[k][j] * g[k][j] + b[k][j];
        if (res) t += rr[k][j];
        if (relu) t = t > 0.f ? t : 0.f;
        out[k][j] = t;
      }
    *reinterpret_cast<u32x4n*>(y + o) = pack8(out[0], out[1]);
  }
}

__global__ __launch_bounds__(256) void bn_bwd_apply8_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                            const bf16_t* __restrict__ y, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ dgamma,
                                                            const float* __restrict__ dbeta, int relu, float inv_n, int64_t rows,
                                                            int C, bf16_t* __restrict__ dx, bf16_t* __restrict__ dres,
                                                            int64_t ld_dy, bf16_t* __restrict__ dx_lo = nullptr) {
  const int C8 = C >> 3;
  const int c = (threadIdx.x % C8) * 8;
  const int rl = threadIdx.x / C8;
  const int rpi = 256 / C8;
  f32x4 gm[2], mu[2], is[2], bt[2], k0[2], k1[2], k2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    gm[k] = *reinterpret_cast<const f32x4*>(gamma + c + 4 * k);
    mu[k] = *reinterpret_cast<const f32x4*>(mean + c + 4 * k);
    is[k] = *reinterpret_cast<const f32x4*>(invstd + c + 4 * k);
    const f32x4 dg = *reinterpret_cast<const f32x4*>(dgamma + c + 4 * k), db = *reinterpret_cast<const f32x4*>(dbeta + c + 4 * k);
    bt[k] = (relu && !y) ? *reinterpret_cast<const f32x4*>(beta + c + 4 * k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) { k0[k][j] = gm[k][j] * is[k][j]; k1[k][j] = db[j] * inv_n; k2[k][j] = dg[j] * inv_n; }
  }
  for (int64_t r = (int64_t)blockIdx.x * rpi + rl; r < rows; r += (int64_t)gridDim.x * rpi) {
    const size_t o = (size_t)r * C + c;
    f32x4 g[2], xv[2], yv[2], out[2];
    unpack8(*reinterpret_cast<const u32x4n*>(dy + (size_t)r * ld_dy + c), g[0], g[1]);
    unpack8(*reinterpret_cast<const u32x4n*>(x + o), xv[0], xv[1]);
    if (relu && y) unpack8(*reinterpret_cast<const u32x4n*>(y + o), yv[0], yv[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (relu) {
          const bool on = y ? yv[k][j] > 0.f : ((xv[k][j] - mu[k][j]) * is[k][j] * gm[k][j] + bt[k][j]) > 0.f;
          g[k][j] = on ? g[k][j] : 0.f;
        }
        const float xh = (xv[k][j] - mu[k][j]) * is[k][j];
        out[k][j] = k0[k][j] * (g[k][j] - k1[k][j] - xh * k2[k][j]);
      }
    if (dres) *reinterpret_cast<u32x4n*>(dres + o) = pack8(g[0], g[1]);
    const u32x4n hi = pack8(out[0], out[1]);
    *reinterpret_cast<u32x4n*>(dx + o) = hi;
    if (dx_lo) {      // the part of the float32 gradient its bf16 rounding dropped, itself in bf16: dx ~= hi + lo to 16 mantissa bits
      f32x4 h0, h1, l0, l1;
      unpack8(hi, h0, h1);
#pragma unroll
      for (int j = 0; j < 4; ++j) { l0[j] = out[0][j] - h0[j]; l1[j] = out[1][j] - h1[j]; }
      *reinterpret_cast<u32x4n*>(dx_lo + o) = pack8(l0, l1);
    }
  }
}

// bf16 always takes the 8-channel kernels (chan_ok: every channel count is a multiple of 32); the 4-channel templates are compiled
// for float32 only

int stream_grid8(int64_t rows, int C) {
  int64_t rpi = 256 / (C / 8);
  int64_t g = wsmg_cdiv(rows, rpi * 4);
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

bool chan_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256 || C == 512; }

int stream_grid(int64_t rows, int C) {
  int64_t rpi = 256 / (C / 4);
  int64_t g = wsmg_cdiv(rows, rpi * 4);   // >= 4 rows per thread
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

template <class T>
int channel_sum_t(const T* x, int64_t rows, int C, float* out, double* workspace, int64_t workspace_bytes,
                  wsmg_stream_t stream) {
  if (!chan_ok(C) || rows <= 0) return WSMG_EINVAL;
  if (workspace_bytes < wsmg_channel_reduce_workspace_bytes(rows, C)) return WSMG_ENOMEM;
  int nb = red_blocks(rows, C);
  hipLaunchKernelGGL((col_reduce_kernel<0, T>), dim3(nb), dim3(RED_THREADS), 0, wsmg_s(stream), x, (const T*)nullptr,
                     (const T*)nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, workspace);
  hipLaunchKernelGGL(sum_finalize_kernel, dim3(C), dim3(64), 0, wsmg_s(stream), workspace, nb, C, out);
  WSMG_RETURN_LAUNCH();
}

template <class T>
int bn_act_fwd_t(const T* x, const T* residual, const float* gamma, const float* beta, float* running_mean,
                 float* running_var, float momentum, float eps, int train, int relu, int64_t rows, int C, T* y,
                 float* save_mean, float* save_invstd, double* workspace, int64_t workspace_bytes,
                 wsmg_stream_t stream) {
  if (!chan_ok(C) || rows <= 0) return WSMG_EINVAL;
  hipStream_t s = wsmg_s(stream);
  if (train) {
    if (workspace_bytes < wsmg_channel_reduce_workspace_bytes(rows, C)) return WSMG_ENOMEM;
    int nb = red_blocks(rows, C);
    hipLaunchKernelGGL((col_reduce_kernel<1, T>), dim3(nb), dim3(RED_THREADS), 0, s, x, (const T*)nullptr,
                       (const T*)nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, workspace);
    hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, s, workspace, nb, C, rows, momentum, eps,
                       running_mean, running_var, save_mean, save_invstd, 0);
  } else {
    hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3((unsigned)wsmg_cdiv(C, 256)), dim3(256), 0, s, running_mean, running_var, eps, C,
                       save_mean, save_invstd);
  }
  if constexpr (std::is_same<T, bf16_t>::value) {
    hipLaunchKernelGGL(bn_apply8_kernel, dim3(stream_grid8(rows, C)), dim3(256), 0, s, x, residual, gamma, beta, save_mean,
                       save_invstd, relu, rows, C, y);
  } else {
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(stream_grid(rows, C)), dim3(256), 0, s, x, residual, gamma, beta,
                       save_mean, save_invstd, relu, rows, C, y);
  }
  WSMG_RETURN_LAUNCH();
}

template <class T>
int bn_act_bwd_t(const T* dy, const T* x, const T* y, const float* gamma, const float* beta, const float* save_mean,
                 const float* save_invstd, int relu, int64_t rows, int C, T* dx, T* dresidual, float* dgamma,
                 float* dbeta, double* workspace, int64_t workspace_bytes, wsmg_stream_t stream, int64_t ld_dy = 0, T* dx_lo = nullptr) {
  if (!chan_ok(C) || rows <= 0) return WSMG_EINVAL;
  if (ld_dy == 0) ld_dy = C;
  if (ld_dy < C || (ld_dy & 7) || ((uintptr_t)dy & 15)) return WSMG_EINVAL;
  if (relu && !y && (!beta || dresidual)) return WSMG_EINVAL;   // the mask can only be recomputed without a residual
  if (workspace_bytes < wsmg_channel_reduce_workspace_bytes(rows, C)) return WSMG_ENOMEM;
  hipStream_t s = wsmg_s(stream);
  int nb = red_blocks(rows, C);
  hipLaunchKernelGGL((col_reduce_kernel<2, T>), dim3(nb), dim3(RED_THREADS), 0, s, x, dy, y, save_mean, save_invstd,
                     gamma, beta, relu, rows, C, workspace, ld_dy);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, s, workspace, nb, C, dgamma, dbeta);
  if constexpr (std::is_same<T, bf16_t>::value) {
    hipLaunchKernelGGL(bn_bwd_apply8_kernel, dim3(stream_grid8(rows, C)), dim3(256), 0, s, dy, x, y, gamma, beta, save_mean,
                       save_invstd, dgamma, dbeta, relu, 1.0f / (float)rows, rows, C, dx, dresidual, ld_dy, dx_lo);
  } else {
    if (dx_lo) return WSMG_EINVAL;
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(stream_grid(rows, C)), dim3(256), 0, s, dy, x, y, gamma, beta, save_mean,
                       save_invstd, dgamma, dbeta, relu, 1.0f / (float)rows, rows, C, dx, dresidual, ld_dy);
  }
  WSMG_RETURN_LAUNCH();
}

}  // namespace

// BatchNorm (train) + residual + ReLU of a bf16 tensor whose per-channel sums were already accumulated by the producing
// convolution's epilogue (wsmg_conv2d_fwd_bf16_stats): finalize (+ clear the slabs) and apply — no statistics pass over x.
extern "C" int wsmg_bn_act_fwd_bf16_pre(const void* x, const void* residual, const float* gamma, const float* beta,
                                        float* running_mean, float* running_var, float momentum, float eps, int relu,
                                        int64_t rows, int C, void* y, float* save_mean, float* save_invstd, double* stats,
                                        int nslab, wsmg_stream_t stream) {
  if (!chan_ok(C) || rows <= 0 || !stats || nslab <= 0) return WSMG_EINVAL;
  hipStream_t s = wsmg_s(stream);
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, s, stats, nslab, C, rows, momentum, eps, running_mean,
                     running_var, save_mean, save_invstd, 1);
  hipLaunchKernelGGL(bn_apply8_kernel, dim3(stream_grid8(rows, C)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)residual, gamma,
                     beta, save_mean, save_invstd, relu, rows, C, (bf16_t*)y);
  WSMG_RETURN_LAUNCH();
}

// The two halves of wsmg_bn_act_fwd_bf16_pre / wsmg_bn_act_bwd_bf16 on their own, for callers that fuse the other half into a
// kernel of theirs (csrc/wsmg_cls_tail.hip): (1) batch statistics from the slabs a convolution's epilogue filled -> mean, 1 / sqrt(
// var + eps), running statistics; the slabs are handed back zeroed.  (2) dx = gamma invstd (dy - dbeta / n - xhat dgamma / n) for a
// dy that is ALREADY masked by the ReLU and whose two per-channel sums (dbeta = sum dy, dgamma = sum dy xhat) the caller supplies.
extern "C" int wsmg_bn_stats_finalize(double* stats, int nslab, int C, int64_t rows, float momentum, float eps, float* running_mean,
                                      float* running_var, float* save_mean, float* save_invstd, wsmg_stream_t stream) {
  if (!chan_ok(C) || rows <= 0 || !stats || nslab <= 0 || !save_mean || !save_invstd) return WSMG_EINVAL;
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, wsmg_s(stream), stats, nslab, C, rows, momentum, eps, running_mean,
                     running_var, save_mean, save_invstd, 1);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_bn_bwd_apply_bf16(const void* dy, const void* x, const float* gamma, const float* mean, const float* invstd,
                                      const float* dgamma, const float* dbeta, int64_t rows, int C, void* dx, wsmg_stream_t stream) {
  if (!chan_ok(C) || (C & 7) || rows <= 0 || !dy || !x || !gamma || !mean || !invstd || !dgamma || !dbeta || !dx) return WSMG_EINVAL;
  hipLaunchKernelGGL(bn_bwd_apply8_kernel, dim3(stream_grid8(rows, C)), dim3(256), 0, wsmg_s(stream), (const bf16_t*)dy, (const bf16_t*)x,
                     (const bf16_t*)nullptr, gamma, (const float*)nullptr, mean, invstd, dgamma, dbeta, 0, 1.0f / (float)rows, rows, C,
                     (bf16_t*)dx, (bf16_t*)nullptr, (int64_t)C);
  WSMG_RETURN_LAUNCH();
}

extern "C" int64_t wsmg_channel_reduce_workspace_bytes(int64_t rows, int C) {
  if (!chan_ok(C)) return 0;
  return (int64_t)red_blocks(rows, C) * 2 * C * (int64_t)sizeof(double);
}

extern "C" int wsmg_channel_sum(const float* x, int64_t rows, int C, float* out, double* workspace,
                                int64_t workspace_bytes, wsmg_stream_t stream) {
  return channel_sum_t<float>(x, rows, C, out, workspace, workspace_bytes, stream);
}
extern "C" int wsmg_channel_sum_bf16(const void* x, int64_t rows, int C, float* out, double* workspace,
                                     int64_t workspace_bytes, wsmg_stream_t stream) {
  return channel_sum_t<bf16_t>((const bf16_t*)x, rows, C, out, workspace, workspace_bytes, stream);
}

extern "C" int wsmg_bn_act_fwd(const float* x, const float* residual, const float* gamma, const float* beta,
                               float* running_mean, float* running_var, float momentum, float eps, int train,
                               int relu, int64_t rows, int C, float* y, float* save_mean, float* save_invstd,
                               double* workspace, int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_fwd_t<float>(x, residual, gamma, beta, running_mean, running_var, momentum, eps, train, relu, rows, C, y,
                             save_mean, save_invstd, workspace, workspace_bytes, stream);
}
extern "C" int wsmg_bn_act_fwd_bf16(const void* x, const void* residual, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, int train,
                                    int relu, int64_t rows, int C, void* y, float* save_mean, float* save_invstd,
                                    double* workspace, int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_fwd_t<bf16_t>((const bf16_t*)x, (const bf16_t*)residual, gamma, beta, running_mean, running_var, momentum,
                              eps, train, relu, rows, C, (bf16_t*)y, save_mean, save_invstd, workspace, workspace_bytes,
                              stream);
}

extern "C" int wsmg_bn_act_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C,
                               float* dx, float* dresidual, float* dgamma, float* dbeta, double* workspace,
                               int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_bwd_t<float>(dy, x, y, gamma, beta, save_mean, save_invstd, relu, rows, C, dx, dresidual, dgamma, dbeta,
                             workspace, workspace_bytes, stream);
}
extern "C" int wsmg_bn_act_bwd_bf16(const void* dy, const void* x, const void* y, const float* gamma, const float* beta,
                                    const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C,
                                    void* dx, void* dresidual, float* dgamma, float* dbeta, double* workspace,
                                    int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_bwd_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)y, gamma, beta, save_mean, save_invstd, relu,
                              rows, C, (bf16_t*)dx, (bf16_t*)dresidual, dgamma, dbeta, workspace, workspace_bytes, stream);
}

// dy with a row stride (`ld_dy` elements, a multiple of 8, >= C): the channel slice of a concatenation's gradient is read in
// place (the decoders' `torch.cat(..., dim=1)` of map_encoder.py:104,110: autograd hands the two halves back as views)
extern "C" int wsmg_bn_act_bwd_ld(const float* dy, int64_t ld_dy, const float* x, const float* y, const float* gamma, const float* beta,
                                  const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C, float* dx,
                                  float* dresidual, float* dgamma, float* dbeta, double* workspace, int64_t workspace_bytes,
                                  wsmg_stream_t stream) {
  return bn_act_bwd_t<float>(dy, x, y, gamma, beta, save_mean, save_invstd, relu, rows, C, dx, dresidual, dgamma, dbeta,
                             workspace, workspace_bytes, stream, ld_dy);
}
extern "C" int wsmg_bn_act_bwd_ld_bf16(const void* dy, int64_t ld_dy, const void* x, const void* y, const float* gamma,
                                       const float* beta, const float* save_mean, const float* save_invstd, int relu, int64_t rows,
                                       int C, void* dx, void* dresidual, float* dgamma, float* dbeta, double* workspace,
                                       int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_bwd_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)y, gamma, beta, save_mean, save_invstd, relu,
                              rows, C, (bf16_t*)dx, (bf16_t*)dresidual, dgamma, dbeta, workspace, workspace_bytes, stream, ld_dy);
}

// Round 6, COMPUTE_DTYPE = "bf16+f32grad" (VERDICT r05 item 8): wsmg_bn_act_bwd_ld_bf16 that also writes dx_lo = bf16(dx_f32 - bf16(dx_f32)),
// the part of the float32 input gradient its bf16 rounding dropped; the layer's weight gradient is then taken from (dx, dx_lo) — two
// launches of the bf16 weight-gradient kernel — i.e. from a 16-mantissa-bit dY.  The reference trains in float32 only
// (dagger_trainer.py:505-541).
extern "C" int wsmg_bn_act_bwd_ld_bf16_lo(const void* dy, int64_t ld_dy, const void* x, const void* y, const float* gamma, const float* beta,
                                          const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C, void* dx,
                                          void* dx_lo, void* dresidual, float* dgamma, float* dbeta, double* workspace,
                                          int64_t workspace_bytes, wsmg_stream_t stream) {
  if (!dx_lo || (C & 7)) return WSMG_EINVAL;
  return bn_act_bwd_t<bf16_t>((const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)y, gamma, beta, save_mean, save_invstd, relu,
                              rows, C, (bf16_t*)dx, (bf16_t*)dresidual, dgamma, dbeta, workspace, workspace_bytes, stream, ld_dy,
                              (bf16_t*)dx_lo);
}

// ----------------------------------------------------------------------------- GroupNorm (frozen DD-PPO depth ResNet50)
// nn.GroupNorm over NHWC bf16 activations, inference only: statistics per (sample, group) over H x W x C/G elements
// (biased variance, eps under the root), then gamma / beta per channel, optional residual add, optional ReLU.
// habitat-lab v0.1.5 resnet.py uses it after every convolution of the depth backbone (reference call site
// vlnce_baselines/models/encoders/resnet_encoders.py:25-32).  One workgroup per (group, sample); the whole path is 0.7 GFLOP
// and a few MB per frame, so the kernel is written for generality (any C/G >= 1), not for the last GB/s: two passes over
// the group's H*W*Cg elements, float accumulation per thread, float64 across the workgroup.
namespace {
template <class TI>
__global__ __launch_bounds__(256) void group_norm_nhwc_bf16_kernel(const TI* __restrict__ x, const bf16_t* __restrict__ res,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   int HW, int C, int G, float eps, int relu, bf16_t* __restrict__ y) {
  __shared__ double red[2][4];
  __shared__ float stat[2];
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cg = C / G;
  const int n = HW * Cg;
  const size_t base = (size_t)b * HW * C + (size_t)g * Cg;
  float s = 0.f, ss = 0.f;
  for (int i = tid; i < n; i += 256) {
    const int p = i / Cg, c = i - p * Cg;
    const float v = (float)x[base + (size_t)p * C + c];
    s += v;
    ss = fmaf(v, v, ss);
  }
  double ds = wave_sum_d((double)s), dss = wave_sum_d((double)ss);
  if (lane == 0) { red[0][wave] = ds; red[1][wave] = dss; }
  __syncthreads();
  if (tid == 0) {
    const double t = red[0][0] + red[0][1] + red[0][2] + red[0][3], tt = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const double mean = t / n;
    double var = tt / n - mean * mean;
    if (var < 0) var = 0;
    stat[0] = (float)mean;
    stat[1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  const float mean = stat[0], inv = stat[1];
  for (int i = tid; i < n; i += 256) {
    const int p = i / Cg, c = i - p * Cg;
    const size_t o = base + (size_t)p * C + c;
    float v = ((float)x[o] - mean) * inv * gamma[g * Cg + c] + beta[g * Cg + c];
    if (res) v += (float)res[o];
    if (relu) v = v > 0.f ? v : 0.f;
    y[o] = (bf16_t)v;
  }
}
}  // namespace

extern "C" int wsmg_group_norm_nhwc_bf16(const void* x, int x_f32, const void* residual, const float* gamma, const float* beta,
                                         int B, int HW, int C, int G, float eps, int relu, void* y, wsmg_stream_t stream) {
  if (B <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G || B > 65535) return WSMG_EINVAL;
  if (x_f32)
    hipLaunchKernelGGL(group_norm_nhwc_bf16_kernel<float>, dim3(G, B), dim3(256), 0, wsmg_s(stream), (const float*)x,
                       (const bf16_t*)residual, gamma, beta, HW, C, G, eps, relu, (bf16_t*)y);
  else
    hipLaunchKernelGGL(group_norm_nhwc_bf16_kernel<bf16_t>, dim3(G, B), dim3(256), 0, wsmg_s(stream), (const bf16_t*)x,
                       (const bf16_t*)residual, gamma, beta, HW, C, G, eps, relu, (bf16_t*)y);
  WSMG_RETURN_LAUNCH();
}
