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

// The BatchNorm element, float32: the forward value before residual and ReLU, xhat, the ReLU gate of the backward, and dx.  The
// rule they exist for: without a residual y is not kept, and the backward (col_reduce_kernel<2>, bn_bwd_apply_kernel) opens the gate
// on the forward value it recomputes — right only if that value rounds exactly as the forward's did.  So there is one bn_value, and
// its form is spelled out instead of left to the compiler's contraction: (x - mean) invstd rounded twice, times gamma plus beta fused.
__device__ __forceinline__ float bn_xhat(float x, float mean, float invstd) { return (x - mean) * invstd; }
__device__ __forceinline__ float bn_value(float x, float mean, float invstd, float gamma, float beta) {
  return __fmaf_rn(bn_xhat(x, mean, invstd), gamma, beta);
}
// kept: y was stored (a residual went into it) and decides; otherwise the recomputed forward value does
__device__ __forceinline__ bool bn_gate(bool kept, float y, float x, float mean, float invstd, float gamma, float beta) {
  return (kept ? y : bn_value(x, mean, invstd, gamma, beta)) > 0.f;
}
// dx = k0 (g - k1 - xhat k2) with k0 = gamma invstd, k1 = dbeta / n, k2 = dgamma / n and g = dy behind the gate
__device__ __forceinline__ float bn_dx(float g, float xhat, float k0, float k1, float k2) { return k0 * __fmaf_rn(-xhat, k2, g - k1); }

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
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = bn_gate(y != nullptr, yv[j], xv[j], mu[j], is[j], gm[j], bt[j]) ? g[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s0[j] += (double)g[j];
        s1[j] += (double)g[j] * (double)bn_xhat(xv[j], mu[j], is[j]);
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

// the plain sums: out0[c] = the first partial's sum (channel sum; dbeta), and for TWO out1[c] = the second's (dgamma).  TWO is a
// template argument, not a null test: without it the compiler drops the loads of the second partial, which a run-time test keeps for
// the channel sums too (4.0-4.9 -> 5.5-5.9 us per launch over the update's shapes, profiles/norm_once.txt section 3)
template <bool TWO>
__global__ __launch_bounds__(64) void sum_finalize_kernel(const double* part, int nblk, int C, float* out0, float* out1) {
  const int c = blockIdx.x;
  double s, q;
  reduce_partials(part, nblk, C, c, s, q);
  if (threadIdx.x == 0) {
    out0[c] = (float)s;
    if (TWO) out1[c] = (float)q;
  }
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

// The streaming kernels, 256 threads: a thread owns the same N adjacent channels c ... c + N - 1 for the whole launch (their
// per-channel constants live in registers) and takes rows r0, r0 + stride, ...  N = 4 for float32, 8 for bf16 (chan_ok: every
// channel count is a multiple of 32): one 16-byte access per tensor and row either way.  No other pair is compiled.  The forward
// apply is written on this walk; the two backward apply kernels below spell the same walk out (their comment says why).
struct RowWalk { int c; int64_t r0, stride; };
template <int N>
__device__ __forceinline__ RowWalk row_walk(int C) {
  const int CN = C / N, rpi = 256 / CN;
  return {(int)(threadIdx.x % CN) * N, (int64_t)blockIdx.x * rpi + threadIdx.x / CN, (int64_t)gridDim.x * rpi};
}
int stream_grid(int64_t rows, int C, int N) {
  int64_t rpi = 256 / (C / N);
  int64_t g = wsmg_cdiv(rows, rpi * 4);   // >= 4 rows per thread
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}
template <class T> constexpr int STREAM_N = std::is_same<T, bf16_t>::value ? 8 : 4;
template <int N>
__device__ __forceinline__ void ld_consts(const float* p, float (&o)[N]) {
#pragma unroll
  for (int k = 0; k < N; k += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[k + j] = v[j];
  }
}

// y = act(bn_value(x) (+ res))
template <class T, int N>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd, int relu,
                                                       int64_t rows, int C, T* __restrict__ y) {
  const RowWalk w = row_walk<N>(C);
  float g[N], b[N], m[N], s[N];
  ld_consts<N>(gamma + w.c, g); ld_consts<N>(beta + w.c, b); ld_consts<N>(mean + w.c, m); ld_consts<N>(invstd + w.c, s);
  for (int64_t r = w.r0; r < rows; r += w.stride) {
    const size_t o = (size_t)r * C + w.c;
    float v[N], rr[N], out[N];
    ld_chans<N>(x + o, v);
    if (res) ld_chans<N>(res + o, rr);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      float t = bn_value(v[j], m[j], s[j], g[j], b[j]);
      if (res) t += rr[j];
      if (relu) t = t > 0.f ? t : 0.f;
      out[j] = t;
    }
    st_chans<N>(y + o, out);
  }
}

// g = dy behind the ReLU's gate (-> dres), dx = bn_dx(g, xhat).  The backward keeps its two walks, 4 channels per thread (float32)
// and 8 (bf16, below), on the shared element functions: as one bn_bwd_apply_kernel<T, N> over float[N] the bf16 instance took 29.57 /
// 29.12 / 29.29 us per launch at the update's shapes where the parent's takes 28.81 / 28.75 / 28.96 and this one 28.75 / 28.58 /
// 28.61, runs alternating in one session (profiles/norm_once.txt).
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
        for (int j = 0; j < 4; ++j) g[j] = bn_gate(true, yv[j], xv[j], mu[j], is[j], gm[j], bt[j]) ? g[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = bn_gate(false, 0.f, xv[j], mu[j], is[j], gm[j], bt[j]) ? g[j] : 0.f;
      }
    }
    if (dres) st4(dres + o, g);
    f32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = bn_dx(g[j], bn_xhat(xv[j], mu[j], is[j]), k0[j], k1[j], k2[j]);
    st4(dx + o, out);
  }
}

// ---- bf16 activations: 8 channels (one 16-byte access) per thread instead of 4 (8 bytes).  16 bytes of bf16 as 8 floats is
// wsmg_common.h's chans_f32<8> / st_chans<8> everywhere else; this kernel keeps the f32x4[2] form and its own unpack8 / pack8 because
// that is the form that was timed: over float[8] through the shared helper (the one-template form of the comment above) it was the slower kernel
__device__ __forceinline__ void unpack8(const u32x4 raw, f32x4& lo, f32x4& hi) {
  lo[0] = __uint_as_float(raw[0] << 16); lo[1] = __uint_as_float(raw[0] & 0xffff0000u);
  lo[2] = __uint_as_float(raw[1] << 16); lo[3] = __uint_as_float(raw[1] & 0xffff0000u);
  hi[0] = __uint_as_float(raw[2] << 16); hi[1] = __uint_as_float(raw[2] & 0xffff0000u);
  hi[2] = __uint_as_float(raw[3] << 16); hi[3] = __uint_as_float(raw[3] & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
  bf16_t x = (bf16_t)a, y = (bf16_t)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ u32x4 pack8(const f32x4& lo, const f32x4& hi) {
  u32x4 r = {pack2(lo[0], lo[1]), pack2(lo[2], lo[3]), pack2(hi[0], hi[1]), pack2(hi[2], hi[3])};
  return r;
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
    unpack8(*reinterpret_cast<const u32x4*>(dy + (size_t)r * ld_dy + c), g[0], g[1]);
    unpack8(*reinterpret_cast<const u32x4*>(x + o), xv[0], xv[1]);
    if (relu && y) unpack8(*reinterpret_cast<const u32x4*>(y + o), yv[0], yv[1]);
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (relu) g[k][j] = bn_gate(y != nullptr, yv[k][j], xv[k][j], mu[k][j], is[k][j], gm[k][j], bt[k][j]) ? g[k][j] : 0.f;
        out[k][j] = bn_dx(g[k][j], bn_xhat(xv[k][j], mu[k][j], is[k][j]), k0[k][j], k1[k][j], k2[k][j]);
      }
    if (dres) *reinterpret_cast<u32x4*>(dres + o) = pack8(g[0], g[1]);
    const u32x4 hi = pack8(out[0], out[1]);
    *reinterpret_cast<u32x4*>(dx + o) = hi;
    if (dx_lo) {      // the part of the float32 gradient its bf16 rounding dropped, itself in bf16: dx ~= hi + lo to 16 mantissa bits
      f32x4 h0, h1, l0, l1;
      unpack8(hi, h0, h1);
#pragma unroll
      for (int j = 0; j < 4; ++j) { l0[j] = out[0][j] - h0[j]; l1[j] = out[1][j] - h1[j]; }
      *reinterpret_cast<u32x4*>(dx_lo + o) = pack8(l0, l1);
    }
  }
}

bool chan_ok(int C) { return C == 32 || C == 64 || C == 128 || C == 256 || C == 512; }

// What every entry point refuses first, before anything is queued: a channel count the kernels are not written for or no rows
// (WSMG_EINVAL) and, where the call reduces over rows, a workspace smaller than the reduction's partials (WSMG_ENOMEM).
int check_args(int64_t rows, int C, bool reduces = false, int64_t workspace_bytes = 0) {
  if (!chan_ok(C) || rows <= 0) return WSMG_EINVAL;
  if (reduces && workspace_bytes < wsmg_channel_reduce_workspace_bytes(rows, C)) return WSMG_ENOMEM;
  return 0;
}

// the three launches more than one entry point makes
void launch_stats_finalize(double* part, int nblk, int C, int64_t rows, float momentum, float eps, float* running_mean,
                           float* running_var, float* save_mean, float* save_invstd, int clear, hipStream_t s) {
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3(C), dim3(64), 0, s, part, nblk, C, rows, momentum, eps, running_mean, running_var,
                     save_mean, save_invstd, clear);
}
template <class T>
void launch_apply(const T* x, const T* residual, const float* gamma, const float* beta, const float* mean, const float* invstd,
                  int relu, int64_t rows, int C, T* y, hipStream_t s) {
  constexpr int N = STREAM_N<T>;
  hipLaunchKernelGGL((bn_apply_kernel<T, N>), dim3(stream_grid(rows, C, N)), dim3(256), 0, s, x, residual, gamma, beta, mean, invstd,
                     relu, rows, C, y);
}
template <class T>
void launch_bwd_apply(const T* dy, int64_t ld_dy, const T* x, const T* y, const float* gamma, const float* beta, const float* mean,
                      const float* invstd, const float* dgamma, const float* dbeta, int relu, int64_t rows, int C, T* dx, T* dresidual,
                      T* dx_lo, hipStream_t s) {
  const dim3 grid(stream_grid(rows, C, STREAM_N<T>));
  if constexpr (std::is_same<T, bf16_t>::value)
    hipLaunchKernelGGL(bn_bwd_apply8_kernel, grid, dim3(256), 0, s, dy, x, y, gamma, beta, mean, invstd, dgamma, dbeta, relu,
                       1.0f / (float)rows, rows, C, dx, dresidual, ld_dy, dx_lo);
  else    // dx_lo: refused by bn_act_bwd_t
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, grid, dim3(256), 0, s, dy, x, y, gamma, beta, mean, invstd, dgamma, dbeta, relu,
                       1.0f / (float)rows, rows, C, dx, dresidual, ld_dy);
}

template <class T>
int channel_sum_t(const T* x, int64_t rows, int C, float* out, double* workspace, int64_t workspace_bytes,
                  wsmg_stream_t stream) {
  if (int e = check_args(rows, C, true, workspace_bytes)) return e;
  int nb = red_blocks(rows, C);
  hipLaunchKernelGGL((col_reduce_kernel<0, T>), dim3(nb), dim3(RED_THREADS), 0, wsmg_s(stream), x, (const T*)nullptr,
                     (const T*)nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, workspace);
  hipLaunchKernelGGL(sum_finalize_kernel<false>, dim3(C), dim3(64), 0, wsmg_s(stream), workspace, nb, C, out, (float*)nullptr);
  WSMG_RETURN_LAUNCH();
}

template <class T>
int bn_act_fwd_t(const T* x, const T* residual, const float* gamma, const float* beta, float* running_mean,
                 float* running_var, float momentum, float eps, int train, int relu, int64_t rows, int C, T* y,
                 float* save_mean, float* save_invstd, double* workspace, int64_t workspace_bytes,
                 wsmg_stream_t stream) {
  if (int e = check_args(rows, C, train != 0, workspace_bytes)) return e;
  hipStream_t s = wsmg_s(stream);
  if (train) {
    int nb = red_blocks(rows, C);
    hipLaunchKernelGGL((col_reduce_kernel<1, T>), dim3(nb), dim3(RED_THREADS), 0, s, x, (const T*)nullptr,
                       (const T*)nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, workspace);
    launch_stats_finalize(workspace, nb, C, rows, momentum, eps, running_mean, running_var, save_mean, save_invstd, 0, s);
  } else {
    hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3((unsigned)wsmg_cdiv(C, 256)), dim3(256), 0, s, running_mean, running_var, eps, C,
                       save_mean, save_invstd);
  }
  launch_apply<T>(x, residual, gamma, beta, save_mean, save_invstd, relu, rows, C, y, s);
  WSMG_RETURN_LAUNCH();
}

// ld_dy: row stride of dy in elements (0: C); dx_lo: bf16 only
template <class T>
int bn_act_bwd_t(const T* dy, int64_t ld_dy, const T* x, const T* y, const float* gamma, const float* beta, const float* save_mean,
                 const float* save_invstd, int relu, int64_t rows, int C, T* dx, T* dx_lo, T* dresidual, float* dgamma, float* dbeta,
                 double* workspace, int64_t workspace_bytes, wsmg_stream_t stream) {
  if (ld_dy == 0) ld_dy = C;
  if (ld_dy < C || (ld_dy & 7) || ((uintptr_t)dy & 15)) return WSMG_EINVAL;
  if (relu && !y && (!beta || dresidual)) return WSMG_EINVAL;   // the mask can only be recomputed without a residual
  if (dx_lo && !std::is_same<T, bf16_t>::value) return WSMG_EINVAL;
  if (int e = check_args(rows, C, true, workspace_bytes)) return e;
  hipStream_t s = wsmg_s(stream);
  int nb = red_blocks(rows, C);
  hipLaunchKernelGGL((col_reduce_kernel<2, T>), dim3(nb), dim3(RED_THREADS), 0, s, x, dy, y, save_mean, save_invstd,
                     gamma, beta, relu, rows, C, workspace, ld_dy);
  hipLaunchKernelGGL(sum_finalize_kernel<true>, dim3(C), dim3(64), 0, s, workspace, nb, C, dbeta, dgamma);
  launch_bwd_apply<T>(dy, ld_dy, x, y, gamma, beta, save_mean, save_invstd, dgamma, dbeta, relu, rows, C, dx, dresidual, dx_lo, s);
  WSMG_RETURN_LAUNCH();
}

}  // namespace

// BatchNorm (train) + residual + ReLU of a bf16 tensor whose per-channel sums were already accumulated by the producing
// convolution's epilogue (wsmg_conv2d_fwd_bf16_stats): finalize (+ clear the slabs) and apply — no statistics pass over x.
extern "C" int wsmg_bn_act_fwd_bf16_pre(const void* x, const void* residual, const float* gamma, const float* beta,
                                        float* running_mean, float* running_var, float momentum, float eps, int relu,
                                        int64_t rows, int C, void* y, float* save_mean, float* save_invstd, double* stats,
                                        int nslab, wsmg_stream_t stream) {
  if (check_args(rows, C) || !stats || nslab <= 0) return WSMG_EINVAL;
  hipStream_t s = wsmg_s(stream);
  launch_stats_finalize(stats, nslab, C, rows, momentum, eps, running_mean, running_var, save_mean, save_invstd, 1, s);
  launch_apply<bf16_t>((const bf16_t*)x, (const bf16_t*)residual, gamma, beta, save_mean, save_invstd, relu, rows, C, (bf16_t*)y, s);
  WSMG_RETURN_LAUNCH();
}

// The two halves of wsmg_bn_act_fwd_bf16_pre / wsmg_bn_act_bwd_bf16 on their own, for callers that fuse the other half into a
// kernel of theirs (csrc/wsmg_cls_tail.hip): (1) batch statistics from the slabs a convolution's epilogue filled -> mean, 1 / sqrt(
// var + eps), running statistics; the slabs are handed back zeroed.  (2) dx = gamma invstd (dy - dbeta / n - xhat dgamma / n) for a
// dy that is ALREADY masked by the ReLU and whose two per-channel sums (dbeta = sum dy, dgamma = sum dy xhat) the caller supplies.
extern "C" int wsmg_bn_stats_finalize(double* stats, int nslab, int C, int64_t rows, float momentum, float eps, float* running_mean,
                                      float* running_var, float* save_mean, float* save_invstd, wsmg_stream_t stream) {
  if (check_args(rows, C) || !stats || nslab <= 0 || !save_mean || !save_invstd) return WSMG_EINVAL;
  launch_stats_finalize(stats, nslab, C, rows, momentum, eps, running_mean, running_var, save_mean, save_invstd, 1, wsmg_s(stream));
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_bn_bwd_apply_bf16(const void* dy, const void* x, const float* gamma, const float* mean, const float* invstd,
                                      const float* dgamma, const float* dbeta, int64_t rows, int C, void* dx, wsmg_stream_t stream) {
  if (check_args(rows, C) || !dy || !x || !gamma || !mean || !invstd || !dgamma || !dbeta || !dx) return WSMG_EINVAL;
  launch_bwd_apply<bf16_t>((const bf16_t*)dy, C, (const bf16_t*)x, nullptr, gamma, nullptr, mean, invstd, dgamma, dbeta, 0, rows, C,
                           (bf16_t*)dx, nullptr, nullptr, wsmg_s(stream));
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

// dy with a row stride (`ld_dy` elements, a multiple of 8, >= C): the channel slice of a concatenation's gradient is read in
// place (the decoders' `torch.cat(..., dim=1)` of map_encoder.py:104,110: autograd hands the two halves back as views)
extern "C" int wsmg_bn_act_bwd_ld(const float* dy, int64_t ld_dy, const float* x, const float* y, const float* gamma, const float* beta,
                                  const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C, float* dx,
                                  float* dresidual, float* dgamma, float* dbeta, double* workspace, int64_t workspace_bytes,
                                  wsmg_stream_t stream) {
  return bn_act_bwd_t<float>(dy, ld_dy, x, y, gamma, beta, save_mean, save_invstd, relu, rows, C, dx, nullptr, dresidual, dgamma, dbeta,
                             workspace, workspace_bytes, stream);
}
extern "C" int wsmg_bn_act_bwd_ld_bf16(const void* dy, int64_t ld_dy, const void* x, const void* y, const float* gamma,
                                       const float* beta, const float* save_mean, const float* save_invstd, int relu, int64_t rows,
                                       int C, void* dx, void* dresidual, float* dgamma, float* dbeta, double* workspace,
                                       int64_t workspace_bytes, wsmg_stream_t stream) {
  return bn_act_bwd_t<bf16_t>((const bf16_t*)dy, ld_dy, (const bf16_t*)x, (const bf16_t*)y, gamma, beta, save_mean, save_invstd, relu,
                              rows, C, (bf16_t*)dx, nullptr, (bf16_t*)dresidual, dgamma, dbeta, workspace, workspace_bytes, stream);
}
// the same with rows of dy that follow each other (ld_dy = C)
extern "C" int wsmg_bn_act_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* beta,
                               const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C,
                               float* dx, float* dresidual, float* dgamma, float* dbeta, double* workspace,
                               int64_t workspace_bytes, wsmg_stream_t stream) {
  return wsmg_bn_act_bwd_ld(dy, C, x, y, gamma, beta, save_mean, save_invstd, relu, rows, C, dx, dresidual, dgamma, dbeta, workspace,
                            workspace_bytes, stream);
}
extern "C" int wsmg_bn_act_bwd_bf16(const void* dy, const void* x, const void* y, const float* gamma, const float* beta,
                                    const float* save_mean, const float* save_invstd, int relu, int64_t rows, int C,
                                    void* dx, void* dresidual, float* dgamma, float* dbeta, double* workspace,
                                    int64_t workspace_bytes, wsmg_stream_t stream) {
  return wsmg_bn_act_bwd_ld_bf16(dy, C, x, y, gamma, beta, save_mean, save_invstd, relu, rows, C, dx, dresidual, dgamma, dbeta, workspace,
                                 workspace_bytes, stream);
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
  return bn_act_bwd_t<bf16_t>((const bf16_t*)dy, ld_dy, (const bf16_t*)x, (const bf16_t*)y, gamma, beta, save_mean, save_invstd, relu,
                              rows, C, (bf16_t*)dx, (bf16_t*)dx_lo, (bf16_t*)dresidual, dgamma, dbeta, workspace, workspace_bytes, stream);
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
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
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
  const double t = block_sum_d((double)s, red[0]), tt = block_sum_d((double)ss, red[1]);   // every thread has both
  const double mean64 = t / n;
  double var = tt / n - mean64 * mean64;
  if (var < 0) var = 0;
  const float mean = (float)mean64, inv = (float)(1.0 / sqrt(var + (double)eps));
  for (int i = tid; i < n; i += 256) {
    const int p = i / Cg, c = i - p * Cg;
    const size_t o = base + (size_t)p * C + c;
    float v = bn_value((float)x[o], mean, inv, gamma[g * Cg + c], beta[g * Cg + c]);
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
