// Shared helpers for the gfx950 kernels of libwsmgmap.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "wsmgmap.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef __bf16 bf16_t;
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

#define WSMG_WAVE 64

// storage-type helpers: activations are float32 or bf16 in HBM, arithmetic is float32
__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const bf16_t* p) { return (float)*p; }
__device__ __forceinline__ void stf(float* p, float v) { *p = v; }
__device__ __forceinline__ void stf(bf16_t* p, float v) { *p = (bf16_t)v; }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4(const bf16_t* p) {
  u16x4 u = *reinterpret_cast<const u16x4*>(p);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = __uint_as_float(((unsigned)u[j]) << 16);
  return o;
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ void st4(bf16_t* p, f32x4 v) {
  u16x4 u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16_t b = (bf16_t)v[j];
    u[j] = __builtin_bit_cast(unsigned short, b);
  }
  *reinterpret_cast<u16x4*>(p) = u;
}

// N consecutive channels of a row: N = 4 (float32, or bf16 through ld4 / st4) or N = 8 (bf16 only, one 16-byte access).  chans_t is
// what the load returns (a kernel that keeps several loads in flight holds them in this form), chans_f32 its N float32 values; the
// store rounds each value to T once.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // four 32-bit words
template <int N> using chans_t = typename std::conditional<N == 8, u32x4, f32x4>::type;
template <int N, class T>
__device__ __forceinline__ chans_t<N> ld_chans_raw(const T* p) {
  if constexpr (N == 8) return *reinterpret_cast<const u32x4*>(p);
  else return ld4(p);
}
template <int N>
__device__ __forceinline__ void chans_f32(chans_t<N> d, float (&o)[N]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (N == 8) {
      o[2 * j] = __uint_as_float(d[j] << 16);
      o[2 * j + 1] = __uint_as_float(d[j] & 0xffff0000u);
    } else {
      o[j] = d[j];
    }
  }
}
template <int N, class T>
__device__ __forceinline__ void ld_chans(const T* p, float (&o)[N]) { chans_f32<N>(ld_chans_raw<N>(p), o); }
template <int N, class T>
__device__ __forceinline__ void st_chans(T* p, const float (&g)[N]) {
  if constexpr (N == 8) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16_t lo = (bf16_t)g[2 * j], hi = (bf16_t)g[2 * j + 1];
      o[j] = (unsigned)__builtin_bit_cast(unsigned short, lo) | ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
    }
    *reinterpret_cast<u32x4*>(p) = o;
  } else {
    const f32x4 o = {g[0], g[1], g[2], g[3]};
    st4(p, o);
  }
}

// after a kernel launch: report launch-time errors through the C ABI's int return
#define WSMG_RETURN_LAUNCH()                      \
  do {                                            \
    hipError_t e__ = hipGetLastError();           \
    return e__ == hipSuccess ? 0 : (int)e__;      \
  } while (0)

static inline hipStream_t wsmg_s(wsmg_stream_t s) { return (hipStream_t)s; }

// Tuning / A-B switches of the library (WSMG_* environment variables of the launchers: tile choices, kernel variants).  Every one
// is read ONCE per process, at the first launch that asks — no launch after that touches the environment.  WSMG_TUNE is the
// only way the library reads it.
static inline int wsmg_tune_read(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
#define WSMG_TUNE(name, dflt) ([]() -> int { static const int v_ = wsmg_tune_read(name, dflt); return v_; }())

static inline int64_t wsmg_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// workgroups of a grid-stride launch of 256 threads over n items (wsmg_pool.hip, wsmg_layout.hip): 1 .. 16384
static inline int wsmg_sgrid(int64_t n) {
  int64_t g = wsmg_cdiv(n, 256);
  if (g > 16384) g = 16384;
  if (g < 1) g = 1;
  return (int)g;
}

// Multi-tensor launches (wsmg_optim.hip's Adam / norm kernels, wsmg_small.hip's guarded copy): tensors per launch — the table lives
// in the kernel arguments, a longer list is cut into several launches — and the guard record of wsmg_grad_norm_multi, four float32.
constexpr int ADAM_MAX = 48;
// Fields per launch of the grouped column gather (wsmg_rollout_gather.hip): its table, 32 x 28 bytes, is in the kernel arguments too.
constexpr int GATHER_MAX = 32;
enum { GUARD_NORM = 0, GUARD_COEF = 1, GUARD_SKIP = 2, GUARD_SKIPPED = 3 };

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// The sum over a workgroup of 256 threads, valid in every thread, in a fixed order: the wave's xor tree, then the four waves in
// index order.  red: four LDS words.  The float form may be called again on the same red at once (it waits before it writes);
// the double form does not wait: a kernel gives each of its sums a red of its own.
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
// the maximum over the same workgroup, the float block_sum's way (same red, same waits)
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(fmaxf(red[0], red[1]), red[2]), red[3]);
}
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// The bf16 conv engine.  Which kernel family takes a layer is decided in ONE place, wsmg_conv_route (wsmg_conv_route.hip, where the
// tunes are listed); the launchers of wsmg_conv_bf16.hip switch on its answer.  Each kernel file owns the acceptance test of its
// kernel — the function the route asks and the entry point's own argument check (a `_fits` answers yes / no, a `_splits` / `_grid`
// the slab / workgroup count, 0 = the layer is not this kernel's) — so an entry point that answers WSMG_EINVAL to a routed layer is a
// bug, which the launchers hand back, not a reason to try another kernel.
struct WsmgConvRoute {
  int kind;                     // WSMG_ROUTE_*: the kernel family
  int mt, by_shape, mixed;      // 3 x 3 window: pixels per workgroup; chosen by shape (not forced); half-size tiles allowed in the last round
  int wgs;                      // k32 / ConvTranspose: workgroups per CU
  int nsplit;                   // weight gradient: partial sums (pixel chunks / image ranges / tile groups) = slabs of the deterministic form
  int tc, tu, gx, gy;           // generic weight gradient: tile shape and grid
  int64_t chunk;                //   ... and pixels per split
};
// pass: WSMG_CONV_FWD / _BWD_DATA / _BWD_WEIGHT; the geometry is the convolution's (x [B][H][W][Cin], y [B][OH][OW][Cout]) in every pass
// and has passed wsmg_check_conv_bf16; needs: the WSMG_NEED_* bits of the call, everything about it that is no pointer
WsmgConvRoute wsmg_conv_route(int pass, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int needs);
// wsmg_conv_bf16.hip: the generic weight-gradient kernel's plan (tc .. chunk, nsplit), written into r
void wsmg_conv_wgrad_plan(int B, int Cin, int Cout, int KH, int KW, int OH, int OW, WsmgConvRoute& r);
// wsmg_conv_win.hip: direct convolution with an LDS-resident input window (64 -> 64 channels, k8 s2 p3)
bool wsmg_conv_win_fits(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
int wsmg_conv_win_fwd_bf16(const void* x, const void* w_ohwi, const float* bias, void* y, int relu, double* stats, int nslab, int B,
                           int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, hipStream_t s);
// wsmg_conv_win_wgrad.hip: weight gradient of the same layer out of an LDS-resident input window (its test: winw_fits)
int wsmg_conv_win_wgrad_splits(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW);
int wsmg_conv_win_wgrad_bf16(const void* x, const void* dy, float* dw_ohwi, long long slab_floats, int B, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, int OH, int OW, hipStream_t s);
// wsmg_conv_s2_wgrad.hip: weight gradient of the k5 s2 (64 -> 128 at 50 x 50) and k7 s2 (256 -> 64 at 24 x 24) layers out of an
// LDS-resident input window (its test: s2w_shape)
int wsmg_conv_s2_wgrad_splits(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW);
int wsmg_conv_s2_wgrad_bf16(const void* x, const void* dy, float* dw_ohwi, long long slab_floats, int B, int H, int W, int Cin, int Cout,
                            int KH, int KW, int stride, int pad, int OH, int OW, hipStream_t s);
// wsmg_conv_win3.hip: 3 x 3 / stride 1 / pad 1 out of a zero-padded LDS pixel window (forward / backward-data), N % 32 == 0,
// Kc % 32 == 0, mt = 512 or 256 pixels per workgroup, mixed != 0: the last partial round as half-size tiles where that pays
// (round 6) relu_z [pixels][N] or null: ReLU outputs the output tile is masked with (wsmg_relu_mask.h); dst_ld: pixel pitch of dst in
// elements (0 = N); dst2 / split_c: output channels >= split_c go to the second tensor (null: none)
bool wsmg_conv_win3_fits(int mt, int B, int H, int W, int Kc, int N);
int wsmg_conv_win3_bf16(int bwd, const void* src, const void* wt, const float* bias, void* dst, int relu, double* stats, int nslab,
                        int B, int H, int W, int Kc, int N, int mt, int mixed, const void* relu_z, int dst_ld, void* dst2, int split_c,
                        hipStream_t s);
// wsmg_conv_win3_k32.hip (round 6): the same convolution over a 32-channel reduction axis (Kc == 32, N % 32 == 0, plain output): weights
// resident in LDS, one barrier per 256-pixel tile, three workgroups per CU; wgs: workgroups per CU of the grid
int64_t wsmg_conv_win3_k32_grid(int B, int H, int W, int N, int wgs);
int wsmg_conv_win3_k32_bf16(int bwd, const void* src, const void* wt, const float* bias, void* dst, int relu, double* stats, int nslab,
                            int B, int H, int W, int N, int dst_ld, int wgs, hipStream_t s);
// wsmg_convt_k4s2.hip (round 6): ConvTranspose2d(64 -> 32, k4, s2, p1) forward — both column parities of a row parity per workgroup,
// weights resident in LDS, full-line stores.  The test takes the adjoint convolution's geometry (its backward-data pass), the entry
// point the ConvTranspose's input grid H x W
int64_t wsmg_convt_k4s2_grid(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int wgs);
int wsmg_convt_k4s2_bf16(const void* src, const void* w_ihwo, void* dst, double* stats, int nslab, int B, int H, int W, int wgs,
                         hipStream_t s);
// wsmg_conv_win3_wgrad.hip: weight gradient of a 3 x 3 / stride 1 / pad 1 layer out of a zero-padded LDS window (W <= 24, channel
// multiples of 64 / 128; its test: w3w_variant)
int wsmg_conv_win3_wgrad_splits(int B, int H, int W, int Cin, int Cout);
int wsmg_conv_win3_wgrad_bf16(const void* x, const void* dy, float* dw_ohwi, long long slab_floats, int B, int H, int W, int Cin, int Cout,
                              hipStream_t s);
// wsmg_rnn.hip: device pointer of the process-wide persistent-kernel status word (host-mapped; bits 1 gru_fwd, 2 gru_bwd, 4 lstm_fwd,
// 8 lstm_bwd), for kernels of other files that wait on a chain counter (wsmg_rows_gemm.hip)
unsigned* wsmgi_rnn_status_dev();
