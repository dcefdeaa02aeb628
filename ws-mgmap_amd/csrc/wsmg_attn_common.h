// What the attention kernels (wsmg_attn.hip, wsmg_attn_fp8.hip, wsmg_attn_fp8_mfma.hip, wsmg_attn_fp8_mfma_bwd.hip) share: the
// channel count and token limits, the e4m3 codec, the token-trip load of the single-query kernels and the combine of the waves'
// partial rows.  Every kernel keeps its own walk over the tokens, its softmax and its tiles.
#pragma once
#include "wsmg_common.h"

constexpr int AC = 256;        // channels (hidden_size / 2): a token row is one wave-wide load of four channels per lane
// tokens per row of the single-query float32 / bf16 kernels: the row's logits stay in LDS (10 KiB); 2304 = the 48 x 48 encoded map of
// the E = 196 geometry
constexpr int AMAX_I = 2560;
// tokens per row / per set of every e4m3 kernel: the row's bytes stay in LDS (224 x 256 = 56 KB); a multiple of the MFMA kernels'
// 32-token chunk (the reference pads instructions to 200)
constexpr int F8_MAX_L = 224;

// ----------------------------------------------------------------------------- e4m3 (OCP, 448 = its largest finite value)
// encode: x * inv_scale clamped to +-448 (the conversion itself makes NaN of anything larger), round to nearest even; byte j of a word
// is value j
__device__ __forceinline__ float e4m3_fit(float x, float inv_scale) { return fminf(fmaxf(x * inv_scale, -448.f), 448.f); }
__device__ __forceinline__ unsigned e4m3_pack4(float a, float b, float c, float d) {      // values inside +-448
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (unsigned)w;
}
__device__ __forceinline__ unsigned e4m3_enc4(f32x4 v, float inv_scale) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = e4m3_fit(v[j], inv_scale);
  return e4m3_pack4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ long e4m3_enc8(f32x4 a, f32x4 b, float inv_scale) {      // 8 consecutive values: one MFMA operand
  float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = e4m3_fit(x[j], inv_scale);
  const unsigned lo = e4m3_pack4(x[0], x[1], x[2], x[3]), hi = e4m3_pack4(x[4], x[5], x[6], x[7]);
  return (long)(((unsigned long)hi << 32) | (unsigned long)lo);
}
__device__ __forceinline__ long e4m3_enc8(const float* p, float inv_scale) {      // ... of 8 consecutive floats in memory
  return e4m3_enc8(*reinterpret_cast<const f32x4*>(p), *reinterpret_cast<const f32x4*>(p + 4), inv_scale);
}
// the factor every quantiser that reads its scale on the device multiplies by: float32(1 / scale) from a float64 quotient, as the
// host computes the inv_scale it hands to wsmg_quantize_e4m3
__device__ __forceinline__ float e4m3_inv_scale(float scale) { return (float)(1.0 / (double)scale); }
// decode to float32: the four codes of a word
__device__ __forceinline__ f32x4 e4m3_dec4(unsigned w) {
  auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return f32x4{lo[0], lo[1], hi[0], hi[1]};
}
// decode to bf16 bits, exact (e4m3 has 4 significant bits): byte BYTE of a word (a single code: byte 0), the 8 codes of an MFMA operand
typedef short bf16x8 __attribute__((ext_vector_type(8)));      // (wsmg_conv_tile.h's type)
template <int BYTE = 0>
__device__ __forceinline__ short e4m3_dec_bf(int w) {
  return __builtin_bit_cast(short, (bf16_t)__builtin_amdgcn_cvt_f32_fp8(w, BYTE));
}
__device__ __forceinline__ bf16x8 e4m3_dec8_bf(long w) {
  const int w0 = (int)(w & 0xffffffffl), w1 = (int)((unsigned long)w >> 32);
  return bf16x8{e4m3_dec_bf<0>(w0), e4m3_dec_bf<1>(w0), e4m3_dec_bf<2>(w0), e4m3_dec_bf<3>(w0),
                e4m3_dec_bf<0>(w1), e4m3_dec_bf<1>(w1), e4m3_dec_bf<2>(w1), e4m3_dec_bf<3>(w1)};
}

// ----------------------------------------------------------------------------- single-query kernels
// One trip of a wave over a row's tokens: rows i0 .. i0 + N - 1 of this lane's four channels (base = the row's first token + 4 lane),
// zeros at and past I
template <int N, class T>
__device__ __forceinline__ void load_tokens(const T* base, int i0, int I, f32x4 (&x)[N]) {
#pragma unroll
  for (int u = 0; u < N; ++u) x[u] = (i0 + u < I) ? ld4(base + (size_t)(i0 + u) * AC) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// The waves' partial rows [NW][AC] through LDS: every wave puts its lanes' four channels, and after the kernel's barrier a thread adds
// the NW values of channel c in wave index order (no atomics: the sum has one order)
__device__ __forceinline__ void put_row(float (*part)[AC], int wave, int lane, f32x4 acc) {
  reinterpret_cast<f32x4*>(&part[wave][0])[lane] = acc;
}
template <int NW>
__device__ __forceinline__ float sum_rows(const float (*part)[AC], int c) {
  float r = part[0][c];
#pragma unroll
  for (int w = 1; w < NW; ++w) r += part[w][c];
  return r;
}
