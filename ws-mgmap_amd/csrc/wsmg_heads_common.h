// What the heads kernels on [B, K] features share: update_heads (wsmg_heads.hip: A action means + the tanh progress head) and
// eval_heads (wsmg_pg_heads.hip: A action means + the critic) are both "A + 1 dot products per row" forward and "A + 1 head
// gradients per row" backward.  The row projection and the column-owned backward are written here once; a kernel adds lane 0's
// epilogue (forward) or a row policy (backward).
#pragma once
#include "wsmg_common.h"

constexpr int HEADS_MAXA = 4;     // action dimensions of update_heads / eval_heads (the reference's waypoint head has 2)
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;

// One wave per row: lane l holds 4 consecutive features per 256-feature pass (K % 4 == 0, 16-byte loads).  s[o] = x_row . wm[o]
// for o < A, s[HEADS_MAXA] = x_row . w1, each summed over the wave (valid in every lane).
__device__ __forceinline__ void heads_row_dots(const float* __restrict__ xr, const float* wm, const float* w1, int K, int A, int lane,
                                               float (&s)[HEADS_MAXA + 1]) {
#pragma unroll
  for (int o = 0; o <= HEADS_MAXA; ++o) s[o] = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + k);
#pragma unroll
    for (int o = 0; o < HEADS_MAXA; ++o)
      if (o < A) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wm + (size_t)o * K + k);
        s[o] += xv[0] * wv[0] + xv[1] * wv[1] + xv[2] * wv[2] + xv[3] * wv[3];
      }
    const f32x4 pv = *reinterpret_cast<const f32x4*>(w1 + k);
    s[HEADS_MAXA] += xv[0] * pv[0] + xv[1] * pv[1] + xv[2] * pv[2] + xv[3] * pv[3];
  }
#pragma unroll
  for (int o = 0; o <= HEADS_MAXA; ++o) s[o] = wave_sum(s[o]);
}

// The backward of both: a workgroup of 256 threads owns 8 features (columns) for ALL rows: thread = (feature f, row group g of 32);
// row b belongs to group b % 32 (8 x 32, not 32 x 8: the kernel sits alone between the recurrent core's forward and backward, and
// 64 workgroups of 16-row loops at B = K = 512 are 12.6 us of dependent loads where 16 of 64-row loops were 45).
// d x[b][f] = sum_o g_o[b] w_o[f] is written directly; d w_o[f] = sum_b g_o[b] x[b][f] is accumulated per thread over its rows in
// row order and the 32 groups are added in group order — no atomics, the same bits every run.  The row's numbers are recomputed by
// every workgroup: a handful of flops.  Workgroup 0 adds, the same way, the sums over rows that have no feature axis.
//
// Row is the kernel's policy, built once per thread from the argument struct a (which has x, wm, dx, dwm, B, K, A):
//   Row::NX                    row sums beyond the HEADS_MAXA + 1 head gradients
//   row.fill(a, b, go, extra)  go[HEADS_MAXA + 1]: the head gradients g_o[b] (0 for A <= o < HEADS_MAXA); extra[NX]: the other terms
//   Row::store(a, o, s)        s is row sum o, of go[o] or of extra[o - HEADS_MAXA - 1] over all rows: store it (workgroup 0's thread o)
// w1 / dw1 [K]: the weight row of head HEADS_MAXA and its gradient.
template <class Row, class Args>
__device__ __forceinline__ void heads_bwd_columns(const Args& a, const float* w1, float* dw1) {
  constexpr int FC = 8, RG = 32, NH = HEADS_MAXA + 1, NS = NH + Row::NX;
  __shared__ float part[RG][NH][FC];
  __shared__ float bpart[RG][NS];
  const int f = threadIdx.x & (FC - 1), g = threadIdx.x / FC;
  const int col = blockIdx.x * FC + f;
  const bool live = col < a.K;
  float wv[NH], acc[NH], bacc[NS];
#pragma unroll
  for (int o = 0; o < NH; ++o) { wv[o] = 0.f; acc[o] = 0.f; }
#pragma unroll
  for (int o = 0; o < NS; ++o) bacc[o] = 0.f;
  const Row row(a);
  if (live) {
#pragma unroll
    for (int o = 0; o < HEADS_MAXA; ++o)
      if (o < a.A) wv[o] = a.wm[(size_t)o * a.K + col];
    wv[HEADS_MAXA] = w1[col];
  }
#pragma unroll 4
  for (int b = g; b < a.B; b += RG) {       // (independent rows: several in flight)
    float go[NH], extra[Row::NX ? Row::NX : 1];
    row.fill(a, b, go, extra);
    if (live) {
      const float xv = a.x[(size_t)b * a.K + col];
      float d = 0.f;
#pragma unroll
      for (int o = 0; o < NH; ++o) {
        d += go[o] * wv[o];
        acc[o] += go[o] * xv;
      }
      a.dx[(size_t)b * a.K + col] = d;
    }
#pragma unroll
    for (int o = 0; o < NH; ++o) bacc[o] += go[o];
#pragma unroll
    for (int o = 0; o < Row::NX; ++o) bacc[NH + o] += extra[o];
  }
#pragma unroll
  for (int o = 0; o < NH; ++o) part[g][o][f] = acc[o];
  if (blockIdx.x == 0 && f == 0) {          // (every feature lane of a group holds the same row sums)
#pragma unroll
    for (int o = 0; o < NS; ++o) bpart[g][o] = bacc[o];
  }
  __syncthreads();
  if (g == 0 && live) {
#pragma unroll
    for (int o = 0; o < NH; ++o) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < RG; ++q) s += part[q][o][f];
      if (o < HEADS_MAXA) { if (o < a.A) a.dwm[(size_t)o * a.K + col] = s; }
      else dw1[col] = s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < NS) {
    const int o = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < RG; ++q) s += bpart[q][o];
    Row::store(a, o, s);
  }
}
