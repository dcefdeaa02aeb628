// The rollout side of a policy-gradient update: what `ppo_loss` (wsmg_pg_heads.hip) takes as `returns` and `adv`, in ONE launch
// instead of the ≈ 6 T host-paced launches of habitat-baselines' `RolloutStorage.compute_returns` + `PPO.get_advantages` in torch
// (restated here; habitat is not a dependency):
//
//   use_gae:   value_preds[T] = next_value;  g = 0
//              for s = T-1 .. 0:  d = ((rewards[s] + (gamma * value_preds[s+1]) * masks[s+1]) - value_preds[s])
//                                 g = d + (gamma_tau * masks[s+1]) * g
//                                 returns[s] = g + value_preds[s]                  (returns[T] is left as it was)
//   else:      returns[T] = next_value
//              for s = T-1 .. 0:  returns[s] = ((returns[s+1] * gamma) * masks[s+1]) + rewards[s]
//   adv[s]   = returns[s] - value_preds[s]                                          s < T
//   adv_norm = (adv - mean(adv)) / (std(adv) + eps),  std unbiased, over all T N entries
//
// The scan.  Every product, sum and difference above is ONE float32 operation rounded on its own, in that parenthesisation and in
// that order over s: with it `returns`, `adv` and `value_preds[T]` are the bits of the float32 torch loop.  The operations are
// written with __fmul_rn / __fadd_rn / __fsub_rn, and the file is compiled with -ffp-contract=off (csrc/Makefile): the intrinsics
// are plain operators in this toolchain's headers, which the default contraction would fuse into multiply-adds.
//
// One workgroup of 256 threads, a thread per environment: thread t owns columns t, t + 256, ... and walks each from s = T-1 down.
// The chain is four dependent float operations per step; what bounds it is the latency of the three row loads (rewards[s],
// value_preds[s], masks[s+1]), so they are issued GAE_PF steps ahead of the chain into a register ring (loads past row 0 are
// clamped to row 0 and dropped).  No LDS staging form: there is no size limit and no second kernel.
//
// The statistics.  float64, fixed order, no atomics: thread t adds the advantages of its columns in the order it produced them,
// block_sum_d adds the 256 partial sums; the mean comes first, sum (adv - mean)^2 in a second pass over what the same thread stored
// (adv is formed again as returns[s] - value_preds[s], the same float32 subtraction, so no `adv` buffer is needed), adv_norm in a
// third, formed in double and rounded once.  T N = 1: 0 / 0, std and adv_norm NaN as torch gives.
#include "wsmg_common.h"

namespace {

constexpr int GAE_PF = 16;          // steps the row loads run ahead of the chain
constexpr int GAE_BATCH = 8;        // independent loads in flight in the two statistics passes
constexpr int GAE_MAXN = 1024;
constexpr long long GAE_MAXTN = 1ll << 24;

struct GaeArgs {
  const float* rewards;     // [T][N]
  float* value_preds;       // [T+1][N]
  const float* masks;       // [T+1][N]
  const float* next_value;  // [N]
  float gamma, gamma_tau;
  int T, N;
  float* returns;           // [T+1][N]
  float* adv;               // [T][N] or null
  float* adv_norm;          // [T][N] or null
  double* stats;            // {mean, std} or null
  float eps;
};

// one column, s = T-1 .. 0; returns the column's advantages added to `sum` in that order
template <bool GAE>
__device__ __forceinline__ void gae_scan_column(const GaeArgs& a, int n, double& sum) {
  const int T = a.T, N = a.N;
  float r[GAE_PF], v[GAE_PF], m[GAE_PF];
#pragma unroll
  for (int j = 0; j < GAE_PF; ++j) {
    const int s = max(T - 1 - j, 0);
    r[j] = a.rewards[s * N + n];
    v[j] = a.value_preds[s * N + n];
    m[j] = a.masks[(s + 1) * N + n];
  }
  float carry = a.next_value[n];       // GAE: value_preds[s+1]; else returns[s+1]
  float g = 0.f;
  if (GAE) a.value_preds[T * N + n] = carry;
  else a.returns[T * N + n] = carry;
  for (int s0 = T - 1; s0 >= 0; s0 -= GAE_PF) {
#pragma unroll
    for (int j = 0; j < GAE_PF; ++j) {
      const int s = s0 - j;
      const float rs = r[j], vs = v[j], ms = m[j];
      const int sp = max(s - GAE_PF, 0);
      r[j] = a.rewards[sp * N + n];
      v[j] = a.value_preds[sp * N + n];
      m[j] = a.masks[(sp + 1) * N + n];
      if (s >= 0) {
        float ret;
        if (GAE) {
          const float d = __fsub_rn(__fadd_rn(rs, __fmul_rn(__fmul_rn(a.gamma, carry), ms)), vs);
          g = __fadd_rn(d, __fmul_rn(__fmul_rn(a.gamma_tau, ms), g));
          ret = __fadd_rn(g, vs);
          carry = vs;
        } else {
          ret = __fadd_rn(__fmul_rn(__fmul_rn(carry, a.gamma), ms), rs);
          carry = ret;
        }
        a.returns[s * N + n] = ret;
        const float ad = __fsub_rn(ret, vs);
        if (a.adv) a.adv[s * N + n] = ad;
        sum += (double)ad;
      }
    }
  }
}

// The advantages of column n again, s = T-1 .. 0, GAE_BATCH loads at a time ahead of their use: f(s, adv) in that order.
template <class F>
__device__ __forceinline__ void gae_column_again(const GaeArgs& a, int n, F f) {
  const int T = a.T, N = a.N;
  for (int s0 = T - 1; s0 >= 0; s0 -= GAE_BATCH) {
    float ret[GAE_BATCH], v[GAE_BATCH];
#pragma unroll
    for (int j = 0; j < GAE_BATCH; ++j) {
      const int s = max(s0 - j, 0);
      ret[j] = a.returns[s * N + n];
      v[j] = a.value_preds[s * N + n];
    }
#pragma unroll
    for (int j = 0; j < GAE_BATCH; ++j)
      if (s0 - j >= 0) f(s0 - j, __fsub_rn(ret[j], v[j]));
  }
}

template <bool GAE>
__device__ __forceinline__ void gae_body(const GaeArgs& a, double* red_sum, double* red_sq) {
  const int N = a.N;
  double sum = 0.0;
  for (int n = threadIdx.x; n < N; n += 256) gae_scan_column<GAE>(a, n, sum);
  if (!a.adv_norm && !a.stats) return;      // (the same for every thread)
  const double count = (double)a.T * (double)N;
  const double mean = block_sum_d(sum, red_sum) / count;
  double sq = 0.0;
  for (int n = threadIdx.x; n < N; n += 256)
    gae_column_again(a, n, [&](int, float ad) {
      const double d = (double)ad - mean;
      sq += d * d;
    });
  const double sd = sqrt(block_sum_d(sq, red_sq) / (count - 1.0));
  if (threadIdx.x == 0 && a.stats) {
    a.stats[0] = mean;
    a.stats[1] = sd;
  }
  if (!a.adv_norm) return;
  const double den = sd + (double)a.eps;
  for (int n = threadIdx.x; n < N; n += 256)
    gae_column_again(a, n, [&](int s, float ad) { a.adv_norm[s * N + n] = (float)(((double)ad - mean) / den); });
}

__global__ __launch_bounds__(256) void gae_returns_kernel(GaeArgs a, int use_gae) {
  __shared__ double red_sum[4], red_sq[4];        // block_sum_d: each sum a red of its own
  if (use_gae) gae_body<true>(a, red_sum, red_sq);
  else gae_body<false>(a, red_sum, red_sq);
}

}  // namespace

extern "C" int wsmg_gae_returns(const float* rewards, float* value_preds, const float* masks, const float* next_value, float gamma,
                                float gamma_tau, int use_gae, int T, int N, float* returns, float* adv, float* adv_norm,
                                double* stats, float eps, wsmg_stream_t stream) {
  if (!rewards || !value_preds || !masks || !next_value || !returns) return WSMG_EINVAL;
  if (T < 1 || N < 1 || N > GAE_MAXN || (long long)T * N >= GAE_MAXTN) return WSMG_EINVAL;
  GaeArgs a{rewards, value_preds, masks, next_value, gamma, gamma_tau, T, N, returns, adv, adv_norm, stats, eps};
  hipLaunchKernelGGL(gae_returns_kernel, dim3(1), dim3(256), 0, wsmg_s(stream), a, use_gae);
  WSMG_RETURN_LAUNCH();
}
