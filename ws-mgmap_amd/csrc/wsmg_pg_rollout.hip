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
//
// The reward normaliser (reward_normalize_kernel, and in front of the scan in gae_returns_normalized_kernel): baselines' `VecNormalize`
// return path, restated (not a dependency): rewards divided by the running standard deviation of the discounted return.  State,
// float64: {mean, var, count, ret[N]}.  For s = s0 .. T-1 in order, every operation float64 and rounded on its own (the file's
// -ffp-contract=off keeps a * b + c two operations here too):
//
//   ret[n]  = ret[n] * gamma + rewards[s][n]
//   bmean   = sum_n ret[n] / N;   bM2 = sum_n (ret[n] - bmean)^2;   delta = bmean - mean;   tot = count + N
//   mean    = mean + (delta * N) / tot
//   var     = ((var * count + bM2) + (((delta * delta) * count) * N) / tot) / tot;   count = tot
//   out[s][n] = float32(clamp(rewards[s][n] / sqrt(var + eps), -clip, +clip))          (rounded once; NaN stays NaN)
//   ret[n] *= masks[s+1][n]
//
// With update == 0 only the `out` line runs, with the stored var, and the state is not written.
// The same workgroup shape: thread t owns columns t, t + 256, ... (at most four), but walks them TOGETHER, forward, since every
// step needs two sums over n.  The columns' `ret` stay in registers as doubles; a step's two sums are the thread's own columns in
// index order, then block_sum_d (wave xor tree, four waves in index order): a fixed order, no atomics, the same bits every launch.
// The step is bound by its two barriers and reductions; the two row loads (rewards[s], masks[s+1]) of a thread's columns run NORM_PF
// steps ahead in a register ring (loads past row T-1 are clamped to it and dropped).
// State hand-over.  mean, var and count are read and written by thread 0 ALONE (it hands the three it read to the others through
// LDS behind a barrier), ret[n] by the owner of column n alone: no thread reads a state word another thread writes.
// Row hand-over in gae_returns_normalized_kernel.  The scan (gae_body, unchanged) reads `rewards_norm` where wsmg_gae_returns reads
// `rewards`.  Thread t's scan, and its two statistics passes, read columns t, t + 256, ... only — the columns whose rows [s0, T) the
// same thread stored in the forward walk (rows below s0 are an earlier launch's).  A wave's vector memory operations on one
// address are performed in program order, so a thread's load sees its own earlier store without a fence, a wait or a barrier, as
// gae_column_again's reads of `returns` already rely on; nothing is handed from one thread to another through global memory.
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

// ---- the reward normaliser ----------------------------------------------------------------------------------------------------------
constexpr int NORM_PF = 8;          // steps the row loads run ahead of the walk

struct NormArgs {
  const float* rewards;     // [T][N]
  const float* masks;       // [T+1][N]
  double* state;            // {mean, var, count, ret[N]}
  float* out;               // [T][N]: rows [s0, T) are written
  float gamma, eps, clip;
  int T, N, s0, update;
};

__device__ __forceinline__ float norm_one(float r, double sd, double clip) {
  const double x = (double)r / sd;
  return (float)(x < -clip ? -clip : (x > clip ? clip : x));      // (a NaN fails both comparisons and stays)
}

// update != 0: rows s0 .. T-1 forward, NC columns per thread; red_m / red_q: a red per sum (a step's second barrier stands between
// the last read of red_m and its next write, the next step's first between those of red_q); bc: three LDS doubles
template <int NC>
__device__ __forceinline__ void norm_walk(const NormArgs& a, double* red_m, double* red_q, double* bc) {
  const int T = a.T, N = a.N, s0 = a.s0;
  const double gamma = (double)a.gamma, eps = (double)a.eps, clip = (double)a.clip, dN = (double)N;
  if (threadIdx.x == 0) {
    bc[0] = a.state[0];
    bc[1] = a.state[1];
    bc[2] = a.state[2];
  }
  __syncthreads();
  double mean = bc[0], var = bc[1], count = bc[2];
  int col[NC];
  bool own[NC];
  double ret[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int n = (int)threadIdx.x + 256 * k;
    own[k] = n < N;
    col[k] = own[k] ? n : 0;           // a column past N loads column 0 and drops it
    ret[k] = own[k] ? a.state[3 + n] : 0.0;
  }
  float r[NORM_PF][NC], m[NORM_PF][NC];
#pragma unroll
  for (int j = 0; j < NORM_PF; ++j) {
    const int s = min(s0 + j, T - 1);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      r[j][k] = a.rewards[s * N + col[k]];
      m[j][k] = a.masks[(s + 1) * N + col[k]];
    }
  }
  for (int sb = s0; sb < T; sb += NORM_PF) {
#pragma unroll
    for (int j = 0; j < NORM_PF; ++j) {
      const int s = sb + j;
      float rs[NC], ms[NC];
      const int sp = min(s + NORM_PF, T - 1);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        rs[k] = r[j][k];
        ms[k] = m[j][k];
        r[j][k] = a.rewards[sp * N + col[k]];
        m[j][k] = a.masks[(sp + 1) * N + col[k]];
      }
      if (s < T) {          // (the same for every thread: the barriers below are met by all)
        double part = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (own[k]) {
            ret[k] = ret[k] * gamma + (double)rs[k];
            part += ret[k];
          }
        const double bmean = block_sum_d(part, red_m) / dN;
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (own[k]) {
            const double d = ret[k] - bmean;
            q += d * d;
          }
        const double bm2 = block_sum_d(q, red_q);
        const double delta = bmean - mean, tot = count + dN;
        mean = mean + delta * dN / tot;
        var = (var * count + bm2 + delta * delta * count * dN / tot) / tot;
        count = tot;
        const double sd = sqrt(var + eps);
#pragma unroll
        for (int k = 0; k < NC; ++k)
          if (own[k]) {
            a.out[s * N + col[k]] = norm_one(rs[k], sd, clip);
            ret[k] = ret[k] * (double)ms[k];
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NC; ++k)
    if (own[k]) a.state[3 + col[k]] = ret[k];
  if (threadIdx.x == 0) {
    a.state[0] = mean;
    a.state[1] = var;
    a.state[2] = count;
  }
}

// update == 0: the stored var; column by column as the walk, so that a thread writes the columns it owns
__device__ __forceinline__ void norm_frozen(const NormArgs& a) {
  const int T = a.T, N = a.N;
  const double sd = sqrt(a.state[1] + (double)a.eps), clip = (double)a.clip;
  for (int n = threadIdx.x; n < N; n += 256)
    for (int sb = a.s0; sb < T; sb += GAE_BATCH) {
      float r[GAE_BATCH];
#pragma unroll
      for (int j = 0; j < GAE_BATCH; ++j) r[j] = a.rewards[min(sb + j, T - 1) * N + n];
#pragma unroll
      for (int j = 0; j < GAE_BATCH; ++j)
        if (sb + j < T) a.out[(sb + j) * N + n] = norm_one(r[j], sd, clip);
    }
}

__device__ __forceinline__ void norm_body(const NormArgs& a, double* red_m, double* red_q, double* bc) {
  if (a.s0 >= a.T) return;                  // no row to normalise: nothing is read or written
  if (!a.update) norm_frozen(a);
  else if (a.N <= 256) norm_walk<1>(a, red_m, red_q, bc);
  else if (a.N <= 512) norm_walk<2>(a, red_m, red_q, bc);
  else norm_walk<4>(a, red_m, red_q, bc);
}

__global__ __launch_bounds__(256) void reward_normalize_kernel(NormArgs a) {
  __shared__ double red_m[4], red_q[4], bc[3];
  norm_body(a, red_m, red_q, bc);
}

// g.rewards is n.out: the scan reads what the walk wrote (the file's header comment: a thread reads back its own columns only)
__global__ __launch_bounds__(256) void gae_returns_normalized_kernel(NormArgs n, GaeArgs g, int use_gae) {
  __shared__ double red_m[4], red_q[4], bc[3], red_sum[4], red_sq[4];
  norm_body(n, red_m, red_q, bc);
  if (use_gae) gae_body<true>(g, red_sum, red_sq);
  else gae_body<false>(g, red_sum, red_sq);
}

bool norm_args_ok(const float* rewards, const float* masks, const double* state, const float* out, int T, int N, int s0) {
  if (!rewards || !masks || !state || !out) return false;
  return T >= 1 && N >= 1 && N <= GAE_MAXN && (long long)T * N < GAE_MAXTN && s0 >= 0 && s0 <= T;
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

extern "C" int wsmg_reward_normalize(const float* rewards, const float* masks, double* state, float gamma, float clip, float eps,
                                     int T, int N, int first_row, int update, float* rewards_norm, wsmg_stream_t stream) {
  if (!norm_args_ok(rewards, masks, state, rewards_norm, T, N, first_row)) return WSMG_EINVAL;
  if (first_row == T) return 0;             // no row: no launch
  NormArgs n{rewards, masks, state, rewards_norm, gamma, eps, clip, T, N, first_row, update};
  hipLaunchKernelGGL(reward_normalize_kernel, dim3(1), dim3(256), 0, wsmg_s(stream), n);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_gae_returns_normalized(const float* rewards, const float* masks, double* state, float norm_gamma, float clip,
                                           float norm_eps, int first_row, int update, float* rewards_norm, float* value_preds,
                                           const float* next_value, float gamma, float gamma_tau, int use_gae, int T, int N,
                                           float* returns, float* adv, float* adv_norm, double* stats, float eps,
                                           wsmg_stream_t stream) {
  if (!norm_args_ok(rewards, masks, state, rewards_norm, T, N, first_row)) return WSMG_EINVAL;
  if (!value_preds || !next_value || !returns) return WSMG_EINVAL;
  NormArgs n{rewards, masks, state, rewards_norm, norm_gamma, norm_eps, clip, T, N, first_row, update};
  GaeArgs g{rewards_norm, value_preds, masks, next_value, gamma, gamma_tau, T, N, returns, adv, adv_norm, stats, eps};
  hipLaunchKernelGGL(gae_returns_normalized_kernel, dim3(1), dim3(256), 0, wsmg_s(stream), n, g, use_gae);
  WSMG_RETURN_LAUNCH();
}
