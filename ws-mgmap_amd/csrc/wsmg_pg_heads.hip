// The policy-gradient side of the heads: what `evaluate_actions` and a PPO / A2C update need after the second recurrence, as four
// launches instead of the ≈45 each way of DiagGaussian + Normal + CriticHead + a host-written clipped-surrogate loss.
//
// habitat's `Policy.evaluate_actions` (the reference's policy has `act` only) evaluates, on features [B, K]:
//
//   eval_heads_fwd_kernel   mean = x Wm^T + bm,  sigma = exp(logstd),  value = x Wc^T + bc,
//                           logp[b]  = sum_a( -(action - mean)^2 / (2 sigma^2) - logstd_a - 0.5 log(2 pi) )   (distributions.py:21-29)
//                           entropy  = sum_a( 0.5 + 0.5 log(2 pi) + logstd_a )        (the same for every row: also the batch mean)
//   eval_heads_bwd_kernel   d mean = d logp (action - mean) / sigma^2,   d logstd_a = sum_b d logp_b ((action - mean)^2 / sigma^2 - 1) + d entropy,
//                           d x, d Wm, d bm, d Wc, d bc as update_heads_bwd_kernel forms them (wsmg_heads_common.h)
//   ppo_loss_fwd_kernel     habitat-baselines' PPO.update: ratio = exp(logp - old_logp), action_loss = -mean(min(ratio adv, clamp(ratio) adv)),
//                           value_loss = 0.5 mean(max((v - ret)^2, (v_clipped - ret)^2)) or 0.5 mean((ret - v)^2),
//                           loss = value_coef value_loss + action_loss - entropy_coef entropy;  + clip fraction and approximate KL
//   ppo_loss_fwd_gated_kernel   the same forward (ppo_loss_rows, written once) behind a KL gate record: closes the gate when
//                           approx_kl > limit, and while it is open adds the five figures to a device `sums` and counts the step
//   ppo_loss_bwd_kernel     d logp, d value, d entropy from d loss, with torch autograd's conventions at ties and clamp edges
//
// float32 throughout; every sum in a fixed order, no atomics (the same bits every run); the rows a mask leaves out are DROPPED from
// the means (selected), not multiplied by zero, as aux_reduce_fwd_kernel does.
// The two heads kernels' row projection and column-owned backward are wsmg_heads_common.h's, shared with wsmg_heads.hip.
#include "wsmg_heads_common.h"

namespace {

constexpr int PPO_MAXB = 1 << 20;          // rows one workgroup walks (4096 per thread); a PPO minibatch is 10^2 .. 10^4

struct EvalFwd {
  const float* x;        // [B][K]
  const float* wm;       // [A][K]
  const float* bm;       // [A]
  const float* logstd;   // [A]
  const float* wc;       // [K]
  const float* bc;       // [1]
  const float* action;   // [B][A]
  float* value;          // [B]
  float* logp;           // [B]
  float* mean;           // [B][A]
  float* entropy;        // [1]
  int B, K, A;
};

// one wave per row (heads_row_dots); lane 0 adds the biases and the log-probability, thread 0 of the grid the entropy
__global__ __launch_bounds__(256) void eval_heads_fwd_kernel(EvalFwd a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float e = 0.f;
    for (int o = 0; o < a.A; ++o) e += (0.5f + HALF_LOG_2PI) + a.logstd[o];
    a.entropy[0] = e;
  }
  const int b = blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  float s[HEADS_MAXA + 1];
  heads_row_dots(a.x + (size_t)b * a.K, a.wm, a.wc, a.K, a.A, lane, s);
  if (lane == 0) {
    float lp = 0.f;
#pragma unroll
    for (int o = 0; o < HEADS_MAXA; ++o)
      if (o < a.A) {
        const float m = s[o] + a.bm[o];
        a.mean[(size_t)b * a.A + o] = m;
        const float ls = a.logstd[o];
        const float sigma = expf(ls);
        const float d = a.action[(size_t)b * a.A + o] - m;
        lp += (-(d * d) / (2.f * (sigma * sigma)) - ls) - HALF_LOG_2PI;
      }
    a.logp[b] = lp;
    a.value[b] = s[HEADS_MAXA] + a.bc[0];
  }
}

struct EvalBwd {
  const float* x;        // [B][K]
  const float* wm;       // [A][K]
  const float* wc;       // [K]
  const float* logstd;   // [A]
  const float* action;   // [B][A]
  const float* mean;     // [B][A]
  const float* dvalue;   // [B] or null
  const float* dlogp;    // [B] or null
  const float* dentropy; // [1] or null
  float* dx;             // [B][K]
  float* dwm;            // [A][K]
  float* dbm;            // [A]
  float* dlogstd;        // [A]
  float* dwc;            // [K]
  float* dbc;            // [1]
  int B, K, A;
};

// The column-owned backward (heads_bwd_columns) with this row: g_o[b] = d mean[b][o] and d value[b]; HEADS_MAXA extra row sums, the
// rows' terms of d logstd.  Row sums: d bm [HEADS_MAXA], d bc, d logstd [HEADS_MAXA] (+ d entropy, the same for every dimension).
struct EvalHeadsRow {
  static constexpr int NX = HEADS_MAXA;
  float ivar[HEADS_MAXA];        // 1 / sigma^2
  __device__ explicit EvalHeadsRow(const EvalBwd& a) {
#pragma unroll
    for (int o = 0; o < HEADS_MAXA; ++o) {
      const float sigma = o < a.A ? expf(a.logstd[o]) : 1.f;
      ivar[o] = 1.f / (sigma * sigma);
    }
  }
  __device__ void fill(const EvalBwd& a, int b, float (&go)[HEADS_MAXA + 1], float (&gl)[HEADS_MAXA]) const {
    const float dl = a.dlogp ? a.dlogp[b] : 0.f;
#pragma unroll
    for (int o = 0; o < HEADS_MAXA; ++o) {
      go[o] = 0.f; gl[o] = 0.f;
      if (o < a.A && a.dlogp) {
        const float d = a.action[(size_t)b * a.A + o] - a.mean[(size_t)b * a.A + o];
        go[o] = dl * d * ivar[o];
        gl[o] = dl * (d * d * ivar[o] - 1.f);
      }
    }
    go[HEADS_MAXA] = a.dvalue ? a.dvalue[b] : 0.f;
  }
  static __device__ void store(const EvalBwd& a, int o, float s) {
    if (o < HEADS_MAXA) { if (o < a.A) a.dbm[o] = s; }
    else if (o == HEADS_MAXA) a.dbc[0] = s;
    else if (o - HEADS_MAXA - 1 < a.A) a.dlogstd[o - HEADS_MAXA - 1] = s + (a.dentropy ? a.dentropy[0] : 0.f);
  }
};

__global__ __launch_bounds__(256) void eval_heads_bwd_kernel(EvalBwd a) { heads_bwd_columns<EvalHeadsRow>(a, a.wc, a.dwc); }

struct PpoRows {
  const float* logp;       // [B]
  const float* old_logp;   // [B]
  const float* adv;        // [B]
  const float* value;      // [B]
  const float* old_value;  // [B]
  const float* ret;        // [B]
  const unsigned char* mask;   // [B] (bool) or null: every row
  float clip, value_coef, entropy_coef;
  int clipped_value, B;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// THE forward, for both kernels below.  One workgroup.  Thread t adds the terms of rows t, t + 256, ... (chunks of 256 rows, in row
// order), then the 256 partial sums are added by the wave butterfly and the four waves in order: the order never depends on anything
// but B.  Thread 0 stores out[0..5) and nsel and gets the five figures back in the order the trainer sums them, {value_loss,
// action_loss, entropy, clip_frac, approx_kl}: the very floats it stored (fig is written by thread 0 only).
__device__ __forceinline__ void ppo_loss_rows(const PpoRows& a, const float* __restrict__ entropy, float* __restrict__ out,
                                              float* __restrict__ nsel, float (&fig)[5]) {
  __shared__ float red[4];
  float n = 0.f, sa = 0.f, sv = 0.f, sc = 0.f, sk = 0.f;
  const float lo = 1.f - a.clip, hi = 1.f + a.clip;
  for (int b = threadIdx.x; b < a.B; b += 256) {
    if (a.mask && !a.mask[b]) continue;
    const float dl = a.logp[b] - a.old_logp[b];
    const float ratio = expf(dl);
    const float s1 = ratio * a.adv[b], s2 = clampf(ratio, lo, hi) * a.adv[b];
    const float v = a.value[b], r = a.ret[b];
    float vl = (r - v) * (r - v);
    if (a.clipped_value) {
      const float vc = a.old_value[b] + clampf(v - a.old_value[b], -a.clip, a.clip);
      const float l1 = (v - r) * (v - r), l2 = (vc - r) * (vc - r);
      vl = l1 > l2 ? l1 : l2;
    }
    n += 1.f;
    sa += s1 < s2 ? s1 : s2;
    sv += vl;
    sc += fabsf(ratio - 1.f) > a.clip ? 1.f : 0.f;
    sk -= dl;
  }
  n = block_sum(n, red);
  sa = block_sum(sa, red);
  sv = block_sum(sv, red);
  sc = block_sum(sc, red);
  sk = block_sum(sk, red);
  if (threadIdx.x == 0) {
    const float action = -(sa / n), vloss = 0.5f * (sv / n);     // (an empty selection is NaN, as aux_reduce's is)
    const float ent = entropy[0], frac = sc / n, kl = sk / n;
    out[0] = a.value_coef * vloss + action - a.entropy_coef * ent;
    out[1] = action;
    out[2] = vloss;
    out[3] = frac;
    out[4] = kl;
    nsel[0] = n;
    fig[0] = vloss; fig[1] = action; fig[2] = ent; fig[3] = frac; fig[4] = kl;
  }
}

__global__ __launch_bounds__(256) void ppo_loss_fwd_kernel(PpoRows a, const float* __restrict__ entropy, float* __restrict__ out,
                                                           float* __restrict__ nsel) {
  float fig[5];
  ppo_loss_rows(a, entropy, out, nsel, fig);
}

// The same forward behind a KL gate (Spinning Up's early stop, decided on the device).  gate is a record of WSMG_KL_GATE floats that
// the host zeroes at the start of an update and nothing but this kernel writes:
//   gate[KL_STOPPED]     0, or 1 from the first call whose approx_kl > limit until the host clears it (a NaN never sets it)
//   gate[KL_TAKEN]       calls that found and left the gate open: the steps an optimizer behind the gate takes
//   gate[KL_SEEN]        calls since the record was cleared: the ordinal of the next minibatch
//   gate[KL_STOP_ORD]    the ordinal of the call that closed the gate    gate[KL_STOP_KL]  its approx_kl        (both 0 while it is open)
//   gate[5..8)           not written
// While the gate is open after this call's decision, sums[i] += fig[i] (float32, one rounding each: what `sums += stack(figures)` of
// the trainer rounds).  The call that closes the gate adds nothing, and neither does any call after it.  Every word above is a plain
// store of thread 0 behind the reduction: no atomics, nothing another workgroup reads in this launch.  Counters are float32 integers
// (exact below 2^24).
enum { KL_STOPPED = 0, KL_TAKEN = 1, KL_SEEN = 2, KL_STOP_ORD = 3, KL_STOP_KL = 4 };

__global__ __launch_bounds__(256) void ppo_loss_fwd_gated_kernel(PpoRows a, const float* __restrict__ entropy, float limit,
                                                                 float* __restrict__ out, float* __restrict__ nsel,
                                                                 float* __restrict__ gate, float* __restrict__ sums) {
  float fig[5];
  ppo_loss_rows(a, entropy, out, nsel, fig);
  if (threadIdx.x == 0) {
    const float seen = gate[KL_SEEN];
    bool stopped = gate[KL_STOPPED] != 0.f;
    if (!stopped && fig[4] > limit) {
      stopped = true;
      gate[KL_STOPPED] = 1.f;
      gate[KL_STOP_ORD] = seen;
      gate[KL_STOP_KL] = fig[4];
    }
    if (!stopped) {
#pragma unroll
      for (int i = 0; i < 5; ++i) sums[i] = sums[i] + fig[i];
      gate[KL_TAKEN] += 1.f;
    }
    gate[KL_SEEN] = seen + 1.f;
  }
}

// torch autograd's conventions, node by node: min / max of two EQUAL terms give each half of the gradient (both halves reach the
// same input here, so inside the clip range it arrives whole), the term that loses gets an exact 0; clamp passes the gradient on its
// closed interval and an exact 0 outside.  The masked mean's gradient is w_b * (d loss / n) with w_b the 0 / 1 selection: a row left
// out gets 0, and with NO row selected 0 * inf = NaN wherever a product carries it (not where a lost branch put an exact 0).
__global__ __launch_bounds__(256) void ppo_loss_bwd_kernel(PpoRows a, const float* __restrict__ nsel, const float* __restrict__ dloss,
                                                           float* __restrict__ dlogp, float* __restrict__ dvalue,
                                                           float* __restrict__ dentropy) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b == 0) dentropy[0] = -a.entropy_coef * dloss[0];
  if (b >= a.B) return;
  const float w = (a.mask && !a.mask[b]) ? 0.f : 1.f;
  const float ga = (-dloss[0] / nsel[0]) * w;                             // into min(s1, s2)
  const float gv = ((a.value_coef * dloss[0]) * 0.5f / nsel[0]) * w;      // into the squared value error
  const float lo = 1.f - a.clip, hi = 1.f + a.clip;
  const float ratio = expf(a.logp[b] - a.old_logp[b]), adv = a.adv[b];
  const float s1 = ratio * adv, s2 = clampf(ratio, lo, hi) * adv;
  const float g1 = s1 > s2 ? 0.f : (s1 == s2 ? 0.5f * ga : ga);
  const float g2 = s1 < s2 ? 0.f : (s1 == s2 ? 0.5f * ga : ga);
  const float gr = g1 * adv + ((ratio >= lo && ratio <= hi) ? g2 * adv : 0.f);
  dlogp[b] = gr * ratio;
  const float v = a.value[b], r = a.ret[b];
  if (a.clipped_value) {
    const float dv = v - a.old_value[b];
    const float vc = a.old_value[b] + clampf(dv, -a.clip, a.clip);
    const float l1 = (v - r) * (v - r), l2 = (vc - r) * (vc - r);
    const float h1 = l1 < l2 ? 0.f : (l1 == l2 ? 0.5f * gv : gv);
    const float h2 = l1 > l2 ? 0.f : (l1 == l2 ? 0.5f * gv : gv);
    dvalue[b] = h1 * (2.f * (v - r)) + ((dv >= -a.clip && dv <= a.clip) ? h2 * (2.f * (vc - r)) : 0.f);
  } else {
    dvalue[b] = gv * (2.f * (v - r));
  }
}

}  // namespace

extern "C" int wsmg_eval_heads_fwd(const float* x, const float* wm, const float* bm, const float* logstd, const float* wc,
                                   const float* bc, const float* action, int B, int K, int A, float* value, float* logp, float* mean,
                                   float* entropy, wsmg_stream_t stream) {
  if (!x || !wm || !bm || !logstd || !wc || !bc || !action || !value || !logp || !mean || !entropy) return WSMG_EINVAL;
  if (B <= 0 || K <= 0 || (K & 3) || A <= 0 || A > HEADS_MAXA) return WSMG_EINVAL;
  EvalFwd a{x, wm, bm, logstd, wc, bc, action, value, logp, mean, entropy, B, K, A};
  hipLaunchKernelGGL(eval_heads_fwd_kernel, dim3((unsigned)wsmg_cdiv(B, 4)), dim3(256), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_eval_heads_bwd(const float* x, const float* wm, const float* wc, const float* logstd, const float* action,
                                   const float* mean, const float* dvalue, const float* dlogp, const float* dentropy, int B, int K,
                                   int A, float* dx, float* dwm, float* dbm, float* dlogstd, float* dwc, float* dbc,
                                   wsmg_stream_t stream) {
  if (!x || !wm || !wc || !logstd || !action || !mean || !dx || !dwm || !dbm || !dlogstd || !dwc || !dbc) return WSMG_EINVAL;
  if (B <= 0 || K <= 0 || (K & 3) || A <= 0 || A > HEADS_MAXA) return WSMG_EINVAL;
  EvalBwd a{x, wm, wc, logstd, action, mean, dvalue, dlogp, dentropy, dx, dwm, dbm, dlogstd, dwc, dbc, B, K, A};
  hipLaunchKernelGGL(eval_heads_bwd_kernel, dim3((unsigned)wsmg_cdiv(K, 8)), dim3(256), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_ppo_loss_fwd(const float* logp, const float* old_logp, const float* adv, const float* value,
                                 const float* old_value, const float* ret, const unsigned char* mask, const float* entropy, float clip,
                                 float value_coef, float entropy_coef, int clipped_value, int B, float* out5, float* nsel,
                                 wsmg_stream_t stream) {
  if (!logp || !old_logp || !adv || !value || !old_value || !ret || !entropy || !out5 || !nsel) return WSMG_EINVAL;
  if (B <= 0 || B > PPO_MAXB) return WSMG_EINVAL;
  PpoRows a{logp, old_logp, adv, value, old_value, ret, mask, clip, value_coef, entropy_coef, clipped_value, B};
  hipLaunchKernelGGL(ppo_loss_fwd_kernel, dim3(1), dim3(256), 0, wsmg_s(stream), a, entropy, out5, nsel);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_ppo_loss_fwd_gated(const float* logp, const float* old_logp, const float* adv, const float* value,
                                       const float* old_value, const float* ret, const unsigned char* mask, const float* entropy,
                                       float clip, float value_coef, float entropy_coef, int clipped_value, int B, float kl_limit,
                                       float* out5, float* nsel, float* gate, float* sums5, wsmg_stream_t stream) {
  if (!logp || !old_logp || !adv || !value || !old_value || !ret || !entropy || !out5 || !nsel || !gate || !sums5) return WSMG_EINVAL;
  if (((uintptr_t)gate & 3) || ((uintptr_t)sums5 & 3)) return WSMG_EINVAL;
  if (B <= 0 || B > PPO_MAXB) return WSMG_EINVAL;
  PpoRows a{logp, old_logp, adv, value, old_value, ret, mask, clip, value_coef, entropy_coef, clipped_value, B};
  hipLaunchKernelGGL(ppo_loss_fwd_gated_kernel, dim3(1), dim3(256), 0, wsmg_s(stream), a, entropy, kl_limit, out5, nsel, gate, sums5);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_ppo_loss_bwd(const float* logp, const float* old_logp, const float* adv, const float* value,
                                 const float* old_value, const float* ret, const unsigned char* mask, const float* nsel,
                                 const float* dloss, float clip, float value_coef, float entropy_coef, int clipped_value, int B,
                                 float* dlogp, float* dvalue, float* dentropy, wsmg_stream_t stream) {
  if (!logp || !old_logp || !adv || !value || !old_value || !ret || !nsel || !dloss || !dlogp || !dvalue || !dentropy) return WSMG_EINVAL;
  if (B <= 0 || B > PPO_MAXB) return WSMG_EINVAL;
  PpoRows a{logp, old_logp, adv, value, old_value, ret, mask, clip, value_coef, entropy_coef, clipped_value, B};
  hipLaunchKernelGGL(ppo_loss_bwd_kernel, dim3((unsigned)wsmg_cdiv(B, 256)), dim3(256), 0, wsmg_s(stream), a, nsel, dloss, dlogp, dvalue,
                     dentropy);
  WSMG_RETURN_LAUNCH();
}
