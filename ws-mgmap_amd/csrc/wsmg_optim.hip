// Adam step over a LIST of parameter tensors in a few launches (the update's optimizer step: `torch.optim.Adam` constructed at
// common_trainer.py:67-69 and stepped at dagger_trainer.py:540-541 in the reference).
//
// The policy has 102 live parameter tensors, 8.1 M floats: read p, g, m, v and write p, m, v = 227 MB, 45 us at HBM speed.
// The stock multi-tensor implementation is 15 launches and 0.25 ms of GPU time per step (0.5 ms when issued back to back).
// Here a launch carries a table of up to 48 tensors in its kernel arguments; a workgroup owns 4 096 consecutive elements
// of one tensor (16-byte accesses when all four pointers are 16-byte aligned) and finds its tensor by a search over the
// table's block prefix.  Arithmetic as torch.optim.Adam (amsgrad = False, maximize = False), in its order:
//     g' = g + wd p;  m += (1 - b1) (g' - m);  v = b2 v + (1 - b2) g' g';  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
// and, through the _ext entry points (flags WSMG_ADAM_*), torch's amsgrad = True (a fifth array, max_exp_avg_sq, whose running
// maximum of v replaces v under the root), maximize = True (g' = -g) and the decoupled weight decay of torch.optim.AdamW
// (p *= 1 - lr wd in front of the moments, no wd p in g').
//
// ONE element step (adam1), ONE table of chunks (ChunkTable, chunk_tensor + locate_chunk, for_each_batch on the host), ONE descriptor check
// (check_descs, before an entry point's first launch), and four front ends that differ in where the step's inputs come from:
//   wsmg_adam_step_multi          hyper-parameters and bias corrections by value
//   wsmg_adam_step_multi_dev      the step COUNT from device memory (a captured HIP graph freezes kernel arguments)
//   wsmg_adam_step_multi_guarded  the _dev form behind the guard record {norm, coef, skip, skipped} of wsmg_grad_norm_multi:
//                                 grad_sumsq_multi_kernel writes one float64 sum of squares per workgroup (same table, same 4 096-
//                                 element ownership, no atomics), grad_guard_finalize_kernel adds them in a fixed order and writes the
//                                 record and the step count, and the step returns before its first load when `skip` is set and reads
//                                 g * coef otherwise (torch.nn.utils.clip_grad_norm_'s arithmetic, without writing the gradients)
//   wsmg_adam_step_multi_hyper    the _dev / _guarded form with lr, betas, eps, weight_decay (and wsmg_grad_norm_multi_hyper with
//                                 max_grad_norm) read from a float32 record in device memory that the host refreshes between replays
//                                 (wsmgmap.optim.Adam(hyper_on_device=True).sync_hyper()); no kernel writes the record
//   wsmg_adam_step_multi{,_dev,_guarded,_hyper}_ext   the same four behind kernels of their own (adam_multi_ext_kernel<GUARD, HYPER,
//                                 AMSGRAD>): `flags` and the decay factor travel as wave-uniform kernel arguments, max_exp_avg_sq as
//                                 a parallel host array of pointers.  The four kernels above are compiled from the same element step
//                                 and chunk walk with the options off at compile time: not one of their instructions knows of them.
//   wsmg_grad_norm_multi{,_hyper}_gated   the guard's finalize behind an external gate word (grad_guard_finalize_gated_kernel): a
//                                 non-zero gate[0] forces the skip — the element kernels above do not change, they read the flag.
// No host synchronisation anywhere.
#include "wsmg_common.h"

namespace {

// ADAM_MAX = 48 tensors per launch (kernel-argument table): wsmg_common.h
constexpr int ADAM_CHUNK = 4096;  // elements per workgroup
// The hyper record (include/wsmgmap.h): one 8-float row per parameter group, then the guard's row.
enum { HYPER_LR = 0, HYPER_BETA1 = 1, HYPER_BETA2 = 2, HYPER_EPS = 3, HYPER_WD = 4, HYPER_MAX_NORM = 0 };

// The tensors of one launch and the workgroups that own their chunks; every batch struct below embeds it and adds its pointers.
struct ChunkTable {
  int first_block[ADAM_MAX + 1];  // prefix of workgroups per tensor
  long long n[ADAM_MAX];
  int count;
};

struct Chunk { int tensor; long long i0, i1; };   // elements [i0, i1) of table entry `tensor`

// This workgroup's tensor: t with first_block[t] <= blockIdx.x < first_block[t + 1].
__device__ __forceinline__ int chunk_tensor(const ChunkTable& tb) {
  int lo = 0, hi = tb.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= tb.first_block[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// This workgroup's chunk, (tensor, i0, i1): its 4 096 elements of its tensor.  Callers that pass t = chunk_tensor(tb) have loaded
// their pointers of entry t in between, so that those loads and the table's are issued together.
__device__ __forceinline__ Chunk locate_chunk(const ChunkTable& tb, int t) {
  const long long n = tb.n[t];
  const long long i0 = (long long)((int)blockIdx.x - tb.first_block[t]) * ADAM_CHUNK;
  return {t, i0, i0 + ADAM_CHUNK < n ? i0 + ADAM_CHUNK : n};
}

// A read-only walk over a chunk of a gradient: f(g[i]) for this thread's elements, in the order the float64 sums depend on —
// 16-byte loads of an aligned gradient with j = 0..3 in order, then the scalar tail; a misaligned gradient element by element.
template <class F>
__device__ __forceinline__ void walk_grad(const float* __restrict__ g, long long i0, long long i1, F f) {
  if (((uintptr_t)g & 15) == 0) {
    const long long nv = i0 + ((i1 - i0) & ~3ll);
    for (long long i = i0 + 4 * (long long)threadIdx.x; i < nv; i += 4 * 256) {
      const f32x4 gg = ld4(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) f(gg[j]);
    }
    for (long long i = nv + threadIdx.x; i < i1; i += 256) f(g[i]);
  } else {
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) f(g[i]);
  }
}

struct AdamHyper {         // what the element step reads: 1 - beta1, beta2, 1 - beta2, eps, weight_decay
  float beta1c, beta2, beta2c, eps, wd;
};

struct AdamBatch {
  float* p[ADAM_MAX];
  const float* g[ADAM_MAX];
  float* m[ADAM_MAX];
  float* v[ADAM_MAX];
  ChunkTable tab;
  AdamHyper h;             // by value (the _hyper kernels derive theirs from the record's row and ignore this one, lr and beta1)
  float lr_bc1, sqrt_bc2;  // by value, when step_dev is null
  const float* step_dev;   // or null: the step count lives on the device (HIP-graph replay: the arguments are frozen at capture) and
  float lr, beta1;         //          the bias corrections are computed from it in the kernel
  const float* guard;      // or null: the guard record of grad_guard_finalize_kernel (read by the guarded kernels only)
  const float* hyper;      // or null: this group's row of the hyper record {lr, beta1, beta2, eps, weight_decay, 0, 0, 0} (read by the
};                         //          _hyper kernels only)

// What the _ext kernels add to a batch: the fifth array of every table entry (read only when AMSGRAD) and the options, the same for
// every lane.  decay = (float)(1.0 - (double)lr * (double)wd), by value (the _hyper kernels form theirs from the record's row).
struct AdamExt {
  float* vmax[ADAM_MAX];
  int flags;               // WSMG_ADAM_MAXIMIZE | WSMG_ADAM_DECOUPLED_WD (WSMG_ADAM_AMSGRAD chose the kernel)
  float decay;
};

struct AdamExtBatch {
  AdamBatch b;
  AdamExt e;
};

struct AdamOpts {          // the element step's view of them
  bool maximize, decoupled;
  float decay;
};

// THE element step.  These forms define it, rounding by rounding, for every front end; nothing else may be contracted:
//     g' = coef g (GUARD only: a product of its own)
//     g' = -g' (maximize: exact; behind the guard's product, so the clip acts on the same norm)
//     wd != 0, the L2 form:        g' = fma(wd, p, g'), behind the negation as in torch
//     wd != 0, the decoupled form: p  = p * decay, decay = (float)(1.0 - (double)lr * (double)wd): one product, in front of the
//                                  moments (torch.optim.AdamW's param.mul_(1 - lr * weight_decay)); g' is left alone
//     m  = fma(1 - b1, g' - m, m)
//     v  = fma(v, b2, ((1 - b2) g') g') in the 16-byte loop (VEC),  fma(g', (1 - b2) g', v b2) in the two scalar loops
//     amsgrad: vmax = (v > vmax || v != v) ? v : vmax (exact; a NaN in v or in vmax stays, as torch.maximum keeps it and fmaxf
//              would not), and vmax stands for v in the next line
//     p  = fma(-lr_bc1, m / (sqrt(v) / sqrt_bc2 + eps), p)
// The two forms of v round differently and which loop an element meets is fixed by its address and index, so both are part of the
// definition: a step's bits do not depend on the front end, the compiler's contraction choices or the layout of AdamBatch.
// tests/test_gpu_adam_hyper.py compares the front ends' bits on every path, tests/test_gpu_adam_variants.py those of the options.
// EXT = false (the four kernels without options) compiles the three options out: `o` and `vmax` are then not read.
template <bool GUARD, bool VEC, bool EXT, bool AMSGRAD>
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float& vmax, const AdamHyper& h, float lr_bc1,
                                      float sqrt_bc2, float coef, const AdamOpts& o) {
#pragma clang fp contract(off)
  if (GUARD) g *= coef;
  if (EXT && o.maximize) g = -g;
  if (h.wd != 0.f) {
    if (EXT && o.decoupled) p = p * o.decay;
    else g = fmaf(h.wd, p, g);
  }
  m = fmaf(h.beta1c, g - m, m);
  const float gc = h.beta2c * g;
  v = VEC ? fmaf(v, h.beta2, gc * g) : fmaf(g, gc, v * h.beta2);
  float s = v;
  if (AMSGRAD) {
    vmax = (v > vmax || v != v) ? v : vmax;
    s = vmax;
  }
  const float denom = sqrtf(s) / sqrt_bc2 + h.eps;
  p = fmaf(-lr_bc1, m / denom, p);
}

// One workgroup's 4 096 elements of its tensor (a loop nest of its own: it loads and stores four arrays, five with AMSGRAD, whose
// address then joins the test for the 16-byte loop).  e is read only when EXT.
template <bool GUARD, bool EXT, bool AMSGRAD>
__device__ __forceinline__ void adam_chunk(const AdamBatch& b, const AdamExt* e, const AdamHyper& h, float lr_bc1, float sqrt_bc2,
                                           float coef, const AdamOpts& o) {
  const int t = chunk_tensor(b.tab);
  float* __restrict__ p = b.p[t];
  const float* __restrict__ g = b.g[t];
  float* __restrict__ m = b.m[t];
  float* __restrict__ v = b.v[t];
  float* __restrict__ x = AMSGRAD ? e->vmax[t] : nullptr;
  const Chunk c = locate_chunk(b.tab, t);
  const long long i0 = c.i0, i1 = c.i1;
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)x) & 15) == 0);
  float none = 0.f;        // vmax of a step without AMSGRAD: never read
  if (vec) {
    const long long nv = i0 + ((i1 - i0) & ~3ll);
    for (long long i = i0 + 4 * (long long)threadIdx.x; i < nv; i += 4 * 256) {
      f32x4 pp = ld4(p + i), mm = ld4(m + i), vv = ld4(v + i), xx = {};
      if (AMSGRAD) xx = ld4(x + i);
      const f32x4 gg = ld4(g + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = pp[j], mj = mm[j], vj = vv[j], xj = xx[j];
        adam1<GUARD, true, EXT, AMSGRAD>(pj, gg[j], mj, vj, xj, h, lr_bc1, sqrt_bc2, coef, o);
        pp[j] = pj; mm[j] = mj; vv[j] = vj; xx[j] = xj;
      }
      st4(p + i, pp); st4(m + i, mm); st4(v + i, vv);
      if (AMSGRAD) st4(x + i, xx);
    }
    for (long long i = nv + threadIdx.x; i < i1; i += 256)
      adam1<GUARD, false, EXT, AMSGRAD>(p[i], g[i], m[i], v[i], AMSGRAD ? x[i] : none, h, lr_bc1, sqrt_bc2, coef, o);
  } else {
    for (long long i = i0 + threadIdx.x; i < i1; i += 256)
      adam1<GUARD, false, EXT, AMSGRAD>(p[i], g[i], m[i], v[i], AMSGRAD ? x[i] : none, h, lr_bc1, sqrt_bc2, coef, o);
  }
}

// The front ends.  GUARD reads skip and coef once, before anything else (otherwise the guard pointer is not read).  HYPER reads its
// group's row once, here, through a wave-uniform address, and derives 1 - beta in float as adam_launch does (otherwise the hyper
// pointer is not read and the values are the kernel arguments).  With a device step count the bias corrections are 1 - beta^step in
// double, the host's expressions: equal values give equal bits.  EXT reads the options from e (otherwise e is not read); with HYPER
// the decay factor is formed here from the row's lr and weight_decay, with adam_launch's expression.
template <bool GUARD, bool HYPER, bool EXT = false, bool AMSGRAD = false>
__device__ __forceinline__ void adam_multi(const AdamBatch& b, const AdamExt* e = nullptr) {
  float coef = 1.f;
  if (GUARD) {
    if (b.guard[GUARD_SKIP] != 0.f) return;     // a skipped step: no load of p / m / v / vmax, nothing written
    coef = b.guard[GUARD_COEF];
  }
  AdamOpts o = {false, false, 1.f};
  if (EXT) {
    o.maximize = (e->flags & WSMG_ADAM_MAXIMIZE) != 0;
    o.decoupled = (e->flags & WSMG_ADAM_DECOUPLED_WD) != 0;
    o.decay = e->decay;
  }
  if (HYPER) {
    const float* __restrict__ row = b.hyper;
    const float lr = row[HYPER_LR], beta1 = row[HYPER_BETA1];
    AdamHyper h;
    h.beta2 = row[HYPER_BETA2];
    h.eps = row[HYPER_EPS];
    h.wd = row[HYPER_WD];
    h.beta1c = 1.f - beta1;
    h.beta2c = 1.f - h.beta2;
    const double st = (double)*b.step_dev;
    const float lr_bc1 = (float)((double)lr / (1.0 - pow((double)beta1, st)));
    const float sqrt_bc2 = (float)sqrt(1.0 - pow((double)h.beta2, st));
    if (EXT) o.decay = (float)(1.0 - (double)lr * (double)h.wd);
    adam_chunk<GUARD, EXT, AMSGRAD>(b, e, h, lr_bc1, sqrt_bc2, coef, o);
    return;
  }
  float lr_bc1 = b.lr_bc1, sqrt_bc2 = b.sqrt_bc2;
  if (b.step_dev) {   // 1 - beta^step in double, as the host path does
    const double st = (double)*b.step_dev;
    lr_bc1 = (float)((double)b.lr / (1.0 - pow((double)b.beta1, st)));
    sqrt_bc2 = (float)sqrt(1.0 - pow((double)b.h.beta2, st));
  }
  const AdamHyper h = b.h;
  adam_chunk<GUARD, EXT, AMSGRAD>(b, e, h, lr_bc1, sqrt_bc2, coef, o);
}

__global__ __launch_bounds__(256) void adam_multi_kernel(AdamBatch b) { adam_multi<false, false>(b); }
__global__ __launch_bounds__(256) void adam_multi_guarded_kernel(AdamBatch b) { adam_multi<true, false>(b); }
__global__ __launch_bounds__(256) void adam_multi_hyper_kernel(AdamBatch b) { adam_multi<false, true>(b); }
__global__ __launch_bounds__(256) void adam_multi_guarded_hyper_kernel(AdamBatch b) { adam_multi<true, true>(b); }

// The same four front ends with the options: 2 x 2 x 2 kernels (amsgrad changes the number of arrays; maximize and the decay form are
// wave-uniform branches on kernel arguments).
template <bool GUARD, bool HYPER, bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_multi_ext_kernel(AdamExtBatch x) { adam_multi<GUARD, HYPER, true, AMSGRAD>(x.b, &x.e); }

// ---- the guard: global gradient norm -> {norm, coef, skip, skipped}

struct GradBatch {         // the table's gradients and this launch's slice of the partials: one float64 per workgroup
  const float* g[ADAM_MAX];
  ChunkTable tab;
  double* partials;
};

__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(GradBatch b) {
  __shared__ double red[4];
  const int t = chunk_tensor(b.tab);
  const float* __restrict__ g = b.g[t];
  const Chunk c = locate_chunk(b.tab, t);
  double acc = 0.0;        // float64: gradients of 1e30 square to 1e60, and the sum's order then costs nothing visible in float32
  walk_grad(g, c.i0, c.i1, [&](float x) { acc += (double)x * (double)x; });
  const double sum = block_sum_d(acc, red);
  if (threadIdx.x == 0) b.partials[blockIdx.x] = sum;
}

// One workgroup: every partial of every launch, strided per thread, then the fixed tree.  Finiteness is judged on the float32 norm
// and the clip coefficient is clip_grad_norm_'s (max_norm / (norm + 1e-6), clamped to 1; a NaN norm gives a NaN coefficient there
// too).  The step count advances here, by 1 - skip: a skipped step does not advance the bias corrections.
// GATED (the _gated entry points; compiled out of the two kernels without a gate): a non-zero gate[0] forces the skip whatever the
// norm is.  Such a step is skipped for everything that reads the record — skip is non-zero, skipped advances, the step count does
// not — but it is no finding about the gradients: the record keeps the norm and the coefficient of the last step that was judged,
// and skip is GUARD_SKIP_GATE (2), not 1, which grad_report_latch_kernel does not latch.
constexpr float GUARD_SKIP_GATE = 2.f;

template <bool GATED>
__device__ __forceinline__ void guard_finalize(const double* __restrict__ partials, int total, float max_norm, int skip_nonfinite,
                                               const float* __restrict__ gate, float* __restrict__ guard,
                                               float* __restrict__ step_dev) {
  __shared__ double red[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < total; i += 256) acc += partials[i];
  const double sum = block_sum_d(acc, red);
  if (threadIdx.x == 0) {
    if (GATED && gate[0] != 0.f) {
      guard[GUARD_SKIP] = GUARD_SKIP_GATE;
      guard[GUARD_SKIPPED] += 1.f;
      return;
    }
    const float norm = (float)sqrt(sum);
    float coef = 1.f;
    if (max_norm > 0.f) {
      const float c = max_norm / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;
    }
    const float skip = (skip_nonfinite && !isfinite(norm)) ? 1.f : 0.f;
    guard[GUARD_NORM] = norm;
    guard[GUARD_COEF] = coef;
    guard[GUARD_SKIP] = skip;
    guard[GUARD_SKIPPED] += skip;
    if (step_dev) *step_dev += 1.f - skip;
  }
}

__global__ __launch_bounds__(256) void grad_guard_finalize_kernel(const double* __restrict__ partials, int total, float max_norm,
                                                                   int skip_nonfinite, float* __restrict__ guard,
                                                                   float* __restrict__ step_dev) {
  guard_finalize<false>(partials, total, max_norm, skip_nonfinite, nullptr, guard, step_dev);
}

// max_norm from the hyper record's guard row {max_grad_norm or 0 for "no clipping", 0, ...}: the same sums, arithmetic and writes.
__global__ __launch_bounds__(256) void grad_guard_finalize_hyper_kernel(const double* __restrict__ partials, int total,
                                                                         const float* __restrict__ hyper_guard_row, int skip_nonfinite,
                                                                         float* __restrict__ guard, float* __restrict__ step_dev) {
  guard_finalize<false>(partials, total, hyper_guard_row[HYPER_MAX_NORM], skip_nonfinite, nullptr, guard, step_dev);
}

// Both of the above behind an external gate (a device word that another kernel owns: ppo_loss_fwd_gated_kernel's `stopped`).
// max_norm comes from hyper_guard_row when that is not null, else by value; with gate[0] == 0 the sums, arithmetic and writes are
// those of the kernel without a gate.
__global__ __launch_bounds__(256) void grad_guard_finalize_gated_kernel(const double* __restrict__ partials, int total, float max_norm,
                                                                         const float* __restrict__ hyper_guard_row, int skip_nonfinite,
                                                                         const float* __restrict__ gate, float* __restrict__ guard,
                                                                         float* __restrict__ step_dev) {
  guard_finalize<true>(partials, total, hyper_guard_row ? hyper_guard_row[HYPER_MAX_NORM] : max_norm, skip_nonfinite, gate, guard,
                       step_dev);
}

// ---- the per-tensor gradient report (wsmg_grad_report_multi / wsmg_grad_stats_multi): which tensor made the guard skip
//
// Shape: three kernels behind the norm's launches, none of which the step's own kernels depend on.
//   grad_scan_multi_kernel     grad_sumsq_multi_kernel's ownership and walk (one 256-thread workgroup per 4 096-element chunk,
//                              locate_chunk, walk_grad): max |g| over the finite
//                              elements, NaN count, Inf count of the chunk -> 4 words of the scan workspace, at the chunk's index in
//                              the norm's partials.
//   grad_report_fold_kernel    one workgroup per tensor (ADAM_MAX per launch, table in the kernel arguments): the tensor's float64
//                              partials in guard_finalize's order (thread t adds chunks t, t + 256, ...; block_sum_d), its scan words
//                              -> the report row {(float)sqrt(S), max |g|, NaNs, Infs}.  A tensor without chunks gets a zero row.
//   grad_report_latch_kernel   one workgroup: returns before its first store unless guard[GUARD_SKIP] is 1; otherwise the header
//                              {skipped, attempt, first non-finite tensor, largest norm, non-finite tensors, 0, 0, 0} and a copy of
//                              the report (the rows strided over the threads, the header from thread 0).
// Every reduction is a maximum or an integer sum (any order gives the same bits) or the float64 tree above; no atomics; thread 0 stores
// each chunk record, report row and header with ordinary stores; the only LDS is the reductions' scratch.

struct ScanBatch {         // GradBatch with the scan workspace's slice: four words per workgroup
  const float* g[ADAM_MAX];
  ChunkTable tab;
  uint32_t* scan;
};

struct FoldBatch {         // tensors row0 .. row0 + gridDim.x of the list; first/chunks index the partials and the scan workspace
  int first[ADAM_MAX];
  int chunks[ADAM_MAX];
  int row0;
  const double* partials;
  const uint32_t* scan;
  uint32_t* report;
};

// |g| as its bit pattern, which orders non-negative floats as unsigned integers: above Inf's pattern is NaN
__device__ __forceinline__ void scan1(float g, uint32_t& mx, uint32_t& nan, uint32_t& inf) {
  const uint32_t a = __float_as_uint(g) & 0x7fffffffu;
  if (a > 0x7f800000u) ++nan;
  else if (a == 0x7f800000u) ++inf;
  else mx = a > mx ? a : mx;
}

__device__ __forceinline__ uint32_t wave_max_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// {max, sum, sum} over the workgroup; red holds 12 words (every thread returns the result)
__device__ __forceinline__ void block_scan_reduce(uint32_t& mx, uint32_t& nan, uint32_t& inf, uint32_t* red) {
  mx = wave_max_u(mx); nan = wave_sum_u(nan); inf = wave_sum_u(inf);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[w] = mx; red[4 + w] = nan; red[8 + w] = inf;
  }
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) mx = red[w] > mx ? red[w] : mx;
  nan = red[4] + red[5] + red[6] + red[7];
  inf = red[8] + red[9] + red[10] + red[11];
}

__global__ __launch_bounds__(256) void grad_scan_multi_kernel(ScanBatch b) {
  __shared__ uint32_t red[12];
  const int t = chunk_tensor(b.tab);
  const float* __restrict__ g = b.g[t];
  const Chunk c = locate_chunk(b.tab, t);
  uint32_t mx = 0, nan = 0, inf = 0;
  walk_grad(g, c.i0, c.i1, [&](float x) { scan1(x, mx, nan, inf); });
  block_scan_reduce(mx, nan, inf, red);
  if (threadIdx.x == 0) {
    uint32_t* __restrict__ out = b.scan + 4 * (long long)blockIdx.x;
    out[0] = mx; out[1] = nan; out[2] = inf; out[3] = 0u;
  }
}

__global__ __launch_bounds__(256) void grad_report_fold_kernel(FoldBatch b) {
  __shared__ double red[4];
  __shared__ uint32_t ured[12];
  const int first = b.first[blockIdx.x], chunks = b.chunks[blockIdx.x];
  const double* __restrict__ partials = b.partials + first;
  const uint32_t* __restrict__ scan = b.scan + 4 * (long long)first;
  double acc = 0.0;
  uint32_t mx = 0, nan = 0, inf = 0;
  for (int i = threadIdx.x; i < chunks; i += 256) {
    acc += partials[i];
    const uint32_t m = scan[4 * (long long)i];
    mx = m > mx ? m : mx;
    nan += scan[4 * (long long)i + 1];
    inf += scan[4 * (long long)i + 2];
  }
  const double sum = block_sum_d(acc, red);
  block_scan_reduce(mx, nan, inf, ured);
  if (threadIdx.x == 0) {
    uint32_t* __restrict__ row = b.report + 4 * ((long long)b.row0 + blockIdx.x);
    row[0] = __float_as_uint((float)sqrt(sum));
    row[1] = mx; row[2] = nan; row[3] = inf;
  }
}

__device__ __forceinline__ unsigned long long wave_max_ull(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// The largest norm as the maximum of (key << 32 | ~i): key is the norm's bit pattern (norms are >= +0, so the patterns order as the
// values do) or 0xffffffff for a NaN, and the complemented index makes the lowest i win a tie.  No row at all gives i = 0xffffffff.
__global__ __launch_bounds__(256) void grad_report_latch_kernel(const uint32_t* __restrict__ report, int n,
                                                                const float* __restrict__ guard, const float* __restrict__ step_dev,
                                                                uint32_t* __restrict__ latch) {
  __shared__ unsigned long long bred[4];
  __shared__ uint32_t ured[12];
  // a step that was taken (0), or one that an external gate skipped (GUARD_SKIP_GATE: the latch names a non-finite gradient, and
  // such a skip has none): not one byte of the latch is stored
  if (guard[GUARD_SKIP] != 1.f) return;
  unsigned long long best = 0ull;
  uint32_t notfirst = 0, bad = 0, unused = 0;    // notfirst = ~(lowest non-finite i): a maximum, as block_scan_reduce takes it
  for (int i = threadIdx.x; i < n; i += 256) {
    const uint32_t w0 = report[4 * (long long)i];
    const uint32_t key = (w0 & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : w0;
    const unsigned long long cand = ((unsigned long long)key << 32) | (uint32_t)~(uint32_t)i;
    best = cand > best ? cand : best;
    if (report[4 * (long long)i + 2] + report[4 * (long long)i + 3] != 0u) {     // (counts of one tensor sum below 2^32: n < 2^32)
      ++bad;
      const uint32_t c = ~(uint32_t)i;
      notfirst = c > notfirst ? c : notfirst;
    }
  }
  best = wave_max_ull(best);
  if ((threadIdx.x & 63) == 0) bred[threadIdx.x >> 6] = best;
  block_scan_reduce(notfirst, bad, unused, ured);          // (its barrier also publishes bred)
  for (long long i = threadIdx.x; i < 4ll * n; i += 256) latch[8 + i] = report[i];
  if (threadIdx.x == 0) {
    best = bred[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) best = bred[w] > best ? bred[w] : best;
    const uint32_t skipped = (uint32_t)guard[GUARD_SKIPPED];
    latch[0] = skipped;
    latch[1] = (uint32_t)*step_dev + skipped;
    latch[2] = ~notfirst;                        // nothing non-finite: ~0
    latch[3] = ~(uint32_t)best;
    latch[4] = bad;
    latch[5] = 0u; latch[6] = 0u; latch[7] = 0u;
  }
}

}  // namespace

// ---- the host side: one descriptor check, one batching loop

// What an entry point needs of a descriptor with n > 0 (of every one: 0 <= n <= max_n).
enum { DESC_GRAD = 0, DESC_ALL = 1, DESC_ALIGN4 = 2, DESC_VMAX = 4 };   // grad only / all four pointers; | DESC_ALIGN4: each a multiple of 4
constexpr long long DESC_MAX_N = (1ll << 30) * ADAM_CHUNK;

// THE descriptor check, run by every entry point before its first launch: the list's chunk total (>= 0; at most 2^30, the grid's
// bound), or WSMG_EINVAL (the error codes are negative, so one return value carries both: callers test `< 0`).
// DESC_VMAX: vmax[i], the parallel host array of the _ext entry points, is a fifth pointer of descriptor i: not null and, whatever
// the entry point, a multiple of 4.
static long long check_descs(const WsmgAdamDesc* descs, int n, int need, long long max_n, float* const* vmax = nullptr) {
  if (n < 0 || (n > 0 && !descs)) return WSMG_EINVAL;
  if ((need & DESC_VMAX) && n > 0 && !vmax) return WSMG_EINVAL;
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    const WsmgAdamDesc& d = descs[i];
    if (d.n < 0 || d.n > max_n) return WSMG_EINVAL;
    if (d.n == 0) continue;
    if (!d.grad || ((need & DESC_ALL) && (!d.param || !d.exp_avg || !d.exp_avg_sq))) return WSMG_EINVAL;
    if ((need & DESC_VMAX) && (!vmax[i] || ((uintptr_t)vmax[i] & 3))) return WSMG_EINVAL;
    uintptr_t bits = (uintptr_t)d.grad;
    if (need & DESC_ALL) bits |= (uintptr_t)d.param | (uintptr_t)d.exp_avg | (uintptr_t)d.exp_avg_sq;
    if ((need & DESC_ALIGN4) && (bits & 3)) return WSMG_EINVAL;
    total += (d.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    if (total > (1ll << 30)) return WSMG_EINVAL;
  }
  return total;
}

// THE batching loop over checked descs: at most ADAM_MAX tensors per launch, descriptors with n == 0 own no chunk and no table
// entry.  The caller's batch b (its other fields already set) is filled in place: slot(k, desc) stores entry k's pointers,
// launch(blocks, base) launches `blocks` workgroups whose first chunk is chunk `base` of the list.  Returns the chunk total.
template <class Slot, class Launch>
static int for_each_batch(const WsmgAdamDesc* descs, int n, ChunkTable& tb, Slot slot, Launch launch) {
  int base = 0;
  for (int i = 0; i < n;) {
    tb.count = 0;
    int blocks = 0;
    for (; i < n && tb.count < ADAM_MAX; ++i) {
      if (descs[i].n == 0) continue;
      const int k = tb.count++;
      slot(k, descs[i]);
      tb.n[k] = descs[i].n;
      tb.first_block[k] = blocks;
      blocks += (int)((descs[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK);
    }
    if (!tb.count) continue;
    tb.first_block[tb.count] = blocks;
    launch(blocks, base);
    base += blocks;
  }
  return base;
}

// What an _ext entry point adds to adam_launch's arguments (null: the entry points without options and their four kernels).
struct AdamExtArgs {
  float* const* vmax;      // host array parallel to descs, read when flags has WSMG_ADAM_AMSGRAD
  int flags;
};
constexpr int ADAM_FLAGS = WSMG_ADAM_AMSGRAD | WSMG_ADAM_MAXIMIZE | WSMG_ADAM_DECOUPLED_WD;

template <bool AMSGRAD>
static void adam_ext_launch(const AdamExtBatch& x, bool hyper, bool guard, dim3 grid, wsmg_stream_t s) {
  if (hyper && guard) hipLaunchKernelGGL((adam_multi_ext_kernel<true, true, AMSGRAD>), grid, dim3(256), 0, wsmg_s(s), x);
  else if (hyper) hipLaunchKernelGGL((adam_multi_ext_kernel<false, true, AMSGRAD>), grid, dim3(256), 0, wsmg_s(s), x);
  else if (guard) hipLaunchKernelGGL((adam_multi_ext_kernel<true, false, AMSGRAD>), grid, dim3(256), 0, wsmg_s(s), x);
  else hipLaunchKernelGGL((adam_multi_ext_kernel<false, false, AMSGRAD>), grid, dim3(256), 0, wsmg_s(s), x);
}

static int adam_launch(const WsmgAdamDesc* descs, int n, int need, float lr, float beta1, float beta2, float eps, float weight_decay,
                       double bias_correction1, double bias_correction2, const float* step_dev, const float* guard,
                       const float* hyper, wsmg_stream_t s, const AdamExtArgs* ext = nullptr) {
  if (!step_dev && (!(bias_correction1 > 0.0) || !(bias_correction2 > 0.0))) return WSMG_EINVAL;
  if (ext && (ext->flags & ~ADAM_FLAGS)) return WSMG_EINVAL;
  const bool amsgrad = ext && (ext->flags & WSMG_ADAM_AMSGRAD);
  if (check_descs(descs, n, need | (amsgrad ? DESC_VMAX : 0), DESC_MAX_N, amsgrad ? ext->vmax : nullptr) < 0) return WSMG_EINVAL;
  AdamExtBatch x;
  AdamBatch& b = x.b;
  b.h = {1.f - beta1, beta2, 1.f - beta2, eps, weight_decay};
  b.lr_bc1 = step_dev ? 0.f : (float)((double)lr / bias_correction1);
  b.sqrt_bc2 = step_dev ? 1.f : (float)sqrt(bias_correction2);
  b.step_dev = step_dev;
  b.lr = lr;
  b.beta1 = beta1;
  b.guard = guard;
  b.hyper = hyper;
  for (int k = 0; k < ADAM_MAX; ++k) x.e.vmax[k] = nullptr;
  x.e.flags = ext ? ext->flags : 0;
  x.e.decay = (float)(1.0 - (double)lr * (double)weight_decay);   // (the _hyper kernels form theirs from the row, with this expression)
  for_each_batch(descs, n, b.tab,
                 [&](int k, const WsmgAdamDesc& d) {
                   b.p[k] = d.param; b.g[k] = d.grad; b.m[k] = d.exp_avg; b.v[k] = d.exp_avg_sq;
                   if (amsgrad) x.e.vmax[k] = ext->vmax[&d - descs];
                 },
                 [&](int blocks, int) {
                   const dim3 grid((unsigned)blocks);
                   if (ext) {
                     if (amsgrad) adam_ext_launch<true>(x, hyper != nullptr, guard != nullptr, grid, s);
                     else adam_ext_launch<false>(x, hyper != nullptr, guard != nullptr, grid, s);
                   }
                   else if (hyper && guard) hipLaunchKernelGGL(adam_multi_guarded_hyper_kernel, grid, dim3(256), 0, wsmg_s(s), b);
                   else if (hyper) hipLaunchKernelGGL(adam_multi_hyper_kernel, grid, dim3(256), 0, wsmg_s(s), b);
                   else if (guard) hipLaunchKernelGGL(adam_multi_guarded_kernel, grid, dim3(256), 0, wsmg_s(s), b);
                   else hipLaunchKernelGGL(adam_multi_kernel, grid, dim3(256), 0, wsmg_s(s), b);
                 });
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_adam_step_multi(const WsmgAdamDesc* descs, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    double bias_correction1, double bias_correction2, wsmg_stream_t s) {
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, nullptr, nullptr,
                     nullptr, s);
}

// The same step with the step COUNT read from device memory (one float32, already incremented for this step): what a captured
// HIP graph replays — its kernel arguments are frozen, so the bias corrections cannot be passed by value.
extern "C" int wsmg_adam_step_multi_dev(const WsmgAdamDesc* descs, int n, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, const float* step_dev, wsmg_stream_t s) {
  if (!step_dev) return WSMG_EINVAL;
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, 0.0, 0.0, step_dev, nullptr, nullptr, s);
}

// The _dev form behind a guard record (wsmg_grad_norm_multi on the same stream, before it): nothing is written when the record's
// `skip` is set, g * coef is read otherwise.  step_dev is the count that call advanced.
extern "C" int wsmg_adam_step_multi_guarded(const WsmgAdamDesc* descs, int n, float lr, float beta1, float beta2, float eps,
                                            float weight_decay, const float* step_dev, const float* guard, wsmg_stream_t s) {
  if (!step_dev || !guard) return WSMG_EINVAL;
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, 0.0, 0.0, step_dev, guard, nullptr, s);
}

// The _dev / _guarded step (guard null / not null) with lr, beta1, beta2, eps and weight_decay read from hyper_row, one 8-float row
// of the hyper record in device memory.  This form also refuses pointers that are not multiples of 4.
extern "C" int wsmg_adam_step_multi_hyper(const WsmgAdamDesc* descs, int n, const float* hyper_row, const float* step_dev,
                                          const float* guard, wsmg_stream_t s) {
  if (!hyper_row || !step_dev) return WSMG_EINVAL;
  if (((uintptr_t)hyper_row & 3) || ((uintptr_t)step_dev & 3) || ((uintptr_t)guard & 3)) return WSMG_EINVAL;
  return adam_launch(descs, n, DESC_ALL | DESC_ALIGN4, 0.f, 0.f, 0.f, 0.f, 0.f, 0.0, 0.0, step_dev, guard, hyper_row, s);
}

// The four front ends with the options of `flags` (WSMG_ADAM_AMSGRAD | WSMG_ADAM_MAXIMIZE | WSMG_ADAM_DECOUPLED_WD; any other bit:
// WSMG_EINVAL), each with the checks of the entry point it mirrors.  max_exp_avg_sq is a HOST array of n device pointers, parallel to
// descs; it is read only with WSMG_ADAM_AMSGRAD, and then a null or not 4-byte aligned entry of a non-empty descriptor is
// WSMG_EINVAL, found before the first launch.  flags = 0 steps as the entry point without `_ext` does, bit for bit, through the
// kernels of this family.
extern "C" int wsmg_adam_step_multi_ext(const WsmgAdamDesc* descs, int n, float* const* max_exp_avg_sq, int flags, float lr, float beta1,
                                        float beta2, float eps, float weight_decay, double bias_correction1, double bias_correction2,
                                        wsmg_stream_t s) {
  const AdamExtArgs ext = {max_exp_avg_sq, flags};
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, nullptr, nullptr,
                     nullptr, s, &ext);
}

extern "C" int wsmg_adam_step_multi_dev_ext(const WsmgAdamDesc* descs, int n, float* const* max_exp_avg_sq, int flags, float lr,
                                            float beta1, float beta2, float eps, float weight_decay, const float* step_dev,
                                            wsmg_stream_t s) {
  if (!step_dev) return WSMG_EINVAL;
  const AdamExtArgs ext = {max_exp_avg_sq, flags};
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, 0.0, 0.0, step_dev, nullptr, nullptr, s, &ext);
}

extern "C" int wsmg_adam_step_multi_guarded_ext(const WsmgAdamDesc* descs, int n, float* const* max_exp_avg_sq, int flags, float lr,
                                                float beta1, float beta2, float eps, float weight_decay, const float* step_dev,
                                                const float* guard, wsmg_stream_t s) {
  if (!step_dev || !guard) return WSMG_EINVAL;
  const AdamExtArgs ext = {max_exp_avg_sq, flags};
  return adam_launch(descs, n, DESC_ALL, lr, beta1, beta2, eps, weight_decay, 0.0, 0.0, step_dev, guard, nullptr, s, &ext);
}

extern "C" int wsmg_adam_step_multi_hyper_ext(const WsmgAdamDesc* descs, int n, float* const* max_exp_avg_sq, int flags,
                                              const float* hyper_row, const float* step_dev, const float* guard, wsmg_stream_t s) {
  if (!hyper_row || !step_dev) return WSMG_EINVAL;
  if (((uintptr_t)hyper_row & 3) || ((uintptr_t)step_dev & 3) || ((uintptr_t)guard & 3)) return WSMG_EINVAL;
  const AdamExtArgs ext = {max_exp_avg_sq, flags};
  return adam_launch(descs, n, DESC_ALL | DESC_ALIGN4, 0.f, 0.f, 0.f, 0.f, 0.f, 0.0, 0.0, step_dev, guard, hyper_row, s, &ext);
}

// The sum-of-squares launches over checked descs: chunk c of the list -> partials[c].  Returns the chunk total.
static int grad_sumsq_launches(const WsmgAdamDesc* descs, int n, double* partials, wsmg_stream_t s) {
  GradBatch b;
  return for_each_batch(descs, n, b.tab, [&](int k, const WsmgAdamDesc& d) { b.g[k] = d.grad; },
                        [&](int blocks, int base) {
                          b.partials = partials + base;
                          hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, wsmg_s(s), b);
                        });
}

// Global L2 norm of the descs' gradients (param / exp_avg / exp_avg_sq are not read) into the guard record.  The partials' capacity
// is checked against the chunk total.  hyper_guard_row (or null): max_norm is read from it on the device and the by-value max_norm
// is ignored.
// gate (or null): the _gated forms' device word; a non-zero gate[0] forces the skip (guard_finalize<true>).
static int grad_norm_launch(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap, float max_norm,
                            const float* hyper_guard_row, int skip_nonfinite, float* guard, float* step_dev, wsmg_stream_t s,
                            const float* gate = nullptr) {
  if (!guard || !partials || partials_cap < 0 || !(max_norm >= 0.f)) return WSMG_EINVAL;
  if (((uintptr_t)partials & 7) || ((uintptr_t)guard & 3) || ((uintptr_t)step_dev & 3) || ((uintptr_t)gate & 3)) return WSMG_EINVAL;
  const long long total = check_descs(descs, n, DESC_GRAD, DESC_MAX_N);
  if (total < 0) return WSMG_EINVAL;
  if (total > partials_cap) return WSMG_ENOMEM;
  const int base = grad_sumsq_launches(descs, n, partials, s);
  if (gate)
    hipLaunchKernelGGL(grad_guard_finalize_gated_kernel, dim3(1), dim3(256), 0, wsmg_s(s), (const double*)partials, base, max_norm,
                       hyper_guard_row, skip_nonfinite, gate, guard, step_dev);
  else if (hyper_guard_row)
    hipLaunchKernelGGL(grad_guard_finalize_hyper_kernel, dim3(1), dim3(256), 0, wsmg_s(s), (const double*)partials, base,
                       hyper_guard_row, skip_nonfinite, guard, step_dev);
  else
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(256), 0, wsmg_s(s), (const double*)partials, base, max_norm,
                       skip_nonfinite, guard, step_dev);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_grad_norm_multi(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap, float max_norm,
                                    int skip_nonfinite, float* guard, float* step_dev, wsmg_stream_t s) {
  return grad_norm_launch(descs, n, partials, partials_cap, max_norm, nullptr, skip_nonfinite, guard, step_dev, s);
}

// wsmg_grad_norm_multi with max_norm read from the hyper record's guard row in device memory (a value <= 0 there: no clipping).
extern "C" int wsmg_grad_norm_multi_hyper(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap,
                                          const float* hyper_guard_row, int skip_nonfinite, float* guard, float* step_dev,
                                          wsmg_stream_t s) {
  if (!hyper_guard_row || ((uintptr_t)hyper_guard_row & 3)) return WSMG_EINVAL;
  return grad_norm_launch(descs, n, partials, partials_cap, 0.f, hyper_guard_row, skip_nonfinite, guard, step_dev, s);
}

// The two entry points above behind an external gate: gate[0] != 0 (read on the device, in the finalize) forces the skip.  A NULL or
// not 4-byte aligned gate is WSMG_EINVAL, with the checks of the entry point each mirrors, before anything is launched.
extern "C" int wsmg_grad_norm_multi_gated(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap, float max_norm,
                                          int skip_nonfinite, const float* gate, float* guard, float* step_dev, wsmg_stream_t s) {
  if (!gate) return WSMG_EINVAL;
  return grad_norm_launch(descs, n, partials, partials_cap, max_norm, nullptr, skip_nonfinite, guard, step_dev, s, gate);
}

extern "C" int wsmg_grad_norm_multi_hyper_gated(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap,
                                                const float* hyper_guard_row, int skip_nonfinite, const float* gate, float* guard,
                                                float* step_dev, wsmg_stream_t s) {
  if (!gate || !hyper_guard_row || ((uintptr_t)hyper_guard_row & 3)) return WSMG_EINVAL;
  return grad_norm_launch(descs, n, partials, partials_cap, 0.f, hyper_guard_row, skip_nonfinite, guard, step_dev, s, gate);
}

// The report's argument checks (the chunk total against both capacities): 0, WSMG_EINVAL or WSMG_ENOMEM.
static int grad_report_check(const WsmgAdamDesc* descs, int n, const double* partials, long long partials_cap, const uint32_t* scan,
                             long long scan_cap, const uint32_t* report) {
  if (!partials || partials_cap < 0 || !scan || scan_cap < 0 || !report) return WSMG_EINVAL;
  if (((uintptr_t)partials & 7) || ((uintptr_t)scan & 3) || ((uintptr_t)report & 3)) return WSMG_EINVAL;
  const long long total = check_descs(descs, n, DESC_GRAD | DESC_ALIGN4, (1ll << 32) - 1);   // 32-bit counters
  if (total < 0) return WSMG_EINVAL;
  return (total > partials_cap || total > scan_cap) ? WSMG_ENOMEM : 0;
}

// The scan launches (grad_sumsq_launches' batches, so a chunk has one index in partials and scan), the fold launches over every
// descriptor (batched by tensor, the empty ones included: every tensor has a row), and the latch's launch if there is one.
// Arguments are checked.
static void grad_report_launches(const WsmgAdamDesc* descs, int n, const double* partials, uint32_t* scan, const float* guard,
                                 const float* step_dev, uint32_t* report, uint32_t* latch, wsmg_stream_t s) {
  ScanBatch sb;
  for_each_batch(descs, n, sb.tab, [&](int k, const WsmgAdamDesc& d) { sb.g[k] = d.grad; },
                 [&](int blocks, int base) {
                   sb.scan = scan + 4 * (long long)base;
                   hipLaunchKernelGGL(grad_scan_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, wsmg_s(s), sb);
                 });
  int first = 0;
  for (int i = 0; i < n;) {
    FoldBatch b;
    b.row0 = i;
    int k = 0;
    for (; i < n && k < ADAM_MAX; ++i, ++k) {
      b.first[k] = first;
      b.chunks[k] = (int)((descs[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK);
      first += b.chunks[k];
    }
    b.partials = partials; b.scan = scan; b.report = report;
    hipLaunchKernelGGL(grad_report_fold_kernel, dim3((unsigned)k), dim3(256), 0, wsmg_s(s), b);
  }
  if (latch)
    hipLaunchKernelGGL(grad_report_latch_kernel, dim3(1), dim3(256), 0, wsmg_s(s), (const uint32_t*)report, n, guard, step_dev, latch);
}

// Per-tensor report of the gradients whose sums of squares wsmg_grad_norm_multi[_hyper] left in partials (the same descs or, as
// wsmgmap.optim.Adam passes them, the same list with zero-length descriptors in between: those own no chunk), and the latch that
// keeps the report of a skipped step.  Only grad and n of a descriptor are read.
extern "C" int wsmg_grad_report_multi(const WsmgAdamDesc* descs, int n, const double* partials, long long partials_cap, uint32_t* scan,
                                      long long scan_cap, const float* guard, const float* step_dev, uint32_t* report, uint32_t* latch,
                                      wsmg_stream_t s) {
  if ((latch && !guard) || (!guard != !step_dev)) return WSMG_EINVAL;
  if (((uintptr_t)guard & 3) || ((uintptr_t)step_dev & 3) || ((uintptr_t)latch & 3)) return WSMG_EINVAL;
  const int rc = grad_report_check(descs, n, partials, partials_cap, scan, scan_cap, report);
  if (rc) return rc;
  grad_report_launches(descs, n, partials, scan, guard, step_dev, report, latch, s);
  WSMG_RETURN_LAUNCH();
}

// The stand-alone form: the sum-of-squares launches into partials, then the report; no guard, no latch, no step count.
extern "C" int wsmg_grad_stats_multi(const WsmgAdamDesc* descs, int n, double* partials, long long partials_cap, uint32_t* scan,
                                     long long scan_cap, uint32_t* report, wsmg_stream_t s) {
  const int rc = grad_report_check(descs, n, partials, partials_cap, scan, scan_cap, report);
  if (rc) return rc;
  grad_sumsq_launches(descs, n, partials, s);
  grad_report_launches(descs, n, partials, scan, nullptr, nullptr, report, nullptr, s);
  WSMG_RETURN_LAUNCH();
}
