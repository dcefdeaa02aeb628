// The update path's two dense losses, each one launch per direction: path_kl, the contrastive-monitor auxiliary loss (below), and
// ce_nhwc, the per-pixel cross-entropy of the semantic-map head over NHWC logits (second half of the file).
//
// path_kl (policy.py:72-82 of the reference):
//
//   t  = (hi - dis) / (hi - lo)                 dis = gt_path [B][H][W]; lo, hi = its batch-global min / max (device scalars)
//   a  = area-resize(t, S x S)                  = adaptive average pooling: bin i = [floor(i H / S), ceil((i + 1) H / S))
//   tg = softmax(a / tau) over the S*S bins
//   kl[b] = mean_j tg_j (log tg_j - log att_j)   = F.kl_div(log att, tg, reduction='none').mean(-1); xlogy: 0 where tg_j == 0
//
// As torch ops this is 13 launches of 4-16 us forward and 8 backward, every one waiting for the one before (the region between
// the second GRU's forward and its backward is ≈70 such launches).  One workgroup per row: the row's H*W distances are read once
// (40 KB), bins are thread-private, the softmax statistics go through LDS.  Only att receives a gradient:
//   d att_j = - g[b] tg_j / att_j / (S*S).
#include "wsmg_common.h"

namespace {

__global__ __launch_bounds__(256) void path_kl_fwd_kernel(const float* __restrict__ dis, const float* __restrict__ lo_p,
                                                          const float* __restrict__ hi_p, const float* __restrict__ att, int H, int W,
                                                          int S, float inv_tau, float* __restrict__ target, float* __restrict__ kl) {
  __shared__ float red[4];
  __shared__ float bc;
  const int b = blockIdx.x, tid = threadIdx.x, n = S * S;
  const float lo = *lo_p, hi = *hi_p, rng = hi - lo;
  const float* __restrict__ d = dis + (size_t)b * H * W;
  float* __restrict__ tg = target + (size_t)b * n;
  // pass 1: pooled values -> target (temporarily a / tau), row maximum
  float mx = -INFINITY;
  for (int j = tid; j < n; j += 256) {
    const int by = j / S, bx = j - by * S;
    const int y0 = (by * H) / S, y1 = ((by + 1) * H + S - 1) / S;
    const int x0 = (bx * W) / S, x1 = ((bx + 1) * W + S - 1) / S;
    float s = 0.f;
    for (int y = y0; y < y1; ++y)
      for (int x = x0; x < x1; ++x) s += (hi - d[y * W + x]) / rng;
    const float z = s / (float)((y1 - y0) * (x1 - x0)) * inv_tau;
    tg[j] = z;
    mx = fmaxf(mx, z);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) bc = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  mx = bc;
  float sum = 0.f;
  for (int j = tid; j < n; j += 256) {
    const float e = expf(tg[j] - mx);
    tg[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) bc = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  const float inv = 1.f / bc;
  const float* __restrict__ a = att + (size_t)b * n;
  float acc = 0.f;
  for (int j = tid; j < n; j += 256) {
    const float t = tg[j] * inv;
    tg[j] = t;
    acc += (t > 0.f ? t * logf(t) : 0.f) - t * logf(a[j]);
  }
  acc = wave_sum(acc);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) kl[b] = (red[0] + red[1] + red[2] + red[3]) / (float)n;
}

__global__ __launch_bounds__(256) void path_kl_bwd_kernel(const float* __restrict__ gkl, const float* __restrict__ target,
                                                          const float* __restrict__ att, int64_t total, int n, float* __restrict__ datt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  datt[i] = -gkl[i / n] * target[i] / att[i] / (float)n;
}

// ---- fused per-pixel cross-entropy over NHWC logits (policy.py:61-66: F.cross_entropy(pred_sem_map, target,
// reduction='none')): the 27 classes of a pixel are one 64/128-byte run of the 32-channel-padded conv output, so the
// loss needs no NHWC->NCHW transpose and no materialised log-softmax.  One thread per pixel row.
// A label outside [0, classes) — F.cross_entropy of the reference faults on it — makes that row's loss and its whole 32-wide
// gradient row NaN, as the fused classifier tail does (wsmg_cls_tail.hip): loud, not a finite wrong number.  The int64 label
// itself is compared (2^40 truncates to 0); -100 is not an ignore_index.
template <class T>
__device__ __forceinline__ void ce_row_load(const T* __restrict__ row, float (&v)[32]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f32x4 q = ld4(row + 4 * j);
    v[4 * j] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
  }
}
// v: the row's logits in, exp(v[c] - mx) out (0 for the padded classes c >= classes); mx the maximum over the classes, sum the sum
// of the exponentials in c order
__device__ __forceinline__ void ce_row_softmax(float (&v)[32], int classes, float& mx, float& sum) {
  mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 32; ++c) if (c < classes) mx = fmaxf(mx, v[c]);
  sum = 0.f;
#pragma unroll
  for (int c = 0; c < 32; ++c) { v[c] = c < classes ? expf(v[c] - mx) : 0.f; sum += v[c]; }
}

template <class T>
__global__ __launch_bounds__(256) void ce_nhwc_fwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                          int64_t rows, int classes, float* __restrict__ loss) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float v[32], mx, sum;
  ce_row_load(logits + r * 32, v);
  const int64_t lab = target[r];
  const bool in_range = (uint64_t)lab < (uint64_t)classes;
  const int t = in_range ? (int)lab : -1;
  float vt = 0.f;
#pragma unroll
  for (int c = 0; c < 32; ++c) if (c == t) vt = v[c];
  ce_row_softmax(v, classes, mx, sum);
  loss[r] = in_range ? (mx + logf(sum)) - vt : __builtin_nanf("");
}

// dlogits[r][c] = (softmax(logits[r])[c] - [c == target[r]]) * gloss[r]; padded channels get 0; a row whose label is outside
// [0, classes) gets NaN in all 32 channels
template <class T>
__global__ __launch_bounds__(256) void ce_nhwc_bwd_kernel(const T* __restrict__ logits, const int64_t* __restrict__ target,
                                                          const float* __restrict__ gloss, int64_t rows, int classes,
                                                          T* __restrict__ dlogits) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float v[32], mx, sum;
  ce_row_load(logits + r * 32, v);
  ce_row_softmax(v, classes, mx, sum);
  const float g = gloss[r], inv = 1.f / sum;
  const int64_t lab = target[r];
  const bool in_range = (uint64_t)lab < (uint64_t)classes;
  const int t = in_range ? (int)lab : -1;
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * j + e;
      const float d = c < classes ? (v[c] * inv - (c == t ? 1.f : 0.f)) * g : 0.f;
      q[e] = in_range ? d : nan;
    }
    st4(dlogits + r * 32 + 4 * j, q);
  }
}

template <class T>
int ce_nhwc_fwd_t(const T* logits, const int64_t* target, int64_t rows, int classes, float* loss, wsmg_stream_t s) {
  if (rows <= 0 || classes <= 0 || classes > 32) return WSMG_EINVAL;
  hipLaunchKernelGGL(ce_nhwc_fwd_kernel<T>, dim3((unsigned)wsmg_cdiv(rows, 256)), dim3(256), 0, wsmg_s(s), logits, target, rows, classes, loss);
  WSMG_RETURN_LAUNCH();
}
template <class T>
int ce_nhwc_bwd_t(const T* logits, const int64_t* target, const float* gloss, int64_t rows, int classes, T* dlogits, wsmg_stream_t s) {
  if (rows <= 0 || classes <= 0 || classes > 32) return WSMG_EINVAL;
  hipLaunchKernelGGL(ce_nhwc_bwd_kernel<T>, dim3((unsigned)wsmg_cdiv(rows, 256)), dim3(256), 0, wsmg_s(s), logits, target, gloss, rows, classes, dlogits);
  WSMG_RETURN_LAUNCH();
}

}  // namespace

extern "C" int wsmg_path_kl_fwd(const float* dis, const float* lo, const float* hi, const float* att, int B, int H, int W, int S, float tau,
                                float* target, float* kl, wsmg_stream_t s) {
  if (B <= 0 || H <= 0 || W <= 0 || S <= 0 || S > H || S > W || !(tau > 0.f)) return WSMG_EINVAL;
  hipLaunchKernelGGL(path_kl_fwd_kernel, dim3((unsigned)B), dim3(256), 0, wsmg_s(s), dis, lo, hi, att, H, W, S, 1.f / tau, target, kl);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_path_kl_bwd(const float* gkl, const float* target, const float* att, int B, int n, float* datt, wsmg_stream_t s) {
  if (B <= 0 || n <= 0) return WSMG_EINVAL;
  const int64_t total = (int64_t)B * n;
  hipLaunchKernelGGL(path_kl_bwd_kernel, dim3((unsigned)wsmg_cdiv(total, 256)), dim3(256), 0, wsmg_s(s), gkl, target, att, total, n, datt);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_ce_nhwc_fwd(const float* logits, const int64_t* target, int64_t rows, int classes, float* loss, wsmg_stream_t s) { return ce_nhwc_fwd_t<float>(logits, target, rows, classes, loss, s); }
extern "C" int wsmg_ce_nhwc_fwd_bf16(const void* logits, const int64_t* target, int64_t rows, int classes, float* loss, wsmg_stream_t s) { return ce_nhwc_fwd_t<bf16_t>((const bf16_t*)logits, target, rows, classes, loss, s); }
extern "C" int wsmg_ce_nhwc_bwd(const float* logits, const int64_t* target, const float* gloss, int64_t rows, int classes, float* dlogits, wsmg_stream_t s) { return ce_nhwc_bwd_t<float>(logits, target, gloss, rows, classes, dlogits, s); }
extern "C" int wsmg_ce_nhwc_bwd_bf16(const void* logits, const int64_t* target, const float* gloss, int64_t rows, int classes, void* dlogits, wsmg_stream_t s) { return ce_nhwc_bwd_t<bf16_t>((const bf16_t*)logits, target, gloss, rows, classes, (bf16_t*)dlogits, s); }
