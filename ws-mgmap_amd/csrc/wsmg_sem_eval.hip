// Scoring the semantic-map head on the device: the confusion matrix of the predicted map against the nearest-resized ground truth,
// and pixel accuracy / per-class IoU / mIoU from it.  Not a reference operator (the reference reports the prediction monitor's
// cross-entropy only, policy.py:61-66); it reads what every forward pass leaves behind — the NHWC logits [B][H][W][32] of
// map_classfier (mg_map_policy.py:78-86), float32 or bf16, channels >= classes padding — and observations['gt_semantic_map'].
//
//   prediction  argmax over channels 0 .. classes-1 (padding never looked at), ties to the lowest index, +Inf an ordinary maximum;
//               a NaN among those channels: no prediction (pred = 255)
//   label       gt[b][min(floorf(y * (float)Hg / (float)H), Hg - 1)][likewise x], truncated, exactly as wsmg_cls_tail.hip forms it;
//               valid iff g > -1.0f && g < (float)classes, decided on the float (NaN and +-Inf invalid, -0.5 a valid 0)
//   counting    invalid label: ignored[0] += 1 and nothing else;  else no prediction: ignored[1] += 1;  else confusion[label][pred] += 1
//
// Bandwidth-bound: 64 (bf16) or 128 (float32) bytes per pixel against ~100 integer / compare instructions.  A thread owns whole
// pixels — one channel row, 16-byte loads — two per loop trip, 512 threads, at most two workgroups per CU: 128 KB of bf16 loads in
// flight per CU (measured at B = 512: 256 x 256 threads 48 us per call, 512 x 256 36, 1 024 x 256 41, 256 x 512 33, 512 x 512 30); the
// label gather is issued in front of the compare chain.  The matrix is a classes x classes uint32 histogram in LDS (<= 4 KB, LDS
// integer atomics), flushed once per workgroup with 64-bit global integer atomics, zero cells skipped: integer sums, exact and
// repeatable in any order.  The entry point refuses B*H*W >= 2^31, so no LDS counter can wrap.
#include "wsmg_common.h"

namespace {

constexpr int CH = 32;          // channels of the logits = padded classes
constexpr int THREADS = 512;
constexpr int PIX = 2;          // pixels in flight per thread
constexpr int MAX_WG = 512;     // two workgroups per CU
constexpr unsigned char NO_PRED = 255;

struct SemArgs {
  const void* logits;            // [B][H][W][32]
  const float* gt;               // [B][Hg][Wg], or null: predictions only
  const unsigned char* row_mask; // [B], or null: every row
  unsigned long long* confusion; // [classes][classes] (int64 of the caller: two's-complement adds)
  unsigned long long* ignored;   // [2]
  unsigned char* pred;           // [B][H][W], or null
  int classes, H, W, Hg, Wg;
  int total;                     // B * H * W < 2^31
  float sy, sx;                  // Hg / H, Wg / W in float32: torch's nearest-neighbour source index is floorf(dst * scale)
};

template <typename T> struct Row;
template <> struct Row<float> {
  u32x4 v[8];
  __device__ __forceinline__ void load(const void* base, int p) {
    const u32x4* q = reinterpret_cast<const u32x4*>(base) + (size_t)p * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = q[j];
  }
  __device__ __forceinline__ float at(int c) const { return __uint_as_float(v[c >> 2][c & 3]); }
};
template <> struct Row<bf16_t> {
  u32x4 v[4];
  __device__ __forceinline__ void load(const void* base, int p) {
    const u32x4* q = reinterpret_cast<const u32x4*>(base) + (size_t)p * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q[j];
  }
  __device__ __forceinline__ float at(int c) const {          // the stored bf16, widened
    const unsigned w = v[c >> 3][(c >> 1) & 3];
    return __uint_as_float((c & 1) ? (w & 0xffff0000u) : (w << 16));
  }
};

template <typename T>
__global__ __launch_bounds__(THREADS) void sem_confusion_kernel(SemArgs a) {
  __shared__ unsigned hist[CH * CH];
  __shared__ unsigned ign[2];
  const int tid = threadIdx.x;
  const int cells = a.classes * a.classes;
  for (int i = tid; i < cells; i += THREADS) hist[i] = 0u;
  if (tid < 2) ign[tid] = 0u;
  __syncthreads();
  const int HW = a.H * a.W;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  for (int64_t p0 = (int64_t)blockIdx.x * THREADS + tid; p0 < a.total; p0 += stride * PIX) {
    bool live[PIX];
    float g[PIX];
    Row<T> row[PIX];
    // every load of the trip first: the label gather (a 4-byte read through two divisions), then the channel rows
#pragma unroll
    for (int u = 0; u < PIX; ++u) {
      const int64_t p = p0 + u * stride;
      live[u] = false;
      g[u] = 0.f;
      if (p < a.total) {
        const int pi = (int)p;
        const int b = pi / HW, rem = pi - b * HW;
        live[u] = !a.row_mask || a.row_mask[b] != 0;
        if (live[u]) {
          if (a.gt) {
            const int y = rem / a.W, x = rem - y * a.W;
            int syi = (int)floorf((float)y * a.sy), sxi = (int)floorf((float)x * a.sx);
            syi = syi < a.Hg - 1 ? syi : a.Hg - 1;
            sxi = sxi < a.Wg - 1 ? sxi : a.Wg - 1;
            g[u] = a.gt[((int64_t)b * a.Hg + syi) * a.Wg + sxi];
          }
          row[u].load(a.logits, pi);
        } else if (a.pred) {
          a.pred[pi] = NO_PRED;          // a masked-out row contributes nothing anywhere
        }
      }
    }
#pragma unroll
    for (int u = 0; u < PIX; ++u) {
      if (!live[u]) continue;
      float best = row[u].at(0);
      int arg = 0;
      bool nan = best != best;
#pragma unroll
      for (int c = 1; c < CH; ++c) {
        if (c < a.classes) {             // wave-uniform: the padding channels are never looked at
          const float v = row[u].at(c);
          nan = nan || v != v;
          if (v > best) { best = v; arg = c; }      // strict: ties, -0.0 against +0.0 among them, stay with the lowest index
        }
      }
      if (a.pred) a.pred[(int)(p0 + u * stride)] = nan ? NO_PRED : (unsigned char)arg;
      if (!a.gt) continue;
      // validity on the float, before any conversion: NaN and +-Inf fail both compares, -0.5 truncates to a valid 0 as .long() does
      if (!(g[u] > -1.0f && g[u] < (float)a.classes)) atomicAdd(&ign[0], 1u);
      else if (nan) atomicAdd(&ign[1], 1u);
      else atomicAdd(&hist[(int)g[u] * a.classes + arg], 1u);
    }
  }
  if (!a.gt) return;
  __syncthreads();
  for (int i = tid; i < cells; i += THREADS) {
    const unsigned n = hist[i];
    if (n) atomicAdd(&a.confusion[i], (unsigned long long)n);
  }
  if (tid < 2 && ign[tid]) atomicAdd(&a.ignored[tid], (unsigned long long)ign[tid]);
}

// scores[0] pixels counted, [1] pixel accuracy, [2] mIoU, then per class c: [3 + 3c] IoU, [4 + 3c] ground-truth pixels,
// [5 + 3c] predicted pixels.  Row and column sums in int64 (exact), one division per figure in float64; the two means run in class order.
__global__ __launch_bounds__(64) void sem_scores_kernel(const long long* __restrict__ m, int classes, double* __restrict__ scores) {
  __shared__ long long tp_s[CH], gt_s[CH];
  __shared__ double iou_s[CH];
  const int c = threadIdx.x;
  if (c < classes) {
    long long gtn = 0, prn = 0;
    for (int j = 0; j < classes; ++j) {
      gtn += m[c * classes + j];
      prn += m[j * classes + c];
    }
    const long long tp = m[c * classes + c], uni = gtn + prn - tp;
    const double iou = uni != 0 ? (double)tp / (double)uni : __builtin_nan("");
    tp_s[c] = tp; gt_s[c] = gtn; iou_s[c] = iou;
    scores[3 + 3 * c] = iou;
    scores[4 + 3 * c] = (double)gtn;
    scores[5 + 3 * c] = (double)prn;
  }
  __syncthreads();
  if (c != 0) return;
  long long total = 0, right = 0;
  double s = 0.0;
  int present = 0;
  for (int j = 0; j < classes; ++j) {
    total += gt_s[j];
    right += tp_s[j];
    if (iou_s[j] == iou_s[j]) { s += iou_s[j]; ++present; }
  }
  scores[0] = (double)total;
  scores[1] = total != 0 ? (double)right / (double)total : __builtin_nan("");
  scores[2] = present ? s / (double)present : __builtin_nan("");
}

template <typename T>
int sem_confusion(const void* logits, int classes, const float* gt, int Hg, int Wg, int B, int H, int W, const uint8_t* row_mask,
                  int64_t* confusion, int64_t* ignored, uint8_t* pred, wsmg_stream_t stream) {
  if (!logits || classes < 1 || classes > CH || B <= 0 || H <= 0 || W <= 0) return WSMG_EINVAL;
  if ((int64_t)B * H * W >= (1ll << 31)) return WSMG_EINVAL;
  const bool pred_only = !gt && !confusion && !ignored;          // the three together, and then a place for the predictions
  if (pred_only ? !pred : (!gt || !confusion || !ignored || Hg <= 0 || Wg <= 0)) return WSMG_EINVAL;
  SemArgs a{};
  a.logits = logits; a.gt = gt; a.row_mask = row_mask; a.pred = pred;
  a.confusion = reinterpret_cast<unsigned long long*>(confusion); a.ignored = reinterpret_cast<unsigned long long*>(ignored);
  a.classes = classes; a.H = H; a.W = W; a.Hg = Hg; a.Wg = Wg; a.total = B * H * W;
  a.sy = gt ? (float)Hg / (float)H : 0.f; a.sx = gt ? (float)Wg / (float)W : 0.f;
  const int64_t wg = wsmg_cdiv(a.total, THREADS * PIX);
  hipLaunchKernelGGL(sem_confusion_kernel<T>, dim3((unsigned)(wg < MAX_WG ? wg : MAX_WG)), dim3(THREADS), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}

}  // namespace

extern "C" int wsmg_sem_confusion_f32(const float* logits, int classes, const float* gt, int Hg, int Wg, int B, int H, int W,
                                      const uint8_t* row_mask, int64_t* confusion, int64_t* ignored, uint8_t* pred,
                                      wsmg_stream_t stream) {
  return sem_confusion<float>(logits, classes, gt, Hg, Wg, B, H, W, row_mask, confusion, ignored, pred, stream);
}

extern "C" int wsmg_sem_confusion_bf16(const void* logits, int classes, const float* gt, int Hg, int Wg, int B, int H, int W,
                                       const uint8_t* row_mask, int64_t* confusion, int64_t* ignored, uint8_t* pred,
                                       wsmg_stream_t stream) {
  return sem_confusion<bf16_t>(logits, classes, gt, Hg, Wg, B, H, W, row_mask, confusion, ignored, pred, stream);
}

extern "C" int wsmg_sem_scores(const int64_t* confusion, int classes, double* scores, wsmg_stream_t stream) {
  if (!confusion || !scores || classes < 1 || classes > CH) return WSMG_EINVAL;
  hipLaunchKernelGGL(sem_scores_kernel, dim3(1), dim3(64), 0, wsmg_s(stream), reinterpret_cast<const long long*>(confusion), classes, scores);
  WSMG_RETURN_LAUNCH();
}
