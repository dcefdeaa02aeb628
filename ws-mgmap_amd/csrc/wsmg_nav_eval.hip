// Scoring the policy's other three supervised heads on the device: the waypoint attention against the ground-truth path, the
// action mean against the waypoint, the progress head against the progress (and as the rollout's stop rule).  Not a reference
// operator (the reference reports the three loss scalars only, policy.py:72-88, dagger_trainer.py:526-534); it reads what every
// forward pass leaves behind — net.att_map_t_m [B][S*S], pred [B][A], policy.prog [B] — and the observations that supervise them.
//
//   nav_rows_kernel        one workgroup per row -> rows float64 [B][WSMG_NAV_ROW] (layout: include/wsmgmap.h)
//     attention  target = argmin over the S x S cells of the area-resized dis [H][W] (the cell's window summed in float32 in
//                row-major order, divided by its count; a NaN cell — +Inf and -Inf in one window — ranks as +Inf), peak = argmax of
//                att, both ties to the lowest index: the reference's target softmax((hi - dis) / (hi - lo) / tau) is monotone
//                decreasing in the resized dis, so no batch-global extremes and no softmax are needed
//     action     e_j = tanh((double)pred_j) - (double)waypoint_j
//     progress   d = (double)prog - (double)progress; the stop code compares the float32 values with the threshold
//   nav_accumulate_kernel  one workgroup, one lane per output: the rows, staged through LDS 256 at a time, folded IN ROW ORDER into
//                          13 int64 counts and 12 float64 sums (no atomics: two runs on the same rows give the same bits)
//
// Bandwidth-trivial (dis is 40 KB per row at 100 x 100, ~22 MB at B = 512).  dis goes through LDS in bands of whole map rows,
// 16-byte coalesced loads behind a scalar head up to the first aligned address and in front of a scalar tail; a thread owns whole
// cells and walks its window in the band, its running sum parked in LDS between bands (so the order of a cell's sum is row-major
// whatever the band height).  A map row longer than the band (W > 10 240) is not staged: the cells read global memory directly
// behind one NaN scan.  Argmin / argmax: per-thread best over ascending cells, a wave-shuffle butterfly on (value, index), the four
// waves' winners through LDS.  The entropy's float64 partials take the same route in a fixed order.
#include "wsmg_common.h"

namespace {

constexpr int R = WSMG_NAV_ROW;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int CELLS_MAX = 4096;     // S * S
constexpr int BAND = 10240;         // floats of dis staged at a time: a 100 x 100 map in one band

struct NavArgs {
  const float* att;              // [B][S*S], or null with dis: the attention group is absent
  const float* dis;              // [B][H][W]
  const float* pred;             // [B][A], or null with waypoint: the action group is absent
  const float* waypoint;         // rows ld_waypoint floats apart
  const float* prog;             // [B], or null with progress: the progress group is absent
  const float* progress;         // [B]
  const unsigned char* row_mask; // [B], or null: every row
  double* rows;                  // [B][R]
  int S, H, W, A, ld_waypoint;
  float thr;
};

__device__ __forceinline__ double nan_d() { return __builtin_nan(""); }

// state + NaN in every other field of the group
__device__ __forceinline__ void write_group(double* out, int first, int last, double state) {
  out[first] = state;
  for (int f = first + 1; f <= last; ++f) out[f] = nan_d();
}

// n floats from global memory, NaN-checked, into dst (LDS) when given: scalar head up to the first 16-byte boundary, 16-byte body,
// scalar tail.  -> whether a NaN was seen by this thread
__device__ __forceinline__ bool scan_or_stage(const float* __restrict__ g, float* dst, int64_t n, int tid) {
  bool nan = false;
  int64_t head = (4 - (int64_t)((reinterpret_cast<uintptr_t>(g) >> 2) & 3)) & 3;
  head = head < n ? head : n;
  const int64_t nv = (n - head) >> 2, tail0 = head + nv * 4;
  if (tid < head) {
    const float v = g[tid];
    nan |= v != v;
    if (dst) dst[tid] = v;
  }
  const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
  for (int64_t i = tid; i < nv; i += THREADS) {
    const f32x4 v = gv[i];
    nan |= v[0] != v[0] || v[1] != v[1] || v[2] != v[2] || v[3] != v[3];
    if (dst) {
      float* d = dst + head + i * 4;          // (head shifts the LDS copy off 16-byte alignment: four 4-byte writes)
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  }
  if (tail0 + tid < n) {                      // at most 3 elements
    const float v = g[tail0 + tid];
    nan |= v != v;
    if (dst) dst[tail0 + tid] = v;
  }
  return nan;
}

// window of cell i along an axis of length L: [floor(i * L / S), ceil((i + 1) * L / S)) — F.interpolate(mode="area")
__device__ __forceinline__ void window(int i, int L, int S, int& lo, int& hi) {
  lo = (int)(((int64_t)i * L) / S);
  hi = (int)((((int64_t)i + 1) * L + S - 1) / S);
}

// every cell of this thread takes the map rows [y0, y1) of its window from src (src[0] = dis[y0][0]) onto its running sum
template <typename P>
__device__ __forceinline__ void pool_rows(P src, float* cell, int y0, int y1, int S, int H, int W, int tid) {
  for (int c = tid; c < S * S; c += THREADS) {
    int wy0, wy1, wx0, wx1;
    window(c / S, H, S, wy0, wy1);
    window(c % S, W, S, wx0, wx1);
    const int ys = wy0 > y0 ? wy0 : y0, ye = wy1 < y1 ? wy1 : y1;
    if (ys >= ye) continue;
    float acc = cell[c];
    for (int y = ys; y < ye; ++y) {
      const int64_t base = (int64_t)(y - y0) * W;
      for (int x = wx0; x < wx1; ++x) acc += src[base + x];
    }
    cell[c] = acc;
  }
}

// lowest index among the smallest values (LESS) or the largest (!LESS) over the workgroup; v / i: this thread's best
template <bool LESS>
__device__ __forceinline__ int block_arg(float v, int i, float* val_s, int* idx_s, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if ((LESS ? ov < v : ov > v) || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();                            // the scratch may still be read from the call before
  if ((tid & 63) == 0) { val_s[tid >> 6] = v; idx_s[tid >> 6] = i; }
  __syncthreads();
  v = val_s[0]; i = idx_s[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) {
    const float ov = val_s[w];
    const int oi = idx_s[w];
    if ((LESS ? ov < v : ov > v) || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  return i;
}

__global__ __launch_bounds__(THREADS) void nav_rows_kernel(NavArgs a) {
  __shared__ float band[BAND];
  __shared__ float cell[CELLS_MAX];
  __shared__ float val_s[WAVES];
  __shared__ int idx_s[WAVES];
  __shared__ double ent_s[WAVES];
  const int tid = threadIdx.x, b = blockIdx.x;
  double* out = a.rows + (size_t)b * R;
  const bool on = !a.row_mask || a.row_mask[b] != 0;          // workgroup-uniform, like every branch around a barrier below

  // ---- action: lane 0 of wave 1
  if (tid == 64) {
    if (!a.pred || !on) {
      write_group(out, WSMG_NAV_ACT_STATE, WSMG_NAV_ACT_ABS + 3, WSMG_NAV_ABSENT);
    } else {
      double sq = 0.0, ab[4] = {0.0, 0.0, 0.0, 0.0};
      bool bad = false;
      for (int j = 0; j < a.A; ++j) {
        const float p = a.pred[(size_t)b * a.A + j], w = a.waypoint[(size_t)b * a.ld_waypoint + j];
        // tanh saturates an infinite pred to a finite e: the inputs are held finite, which covers every non-finite e
        bad = bad || !isfinite(p) || !isfinite(w);
        const double e = tanh((double)p) - (double)w;
        ab[j] = fabs(e);
        sq += e * e;
      }
      if (bad) {
        write_group(out, WSMG_NAV_ACT_STATE, WSMG_NAV_ACT_ABS + 3, WSMG_NAV_INVALID);
      } else {
        out[WSMG_NAV_ACT_STATE] = WSMG_NAV_COUNTED;
        out[WSMG_NAV_ACT_SQ] = sq;
        out[WSMG_NAV_ACT_L2] = sqrt(sq);
        for (int j = 0; j < 4; ++j) out[WSMG_NAV_ACT_ABS + j] = ab[j];          // axes >= A: 0
      }
    }
  }
  // ---- progress: lane 0 of wave 2
  if (tid == 128) {
    if (!a.prog || !on) {
      write_group(out, WSMG_NAV_PROG_STATE, WSMG_NAV_PROG_STOP, WSMG_NAV_ABSENT);
    } else {
      const float p = a.prog[b], q = a.progress[b];
      if (!isfinite(p) || !isfinite(q)) {
        write_group(out, WSMG_NAV_PROG_STATE, WSMG_NAV_PROG_STOP, WSMG_NAV_INVALID);
      } else {
        const double d = (double)p - (double)q;
        out[WSMG_NAV_PROG_STATE] = WSMG_NAV_COUNTED;
        out[WSMG_NAV_PROG_ABS] = fabs(d);
        out[WSMG_NAV_PROG_SQ] = d * d;
        out[WSMG_NAV_PROG_STOP] = (double)(2 * (q >= a.thr) + (p >= a.thr));
      }
    }
  }
  // ---- attention: the whole workgroup
  if (!a.att || !on) {
    if (tid == 0) write_group(out, WSMG_NAV_ATT_STATE, WSMG_NAV_ATT_ENTROPY, WSMG_NAV_ABSENT);
    return;
  }
  const int S = a.S, H = a.H, W = a.W, n = S * S;
  const float* dis = a.dis + (size_t)b * H * W;
  const float* att = a.att + (size_t)b * n;
  for (int c = tid; c < n; c += THREADS) cell[c] = 0.f;
  bool bad = false;
  if (W > BAND) {                             // a map row does not fit the band: scan for NaN, then pool straight from global memory
    bad = scan_or_stage(dis, nullptr, (int64_t)H * W, tid);
    __syncthreads();                          // (cell[] zeroed by its owner: no hazard; keeps the two routes' barriers alike)
    pool_rows(dis, cell, 0, H, S, H, W, tid);
  } else {
    const int per = BAND / W;                 // whole map rows per band
    for (int y0 = 0; y0 < H; y0 += per) {
      const int y1 = y0 + per < H ? y0 + per : H;
      bad |= scan_or_stage(dis + (size_t)y0 * W, band, (int64_t)(y1 - y0) * W, tid);
      __syncthreads();
      pool_rows(band, cell, y0, y1, S, H, W, tid);
      __syncthreads();
    }
  }
  // target cell: the mean's argmin (a cell is its owner's alone up to here)
  float tv = __builtin_inff();
  int ti = 0x7fffffff;
  for (int c = tid; c < n; c += THREADS) {
    int wy0, wy1, wx0, wx1;
    window(c / S, H, S, wy0, wy1);
    window(c % S, W, S, wx0, wx1);
    float m = cell[c] / (float)((int64_t)(wy1 - wy0) * (wx1 - wx0));
    if (m != m) m = __builtin_inff();
    if (m < tv || ti == 0x7fffffff) { tv = m; ti = c; }          // ascending c: strict, so ties stay with the lowest index
  }
  const int target = block_arg<true>(tv, ti, val_s, idx_s, tid);
  // attention peak, validity and entropy in one pass
  float pv = -__builtin_inff();
  int pi = 0x7fffffff;
  double ent = 0.0;
  for (int c = tid; c < n; c += THREADS) {
    const float v = att[c];
    bad = bad || !(v >= 0.f);                 // NaN or negative (-0.0 passes)
    if (v > pv || pi == 0x7fffffff) { pv = v; pi = c; }
    if (v > 0.f) ent -= (double)v * log((double)v);
  }
  const int peak = block_arg<false>(pv, pi, val_s, idx_s, tid);
  ent = wave_sum_d(ent);
  if ((tid & 63) == 0) ent_s[tid >> 6] = ent;
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid != 0) return;
  if (any_bad) {
    write_group(out, WSMG_NAV_ATT_STATE, WSMG_NAV_ATT_ENTROPY, WSMG_NAV_INVALID);
    return;
  }
  double e = ent_s[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) e += ent_s[w];
  const int ty = target / S, tx = target % S, dy = abs(peak / S - ty), dx = abs(peak % S - tx);
  double mass = 0.0;
  for (int y = ty > 0 ? ty - 1 : 0; y <= (ty + 1 < S ? ty + 1 : S - 1); ++y)
    for (int x = tx > 0 ? tx - 1 : 0; x <= (tx + 1 < S ? tx + 1 : S - 1); ++x) mass += (double)att[y * S + x];
  out[WSMG_NAV_ATT_STATE] = WSMG_NAV_COUNTED;
  out[WSMG_NAV_ATT_TARGET] = (double)target;
  out[WSMG_NAV_ATT_PEAK] = (double)peak;
  out[WSMG_NAV_ATT_CHEB] = (double)(dy > dx ? dy : dx);
  out[WSMG_NAV_ATT_EUCLID] = sqrt((double)(dy * dy + dx * dx));
  out[WSMG_NAV_ATT_MASS] = mass;
  out[WSMG_NAV_ATT_ENTROPY] = e;
}

// which state field decides a float field / where a sum's field sits in the row
__constant__ int SUM_FIELD[WSMG_NAV_SUMS] = {WSMG_NAV_ATT_CHEB, WSMG_NAV_ATT_EUCLID, WSMG_NAV_ATT_MASS, WSMG_NAV_ATT_ENTROPY,
                                             WSMG_NAV_ACT_SQ, WSMG_NAV_ACT_L2, WSMG_NAV_ACT_ABS, WSMG_NAV_ACT_ABS + 1,
                                             WSMG_NAV_ACT_ABS + 2, WSMG_NAV_ACT_ABS + 3, WSMG_NAV_PROG_ABS, WSMG_NAV_PROG_SQ};

__device__ __forceinline__ int state_of(int field) {
  return field >= WSMG_NAV_PROG_STATE ? WSMG_NAV_PROG_STATE : field >= WSMG_NAV_ACT_STATE ? WSMG_NAV_ACT_STATE : WSMG_NAV_ATT_STATE;
}

// counts[k] takes a row iff row[state] == want and, where a value field is named, row[field] <= limit (hits) or == limit (stop
// codes): one table walk for every lane, no branch per count (thirteen divergent cases cost 350 us at B = 512)
struct CountRule { int state, want, field, equal; double limit; };
__constant__ CountRule COUNT_RULE[WSMG_NAV_COUNTS] = {
    {WSMG_NAV_ATT_STATE, WSMG_NAV_COUNTED, -1, 0, 0.0},           {WSMG_NAV_ATT_STATE, WSMG_NAV_INVALID, -1, 0, 0.0},
    {WSMG_NAV_ATT_STATE, WSMG_NAV_COUNTED, WSMG_NAV_ATT_CHEB, 0, 0.0}, {WSMG_NAV_ATT_STATE, WSMG_NAV_COUNTED, WSMG_NAV_ATT_CHEB, 0, 1.0},
    {WSMG_NAV_ATT_STATE, WSMG_NAV_COUNTED, WSMG_NAV_ATT_CHEB, 0, 2.0}, {WSMG_NAV_ACT_STATE, WSMG_NAV_COUNTED, -1, 0, 0.0},
    {WSMG_NAV_ACT_STATE, WSMG_NAV_INVALID, -1, 0, 0.0},           {WSMG_NAV_PROG_STATE, WSMG_NAV_COUNTED, -1, 0, 0.0},
    {WSMG_NAV_PROG_STATE, WSMG_NAV_INVALID, -1, 0, 0.0},          {WSMG_NAV_PROG_STATE, WSMG_NAV_COUNTED, WSMG_NAV_PROG_STOP, 1, 0.0},
    {WSMG_NAV_PROG_STATE, WSMG_NAV_COUNTED, WSMG_NAV_PROG_STOP, 1, 1.0}, {WSMG_NAV_PROG_STATE, WSMG_NAV_COUNTED, WSMG_NAV_PROG_STOP, 1, 2.0},
    {WSMG_NAV_PROG_STATE, WSMG_NAV_COUNTED, WSMG_NAV_PROG_STOP, 1, 3.0}};

// The rows come through LDS, FOLD_ROWS at a time, loaded by the whole workgroup (a lane walking global memory row by row pays one
// memory round trip per row: 443 us at B = 512).  Lane t < WSMG_NAV_SUMS of wave 0 owns sums[t], lane k < WSMG_NAV_COUNTS of wave 1
// owns counts[k]; each walks the rows 0 .. B-1 in order.
constexpr int FOLD_ROWS = 256;

__global__ __launch_bounds__(THREADS) void nav_accumulate_kernel(const double* __restrict__ rows, int B, long long* counts, double* sums) {
  __shared__ double tile[FOLD_ROWS * R];
  const int t = threadIdx.x, k = t - 64;
  const bool sums_lane = t < WSMG_NAV_SUMS, counts_lane = k >= 0 && k < WSMG_NAV_COUNTS;
  const int f = sums_lane ? SUM_FIELD[t] : 0, st = state_of(f);
  const CountRule rule = COUNT_RULE[counts_lane ? k : 0];
  const int vf = rule.field < 0 ? rule.state : rule.field;          // no value field: the state stands in, its test always passes
  double s = sums_lane ? sums[t] : 0.0;
  long long c = counts_lane ? counts[k] : 0;
  for (int b0 = 0; b0 < B; b0 += FOLD_ROWS) {
    const int nb = B - b0 < FOLD_ROWS ? B - b0 : FOLD_ROWS;
    for (int i = t; i < nb * R; i += THREADS) tile[i] = rows[(size_t)b0 * R + i];
    __syncthreads();
    if (sums_lane) {
#pragma unroll 8
      for (int b = 0; b < nb; ++b) {
        const double state = tile[b * R + st], v = tile[b * R + f];
        if (state == (double)WSMG_NAV_COUNTED) s += v;
      }
    } else if (counts_lane) {
#pragma unroll 8
      for (int b = 0; b < nb; ++b) {
        const double state = tile[b * R + rule.state], v = tile[b * R + vf];
        const bool pass = rule.field < 0 || (rule.equal ? v == rule.limit : v <= rule.limit);
        c += (state == (double)rule.want && pass) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  if (sums_lane) sums[t] = s;
  if (counts_lane) counts[k] = c;
}

}  // namespace

extern "C" int wsmg_nav_rows(const float* att, const float* dis, int S, int H, int W, const float* pred, const float* waypoint,
                             int ld_waypoint, int A, const float* prog, const float* progress, float stop_threshold,
                             const uint8_t* row_mask, int B, double* rows, wsmg_stream_t stream) {
  if (!rows || B <= 0 || S <= 0 || S > 64 || S * S > CELLS_MAX) return WSMG_EINVAL;
  if ((att != nullptr) != (dis != nullptr) || (pred != nullptr) != (waypoint != nullptr) || (prog != nullptr) != (progress != nullptr))
    return WSMG_EINVAL;
  if (dis && (H <= 0 || W <= 0 || (int64_t)H * W >= (1ll << 31))) return WSMG_EINVAL;
  if (pred && (A < 1 || A > 4 || ld_waypoint < A)) return WSMG_EINVAL;
  NavArgs a{};
  a.att = att; a.dis = dis; a.pred = pred; a.waypoint = waypoint; a.prog = prog; a.progress = progress; a.row_mask = row_mask;
  a.rows = rows; a.S = S; a.H = H; a.W = W; a.A = A; a.ld_waypoint = ld_waypoint; a.thr = stop_threshold;
  hipLaunchKernelGGL(nav_rows_kernel, dim3((unsigned)B), dim3(THREADS), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}

extern "C" int wsmg_nav_accumulate(const double* rows, int B, int64_t* counts, double* sums, wsmg_stream_t stream) {
  if (!rows || !counts || !sums || B <= 0) return WSMG_EINVAL;
  hipLaunchKernelGGL(nav_accumulate_kernel, dim3(1), dim3(THREADS), 0, wsmg_s(stream), rows, B, reinterpret_cast<long long*>(counts), sums);
  WSMG_RETURN_LAUNCH();
}
