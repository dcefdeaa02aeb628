// A PPO minibatch in ONE launch: the columns `ind` of every stored rollout tensor, gathered into the minibatch's tensors,
//
//   dst_f[r][j][:] = src_f[r][ind[j]][:]        for every field f, r < rows_f, j < n
//
// src_f is [>= rows_f][N][row_bytes_f], dst_f is [rows_f][n][row_bytes_f], ind is a DEVICE list of n int64 column indices: what
// `src[:rows].index_select(1, ind)` gives per field, an allocation and a launch each, behind a host copy of the index list
// (habitat-baselines' `RolloutStorage.recurrent_generator`, restated: sixteen fields with the update path's observations).  Bytes are
// copied, whatever the dtype; the flattened [rows * n, ...] view of a destination is free.
//
// The table of fields rides in the kernel arguments (GATHER_MAX fields per launch: wsmg_common.h; a longer list is several launches),
// as the multi-tensor Adam's table does; this file keeps its own small table and chunk location (wsmg_optim.hip is not touched).
// A field is copied in units: 16 bytes (one 16-byte load and store per lane) when row_bytes_f is a multiple of 16 and both bases are
// 16-byte aligned, else 4 bytes (the scalar, action and waypoint fields: 4, 8, 12 bytes per row).  One workgroup of 256 threads owns
// GATHER_RUN = 2 048 consecutive destination units of ONE field (32 KB of 16-byte units: the ego-map field at T = 128, n = 4,
// 2.56 MB rows is 40 000 workgroups); its field is found by bisection of the block prefix, its first unit is a multiple of
// GATHER_RUN.  Consecutive lanes own consecutive units, so a wave's stores are 1 KB contiguous and its loads are contiguous
// within a source row; every thread has its GATHER_PER = 8 loads in flight before its first store.
//
// Offsets.  A field's units and bytes exceed 2^31 (the ego map: 1.3 GB), so every unit offset is `long long`.  What stays in 32
// bits, by the launcher's checks: rows_f n (destination rows) and the units per row.  The workgroup divides its first unit by the
// units per row ONCE (uniform, 64-bit); a lane's (row, unit in row) follows by 32-bit divisions.
//
// A column index outside [0, N) copies nothing: the lane skips its load and its store (the destination keeps what it held).  No
// index ever becomes an address unchecked.  No LDS, no atomics; plain loads and stores only.
#include "wsmg_common.h"

#include <climits>

namespace {

// the unit below is a u32x4, 16 bytes: one global_load_dwordx4 / store per lane
constexpr int GATHER_PER = 8;                     // units per thread, all loaded before the first store
constexpr int GATHER_RUN = 256 * GATHER_PER;      // consecutive destination units of one field per workgroup

struct GatherTable {
  const char* src[GATHER_MAX];
  char* dst[GATHER_MAX];
  int first_block[GATHER_MAX + 1];  // prefix of workgroups per field
  int upr[GATHER_MAX];              // units per row
  int drows[GATHER_MAX];            // destination rows, rows_f * n
  int wide[GATHER_MAX];             // 16-byte units (else 4-byte)
  int count;
};

// This workgroup's field: f with first_block[f] <= blockIdx.x < first_block[f + 1].
__device__ __forceinline__ int gather_field(const GatherTable& tb) {
  int lo = 0, hi = tb.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int)blockIdx.x >= tb.first_block[mid]) lo = mid; else hi = mid;
  }
  return lo;
}

// Units [u0, u0 + GATHER_RUN) of a destination of `drows` rows of `upr` units U; source rows are N per step, destination rows n.
template <class U>
__device__ __forceinline__ void gather_run(const U* __restrict__ src, U* __restrict__ dst, long long u0, int upr, int drows, int n,
                                           int N, const long long* __restrict__ ind) {
  const long long q0 = u0 / upr;                  // first destination row of the run (uniform)
  const unsigned w0 = (unsigned)(u0 - q0 * upr);  // and the unit in it: w0 + t < upr + GATHER_RUN <= INT_MAX
  U v[GATHER_PER];
  bool ok[GATHER_PER];
#pragma unroll
  for (int k = 0; k < GATHER_PER; ++k) {
    const unsigned t = threadIdx.x + 256u * k;
    const unsigned dq = (w0 + t) / (unsigned)upr;
    const unsigned w = (w0 + t) - dq * (unsigned)upr;
    const long long q = q0 + dq;                  // destination row r * n + j
    ok[k] = q < drows;
    if (ok[k]) {
      const unsigned r = (unsigned)q / (unsigned)n;
      const unsigned j = (unsigned)q - r * (unsigned)n;
      const long long c = ind[j];
      ok[k] = c >= 0 && c < N;
      if (ok[k]) v[k] = src[((long long)r * N + c) * upr + w];
    }
  }
#pragma unroll
  for (int k = 0; k < GATHER_PER; ++k)
    if (ok[k]) dst[u0 + threadIdx.x + 256 * k] = v[k];
}

__global__ __launch_bounds__(256) void rollout_gather_kernel(GatherTable tb, const long long* __restrict__ ind, int n, int N) {
  const int f = gather_field(tb);
  const char* src = tb.src[f];
  char* dst = tb.dst[f];
  const int upr = tb.upr[f], drows = tb.drows[f];
  const long long u0 = (long long)((int)blockIdx.x - tb.first_block[f]) * GATHER_RUN;
  if (tb.wide[f]) gather_run(reinterpret_cast<const u32x4*>(src), reinterpret_cast<u32x4*>(dst), u0, upr, drows, n, N, ind);
  else gather_run(reinterpret_cast<const unsigned*>(src), reinterpret_cast<unsigned*>(dst), u0, upr, drows, n, N, ind);
}

struct GatherField {        // one checked entry of the launcher's four host arrays
  void* dst;
  const void* src;
  long long rows, row_bytes;
};

// 16-byte units: rows of a multiple of 16 bytes between 16-byte aligned bases
static bool gather_wide(const GatherField& d) {
  return !(d.row_bytes & 15) && !(((uintptr_t)d.src | (uintptr_t)d.dst) & 15);
}

// the workgroups of a checked field with rows
static long long gather_blocks(const GatherField& d, int n) {
  const long long units = d.rows * (long long)n * (d.row_bytes / (gather_wide(d) ? 16 : 4));
  return (units + GATHER_RUN - 1) / GATHER_RUN;
}

}  // namespace

extern "C" int wsmg_rollout_gather(void* const* dst, const void* const* src, const long long* rows, const long long* row_bytes,
                                   int n_fields, const int64_t* ind, int n, int N, wsmg_stream_t stream) {
  if (n_fields < 0 || (n_fields > 0 && (!dst || !src || !rows || !row_bytes))) return WSMG_EINVAL;
  if (!ind || ((uintptr_t)ind & 7) || n < 1 || N < 1) return WSMG_EINVAL;
  const auto field = [&](int i) { return GatherField{dst[i], src[i], rows[i], row_bytes[i]}; };
  // every field is checked before the first launch
  for (int i = 0; i < n_fields; ++i) {
    const GatherField d = field(i);
    if (d.rows < 0 || d.row_bytes <= 0 || (d.row_bytes & 3)) return WSMG_EINVAL;
    if (((uintptr_t)d.src | (uintptr_t)d.dst) & 3) return WSMG_EINVAL;
    if (d.rows > 0 && (!d.src || !d.dst)) return WSMG_EINVAL;
    if (d.rows > INT_MAX || d.rows * (long long)n > INT_MAX) return WSMG_EINVAL;
    if (d.row_bytes / 4 > INT_MAX - GATHER_RUN) return WSMG_EINVAL;
    if (gather_blocks(d, n) > INT_MAX) return WSMG_EINVAL;       // one field beyond a grid (2^42 bytes)
  }
  GatherTable tb;
  for (int i = 0; i < n_fields;) {
    tb.count = 0;
    long long blocks = 0;
    for (; i < n_fields && tb.count < GATHER_MAX; ++i) {
      const GatherField d = field(i);
      if (d.rows == 0) continue;                  // owns no workgroup and no table entry
      const bool wide = gather_wide(d);
      const long long nb = gather_blocks(d, n);
      if (blocks + nb > INT_MAX) break;           // the grid is full: this field opens the next launch
      const int k = tb.count++;
      tb.src[k] = static_cast<const char*>(d.src);
      tb.dst[k] = static_cast<char*>(d.dst);
      tb.upr[k] = (int)(d.row_bytes / (wide ? 16 : 4));
      tb.drows[k] = (int)(d.rows * n);
      tb.wide[k] = wide;
      tb.first_block[k] = (int)blocks;
      blocks += nb;
    }
    if (!tb.count) continue;
    tb.first_block[tb.count] = (int)blocks;
    hipLaunchKernelGGL(rollout_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, wsmg_s(stream), tb,
                       reinterpret_cast<const long long*>(ind), n, N);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}
