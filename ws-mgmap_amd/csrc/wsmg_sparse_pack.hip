// The sparse record form of the ego map (wsmgmap/data/codec.py: sparse_pack_ego), written on the device: the inverse of
// collate_ego_sparse_nhwc_bf16_kernel (wsmg_collate.hip) for one rollout step of B independent rows.
//
// A row is a channels-last float32 map [HW][64] — what wsmg_map_retrieve* writes.  The record stores float16 (common_trainer.py:514-532),
// so every element is cast first (round to nearest even, overflow to inf, subnormals kept) and is PRESENT iff the float16 bit pattern
// is not 0 (-0.0 is present, a float32 that rounds to +0 is not).  Three ordinary launches, no atomics, no workgroup waits on another:
//   1. sparse_pack_bits_kernel   one wave per pixel, lane c = channel c: the ballot of "present" is the pixel's 8 presence bytes as one
//                                little-endian word (channel c = bit c % 8 of byte c / 8); its popcount is parked in off[p]
//   2. sparse_pack_scan_kernel   one workgroup per row turns the counts into the exclusive prefix off[p], 1024 pixels per trip with a
//                                carried prefix; the row's total is nnz[b]
//   3. sparse_pack_vals_kernel   the same wave-per-pixel walk: lane c's value goes to off[p] + popcount(word & lanes below c) of the
//                                row's own region of vals — <= 64 consecutive float16 per pixel, pixel after pixel
// Every output element has exactly one writer at an address that depends on the input alone: the result is the same bit for bit on
// every run.
#include "wsmg_common.h"

namespace {

constexpr int PPW = 16, U = 4;      // pixels per wave and workgroup trip; loads of U pixels in flight (as the expansion kernel)
constexpr int SCAN = 1024;          // pixels per trip of the scan workgroup

__device__ __forceinline__ unsigned short f16_bits(float v) {
  const _Float16 h = (_Float16)v;   // v_cvt_f16_f32: round to nearest even, float16 subnormals kept
  return __builtin_bit_cast(unsigned short, h);
}

__global__ __launch_bounds__(256) void sparse_pack_bits_kernel(const float* __restrict__ x, int HW, unsigned long long* __restrict__ bits,
                                                               unsigned* __restrict__ off) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.y * HW;
  const int p0 = (blockIdx.x * 4 + wave) * PPW;
  unsigned long long mine = 0ull;    // lane i keeps the word of pixel p0 + i: one 128-byte store of the wave's 16 words
  for (int i = 0; i < PPW; i += U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + i + u;
      v[u] = p < HW ? x[(row + p) * 64 + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned long long w = __ballot(f16_bits(v[u]) != 0);
      if (lane == i + u) mine = w;
    }
  }
  if (lane < PPW && p0 + lane < HW) {
    bits[row + p0 + lane] = mine;
    off[row + p0 + lane] = (unsigned)__popcll(mine);
  }
}

__global__ __launch_bounds__(SCAN) void sparse_pack_scan_kernel(int HW, unsigned* __restrict__ off, long long* __restrict__ nnz) {
  __shared__ unsigned wave_total[SCAN / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* const o = off + (size_t)blockIdx.x * HW;
  unsigned carry = 0;                // non-zeros of the row in front of this trip's first pixel (H*W*64 < 2^32: the launcher's check)
  for (int p0 = 0; p0 < HW; p0 += SCAN) {
    const int p = p0 + tid;
    const unsigned c = p < HW ? o[p] : 0u;
    unsigned s = c;                  // inclusive prefix inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    if (lane == 63) wave_total[wave] = s;
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < SCAN / 64; ++k) {
      const unsigned t = wave_total[k];
      before += k < wave ? t : 0u;
      total += t;
    }
    if (p < HW) o[p] = carry + before + s - c;
    carry += total;
    __syncthreads();                 // wave_total is rewritten by the next trip
  }
  if (tid == 0) nnz[blockIdx.x] = (long long)carry;
}

__global__ __launch_bounds__(256) void sparse_pack_vals_kernel(const float* __restrict__ x, int HW, const unsigned* __restrict__ off,
                                                               _Float16* __restrict__ vals) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.y * HW;
  _Float16* const out = vals + row * 64;          // the row's own region: capacity HW * 64
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int p0 = (blockIdx.x * 4 + wave) * PPW;
  for (int i = 0; i < PPW; i += U) {
    float v[U];
    unsigned o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + i + u;
      const bool ok = p < HW;
      v[u] = ok ? x[(row + p) * 64 + lane] : 0.f;
      o[u] = ok ? off[row + p] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const unsigned short h = f16_bits(v[u]);
      const unsigned long long w = __ballot(h != 0);
      // off[p] + popcount(w) <= the row's nnz <= HW * 64: inside the row's region
      if (h != 0) out[(size_t)o[u] + __popcll(w & below)] = __builtin_bit_cast(_Float16, h);
    }
  }
}

}  // namespace

/* One rollout step of the ego map, float32 channels-last [B][HW][64], into the sparse record form (see the header). */
extern "C" int wsmg_ego_sparse_pack(const float* x, int B, int C, int HW, uint8_t* bits, uint32_t* off, int64_t* nnz, void* vals,
                                    wsmg_stream_t stream) {
  if (B <= 0 || B > 65535 || C != 64 || HW <= 0 || (int64_t)HW * 64 > 0xFFFFFFFFll) return WSMG_EINVAL;
  if (!x || !bits || !off || !nnz || !vals || ((uintptr_t)bits & 7)) return WSMG_EINVAL;   // a pixel's 8 bytes are stored as one word
  hipStream_t s = wsmg_s(stream);
  const dim3 grid((unsigned)wsmg_cdiv(HW, 4 * PPW), (unsigned)B);
  hipLaunchKernelGGL(sparse_pack_bits_kernel, grid, dim3(256), 0, s, x, HW, reinterpret_cast<unsigned long long*>(bits), off);
  hipLaunchKernelGGL(sparse_pack_scan_kernel, dim3((unsigned)B), dim3(SCAN), 0, s, HW, off, reinterpret_cast<long long*>(nnz));
  hipLaunchKernelGGL(sparse_pack_vals_kernel, grid, dim3(256), 0, s, x, HW, (const unsigned*)off, (_Float16*)vals);
  WSMG_RETURN_LAUNCH();
}
