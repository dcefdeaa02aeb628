// What the bf16 MFMA kernels share: vector types, bf16 bit helpers, buffer / LDS-DMA / transposing-read wrappers, the XCD block
// remap, the contract of the staged epilogue's BatchNorm sums, and the launchers' shape helpers.  Every kernel keeps
// its own tiling, pipeline and store loop.
#pragma once
#include "wsmg_common.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short bf16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned short f2bf_bits(float f) {   // round to nearest even
  bf16_t b = (bf16_t)f;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

// raw buffer resource over a tensor: 32-bit byte offsets, out-of-range lanes read 0 (no branches)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ u32x4 buf_load16(__amdgpu_buffer_rsrc_t r, int byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0);
}
// LDS-DMA: 16 bytes per lane from the buffer straight into LDS, lane-linear from the wave's base (1 KB per instruction)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, unsigned char* lds_wave_base, int byte_off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_wave_base, 16, byte_off, 0, 0, 0);
}
// transposing LDS read (ds_read_b64_tr_b16): every lane participates, EXEC must be full
__device__ __forceinline__ bf16x4 tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)(p));
}

// XCD-aware, bijective remap of a 1-D block id: the dispatcher deals blocks round-robin over the
// 8 XCDs, so give each XCD one contiguous run of logical tiles (tiles that share input windows /
// the same A rows then share one L2).  Speed only — any placement is correct.
__device__ __forceinline__ int xcd_swizzle(int bid, int nb) {
  const int q = nb >> 3, r = nb & 7, x = bid & 7;
  return x * q + (x < r ? x : r) + (bid >> 3);
}

// ----------------------------------------------------------------------------- staged epilogue: BatchNorm sums
// The five forward / backward-data kernels (igemm, stem window, 3 x 3 window, its 32-channel form, ConvTranspose k4 s2) stage a 32 x 32
// accumulator tile the same way, each in its own loop (a shared function for the loop changed the kernels' registers and occupancy: it
// is optimised on its own before it is inlined).  C layout of v_mfma_f32_32x32x16_bf16: the lane
// holds ONE column (lane & 31) of the 16 rows (g & 3) + 8 (g >> 2) + 4 h, h = lane >> 5.  Per value: + bias, optional ReLU, round to
// bf16, two bytes into the LDS staging tile the 16-byte stores read.
//
// With `stats`, the train-mode BatchNorm statistics of THIS output (map_encoder.py:10-12 of the reference: every conv of the map stack
// feeds one) are taken on the way: per-channel sum and sum of squares of the bf16-ROUNDED values, from the registers while the tile is
// staged (a second pass over the staged tile was 32-64 two-byte LDS reads per thread, 0.07 ms of the stem), so that the separate
// statistics pass over y (one full read of every conv output) disappears.  Rows past the last pixel count as zero.  The order is fixed
// — sv += vr; qv = fma(vr, vr, qv), g ascending — and the sums end in one of `nslab` float64 slabs (slab = m-tile mod nslab: 72 adders
// per address instead of 4608): lanes r and r + 32 hold different rows of one channel, so a half-wave exchange comes first; then per tile
// (igemm, 3 x 3 window) or once per workgroup run (stem; the 32-channel and ConvTranspose kernels add their four waves in order in LDS).

// ----------------------------------------------------------------------------- host side
// Window entries a tile of mt consecutive pixels of a zero-padded 3 x 3 window (wsmg_conv_win3.hip's geometry) can need: the pixels,
// 2 pads per image row crossed, the pad rows between images, and one padded row + 1 entry of halo on either side
inline int wsmg_win3_window_bound(int mt, int H, int W) {
  const int rows = (mt + W - 2) / W + 1;             // image rows a run of mt pixels can touch
  const int imgs = (mt + H * W - 2) / (H * W) + 1;   // images
  return mt + 2 * (rows - 1) + 2 * (W + 2) * (imgs - 1) + 2 * (W + 3) + 1;
}

// CU count of the current device, asked once per process (inline, not static: one cache for the whole library); 256 — the MI355X —
// where no device can be asked (the plan call of a GPU-less build check)
inline int wsmg_cu_count() {
  static const int cus = []() {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
      return prop.multiProcessorCount;
    return 256;
  }();
  return cus;
}

// Launch of a kernel whose dynamic LDS exceeds the 64 KB default: the limit is raised once per KERNEL INSTANCE (the kernel is a template
// argument, so every instance has its own latch), then the launch; returns the launch error
template <auto kernel, class Args>
int wsmg_launch_dyn_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const Args& args) {
  static bool raised = false;
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return (int)e;
    raised = true;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, args);
  WSMG_RETURN_LAUNCH();
}

// geometry every convolution entry point checks (the bf16 engine adds its 32-bit byte-offset limits: wsmg_check_conv_bf16)
inline int wsmg_check_conv(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0) return WSMG_EINVAL;
  if (Cin % 32 || Cout % 32) return WSMG_EINVAL;
  if (stride != 1 && stride != 2) return WSMG_EINVAL;
  if (OH != (H + 2 * pad - KH) / stride + 1 || OW != (W + 2 * pad - KW) / stride + 1) return WSMG_EINVAL;
  if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)B * OH * OW >= (1ll << 31)) return WSMG_EINVAL;
  return 0;
}
inline int wsmg_check_conv_bf16(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW) {
  if (int e = wsmg_check_conv(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) return e;
  // 32-bit byte offsets into the buffer resources
  if ((int64_t)B * H * W * Cin * 2 >= (1ll << 31) || (int64_t)B * OH * OW * Cout * 2 >= (1ll << 31)) return WSMG_EINVAL;
  return 0;
}
