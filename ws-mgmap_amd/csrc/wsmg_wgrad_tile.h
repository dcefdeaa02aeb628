// What the five weight-gradient kernels share (conv_wgrad_kernel, conv_wgrad_bf16_kernel, conv_win_wgrad_kernel, conv_s2_wgrad_kernel,
// conv_win3_wgrad_kernel): the transposing-read lane map, the fragment assembly, the accumulator flush and the persistent kernels'
// (role, tile group) numbering.  Tiling, LDS layout, staging loops, scheduling interleaves and fragment rings stay per kernel.
// (conv_win3_wgrad_kernel follows the same rules in its own spelling: through these helpers it measured slower, profiles/wgrad_once.txt.)
#pragma once
#include "wsmg_conv_tile.h"

// Transposing-read lane map.  The reduction axis (pixels) is the strided axis of NHWC for both operands, so both are read with tr_read:
// the lane supplies the address of pixel 8 h + q4 of a 16-pixel MFMA step (+ 4 for the second read) and channels 16 half16 + 4 p4 .. + 3
// of its 32-channel tile (chan_off, bytes); the hardware hands each lane 4 pixels of ITS channel.  Every lane takes part (EXEC full).
struct TrLane {
  const int li, q4, p4, half16, h, chan_off;
  __device__ __forceinline__ explicit TrLane(int lane)
      : li(lane & 15), q4(li >> 2), p4(li & 3), half16((lane >> 4) & 1), h(lane >> 5), chan_off((half16 * 16 + p4 * 4) * 2) {}
};

// one MFMA operand (8 pixels of the lane's channel) out of two transposing reads four pixels apart: at lo and hi, or step_bytes per pixel
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* lo, const unsigned char* hi) {
  const bf16x4 l = tr_read(lo), hh = tr_read(hi);
  return __builtin_shufflevector(l, hh, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* p, int step_bytes) { return tr_frag(p, p + 4 * step_bytes); }

// Flush of one 32 x 32 float32 accumulator tile into dW (OHWI: [Cout][taps][Cin]).  C layout of the 32 x 32 MFMAs: the lane holds ONE
// column — input channel ci, consecutive over lane & 31: 128-byte segments of an OHWI row — of the 16 rows co0 + (g & 3) + 8 (g >> 2) + 4 h,
// h = lane >> 5.  slab > 0 (floats per slab, the deterministic form): the workgroup STORES into slab `part` of the workspace dw — every
// element of every slab is written exactly once, nothing is zeroed beforehand, wsmg_weight_grad_reduce_oihw adds the slabs in order.
// slab == 0: float atomics into a dW the caller zeroed.  live == false is a workgroup that found no work (a tile group beyond the tile
// count): its accumulators are zero, it STORES them into its slab and ADDS NOTHING in the atomic form.
__device__ __forceinline__ void wgrad_flush_tile(const f32x16& acc, float* dw, int64_t slab, int part, int co0, int taps, int tap, int Cin,
                                                 int ci, int h, bool live) {
  auto at = [&](int g) { return dw + (size_t)part * slab + ((size_t)(co0 + (g & 3) + 8 * (g >> 2) + 4 * h) * taps + tap) * Cin + ci; };
  if (slab) {   // (one branch per tile, not per element: the 16 stores then issue back to back)
#pragma unroll
    for (int g = 0; g < 16; ++g) *at(g) = acc[g];
  } else if (live) {
#pragma unroll
    for (int g = 0; g < 16; ++g) atomicAdd(at(g), acc[g]);
  }
}

// Persistent window kernels: workgroup -> (role, tile group), R roles per group.  Consecutive block ids go round the 8 XCDs, and the roles
// of a group read the same dY tiles and overlapping input rows at about the same time, so they share an XCD (its L2): local index
// i = bid / 8 on XCD bid % 8 -> role i % R, group (bid % 8) + 8 (i / R).  (With the k8 stem's roles spread over the XCDs, role = bid % 8,
// that kernel moved 4.2 GB through the fabric in 0.78 ms and waited on it.)
__device__ __forceinline__ void wgrad_role_group(unsigned bid, unsigned R, int& role, int& grp) {
  const unsigned xcd = bid & 7, i = bid >> 3;
  role = (int)(i % R);
  grp = (int)(xcd + 8 * (i / R));
}
// tile groups of such a grid (= slabs of the deterministic form): at most `want`, no more than tiles, whole XCD rounds — a group beyond
// the tile count finds no tile and flushes as wgrad_flush_tile's `live` says
inline int wgrad_groups(int want, int ntiles) { return ((want < ntiles ? want : ntiles) + 7) / 8 * 8; }
