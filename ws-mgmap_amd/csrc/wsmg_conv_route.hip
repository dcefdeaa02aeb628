// The route of the bf16 conv engine: which of its nine kernel families takes a layer.  Host arithmetic only — no kernel lives here.
// Every bf16 convolution call (wsmg_conv_bf16.hip) asks wsmg_conv_route once and its launcher switches on the answer; the query entry
// point at the end hands the same answer to tests and tools.  The acceptance tests the route calls belong to the kernels' files
// (declared at the end of wsmg_common.h); the thresholds and the A/B switches are its own.  The tunes (environment, read once per
// process through WSMG_TUNE; no other file of the library reads one of them):
//
//   name                  default  meaning
//   WSMG_CONV_WIN             1    forward of the k8 stem on the LDS-window kernel (wsmg_conv_win.hip); 0: implicit GEMM
//   WSMG_CONV_WIN3            1    the 3 x 3 window kernels: 0 off (the 3 x 3 window weight gradient too), 1 by shape, 512 / 256: that
//                                  tile for every layer it fits — the state wsmg_conv_debug_win3_tile sets.  A forced tile keeps the
//                                  k32 and ConvTranspose kernels off and every launch at one tile size, which is how the tests hold
//                                  the kernels against each other
//   WSMG_CONV_WIN3_N32      256    by shape, 32-channel tiles (N % 64 != 0): the tile; 0: implicit GEMM
//   WSMG_CONV_WIN3_N64        1    by shape, 64-channel tiles (N % 128 != 0): 1 = 512-pixel tiles, 512 / 256: the tile; 0: implicit GEMM
//   WSMG_CONV_WIN3_MIXED      1    by shape, the last partial round of a launch as half-size tiles (round 5); 0: one tile size per
//                                  launch (rounds 2-4)
//   WSMG_CONV_K32             1    a 32-channel reduction axis on wsmg_conv_win3_k32.hip; 0: the general window kernel
//   WSMG_CONV_K32_WGS         6    its workgroups per CU
//   WSMG_CONVT_K4S2           1    the classifier's ConvTranspose2d on wsmg_convt_k4s2.hip; 0: implicit GEMM
//   WSMG_CONVT_WGS            6    its workgroups per CU
//   WSMG_WGRAD_WIN            1    weight gradient of the k8 stem on wsmg_conv_win_wgrad.hip; 0: the generic kernel
//   WSMG_WGRAD_S2WIN          1    of the k5 / k7 stride-2 layers on wsmg_conv_s2_wgrad.hip; 0: the generic kernel
//   WSMG_WGRAD_WIN3           1    of the 3 x 3 layers on wsmg_conv_win3_wgrad.hip; 0: the generic kernel
#include "wsmg_conv_tile.h"

namespace {

int g_win3_tile = -1;
int win3_tile() {   // WSMG_CONV_WIN3
  if (g_win3_tile < 0) g_win3_tile = WSMG_TUNE("WSMG_CONV_WIN3", 1);
  return g_win3_tile;
}
// The LDS-window kernel (wsmg_conv_win3.hip) for a 3 x 3 / stride 1 / pad 1 layer of M pixels, Kc reduction channels and N output
// channels: 0 = no (implicit-GEMM kernel), else pixels per workgroup.  Measured at B = 512 (tools/ab_win3.sh): at Kc = 32 (9
// k-steps) its prologue costs more than the window saves; 512-pixel tiles move half the weight bytes per MFMA of 256-pixel
// ones but need >= 4 rounds of workgroups over the 256 CUs to keep the last round's idle CUs cheap (N = 128 layers: 256).
// round 6: a 32-channel reduction axis takes wsmg_conv_win3_k32.hip (by-shape choice only)
bool k32_choice(int64_t M, int Kc, int N) {
  // (N = 128, the classifier's 32 -> 128 projection: 41 us on either kernel alone, 48.7 against 55.6 us in the update — rocprofv3 --stats)
  return win3_tile() == 1 && Kc == 32 && (N == 32 || N == 64 || N == 128) && M >= 2 * 256 * 256 && WSMG_TUNE("WSMG_CONV_K32", 1) != 0;
}
int win3_choice(int64_t M, int Kc, int N) {
  const int t = win3_tile();
  if (t == 0 || M < 256 * 256 || Kc % 32 || N % 32) return 0;
  if (N % 64) {                      // 32-channel tiles (round 3).
    // The classifier's 32 -> 32 layer at 48 x 48 (B = 512), alone: forward 0.071 -> 0.063 (512-pixel tiles) -> 0.055 ms (256),
    // backward-data 0.075 -> 0.063 -> 0.056: the implicit-GEMM kernel pads the 32 channels to a 64-wide tile and re-fetches the
    // pixels per tap; nine k-steps are too few to hide the window's load, so this is 390 TFLOP/s, not 800
    const int n32 = WSMG_TUNE("WSMG_CONV_WIN3_N32", 256);
    if (t != 1) return t;
    if (n32 == 0 || M < 2 * 256 * 256) return 0;
    return n32;
  }
  if (Kc < 64) return 0;
  if (N % 128) {                     // 64-channel tiles (round 3)
    const int n64 = WSMG_TUNE("WSMG_CONV_WIN3_N64", 1);
    if (t != 1) return t;           // (forced by wsmg_conv_debug_win3_tile / WSMG_CONV_WIN3)
    // measured alone at B = 512, 24 x 24 (tools/bench_conv.py): orig0 (256 -> 64) forward 0.118 -> 0.103 ms, orig2 (192 -> 64)
    // forward 0.091 -> 0.083 and backward-data (64 -> 192) 0.106 -> 0.090; orig1 (64 -> 64: 18 k-steps, one 64-channel tile)
    // 0.037 -> 0.043: that one stays on the implicit-GEMM kernel
    if (n64 == 0 || M < 2 * 256 * 256 || (Kc < 128 && N < 192)) return 0;
    return n64 == 1 ? 512 : n64;
  }
  if (t != 1) return t;
  if (M < 2 * 256 * 256) return 0;   // 12 x 12 maps at B = 512 (73 728 pixels, 128 -> 128): 0.035 vs 0.033 ms
  return ((M + 511) / 512) * (N / 128) >= 1024 ? 512 : 256;
}

// The weight gradient's kernel, and over how many partial sums its reduction is split
WsmgConvRoute wgrad_route(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW) {
  WsmgConvRoute r{WSMG_ROUTE_WGRAD};
  // the map encoder's stem: LDS-window variant
  if (WSMG_TUNE("WSMG_WGRAD_WIN", 1)) {
    if (const int n = wsmg_conv_win_wgrad_splits(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) { r.kind = WSMG_ROUTE_WGRAD_STEM_WIN; r.nsplit = n; return r; }
  }
  // the other two stride-2 layers (k5 64 -> 128, k7 256 -> 64)
  if (WSMG_TUNE("WSMG_WGRAD_S2WIN", 1)) {
    if (const int n = wsmg_conv_s2_wgrad_splits(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) { r.kind = WSMG_ROUTE_WGRAD_S2WIN; r.nsplit = n; return r; }
  }
  // 3 x 3 stride-1 layers: zero-padded LDS window (the tests' tile switch = 0 keeps the generic kernel too)
  const int use_w3w = WSMG_TUNE("WSMG_WGRAD_WIN3", 1);
  if (KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W && use_w3w && win3_tile() && (int64_t)B * H * W >= 256 * 256) {
    if (const int n = wsmg_conv_win3_wgrad_splits(B, H, W, Cin, Cout)) { r.kind = WSMG_ROUTE_WGRAD_WIN3; r.nsplit = n; return r; }
  }
  wsmg_conv_wgrad_plan(B, Cin, Cout, KH, KW, OH, OW, r);   // the generic kernel takes every layer
  return r;
}

}  // namespace

WsmgConvRoute wsmg_conv_route(int pass, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH, int OW, int needs) {
  if (pass == WSMG_CONV_BWD_WEIGHT) return wgrad_route(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW);
  WsmgConvRoute r{WSMG_ROUTE_IGEMM};
  if (needs & WSMG_NEED_F32) return r;                     // a float32 or accumulated output: no window kernel writes one
  const bool bwd = pass == WSMG_CONV_BWD_DATA;
  const bool aux = (needs & (WSMG_NEED_RELU_Y | WSMG_NEED_SPLIT)) != 0;
  // the map encoder's stem: direct convolution out of an LDS-resident input window, into a plain output
  if (!bwd && !(needs & WSMG_NEED_SLICE) && WSMG_TUNE("WSMG_CONV_WIN", 1) && wsmg_conv_win_fits(B, H, W, Cin, Cout, KH, KW, stride, pad)) {
    r.kind = WSMG_ROUTE_STEM_WIN;
    return r;
  }
  if (KH == 3 && KW == 3 && stride == 1 && pad == 1 && OH == H && OW == W) {
    const int64_t M = (int64_t)B * H * W;
    const int Kc = bwd ? Cout : Cin, N = bwd ? Cin : Cout;
    const int wgs = WSMG_TUNE("WSMG_CONV_K32_WGS", 6);
    if (!aux && k32_choice(M, Kc, N) && wsmg_conv_win3_k32_grid(B, H, W, N, wgs)) {      // (no mask, no split output in that kernel)
      r.kind = WSMG_ROUTE_WIN3_K32;
      r.wgs = wgs;
      return r;
    }
    const int mt = win3_choice(M, Kc, N);
    if (mt && wsmg_conv_win3_fits(mt, B, H, W, Kc, N)) {
      r.kind = WSMG_ROUTE_WIN3;
      r.mt = mt;
      r.by_shape = win3_tile() == 1;
      r.mixed = r.by_shape && WSMG_TUNE("WSMG_CONV_WIN3_MIXED", 1) != 0;
      return r;
    }
  }
  // the classifier's ConvTranspose2d(64 -> 32, k4, s2, p1) forward = this backward-data pass (by-shape choice only, like the k32 kernel)
  const int ct_wgs = WSMG_TUNE("WSMG_CONVT_WGS", 6);
  if (bwd && !aux && win3_tile() == 1 && (int64_t)B * OH * OW >= 2 * 256 * 256 && WSMG_TUNE("WSMG_CONVT_K4S2", 1) != 0 &&
      wsmg_convt_k4s2_grid(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, ct_wgs)) {
    r.kind = WSMG_ROUTE_CONVT_K4S2;
    r.wgs = ct_wgs;
  }
  return r;
}

// tests / tools: choose the window kernel's tile (0 = off, 1 = by shape, 256, 512) for the calls that follow; returns the previous choice
extern "C" int wsmg_conv_debug_win3_tile(int mt) {
  const int old = win3_tile();
  if (mt == 0 || mt == 1 || mt == 256 || mt == 512) g_win3_tile = mt;
  return old;
}

// The route of one call, for tests and tools: route[WSMG_ROUTE_WORDS] as include/wsmgmap.h indexes it.  Queues nothing.
extern "C" int wsmg_conv_route_bf16(int pass, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int OH,
                                    int OW, int needs, int* route) {
  const int allowed = pass == WSMG_CONV_FWD ? (WSMG_NEED_F32 | WSMG_NEED_SLICE | WSMG_NEED_STATS)
                    : pass == WSMG_CONV_BWD_DATA ? (WSMG_NEED_F32 | WSMG_NEED_RELU_Y | WSMG_NEED_SPLIT | WSMG_NEED_STATS) : 0;
  if (!route || pass < WSMG_CONV_FWD || pass > WSMG_CONV_BWD_WEIGHT || (needs & ~allowed)) return WSMG_EINVAL;
  if (int e = wsmg_check_conv_bf16(B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW)) return e;
  const WsmgConvRoute r = wsmg_conv_route(pass, B, H, W, Cin, Cout, KH, KW, stride, pad, OH, OW, needs);
  const int words[WSMG_ROUTE_WORDS] = {r.kind, r.mt, r.by_shape, r.nsplit, r.tc, r.tu, r.gx, r.gy, (int)r.chunk};
  for (int i = 0; i < WSMG_ROUTE_WORDS; ++i) route[i] = words[i];
  return 0;
}
