// Layout changes at the engine's boundaries; nothing here does arithmetic beyond the deterministic slab sum:
//   - the NCHW <-> NHWC transposes of activations (with channel padding and the float32 -> bf16 conversion fused),
//   - the conv weight re-layouts OIHW -> OHWI / IHWO in the compute dtype, one parameter or a batch of them per launch,
//   - the weight gradient's way back: OHWI float32 -> OIHW, alone or as the last step of the deterministic slab reduction.
// Reference call sites: map_encoder.py:80, mg_map_policy.py:89-100,197 (the layouts torch keeps implicit).
#include <type_traits>

#include "wsmg_common.h"

namespace {

// ---- [B][R][S] -> [B][S][R'] transposes through a 32x33 LDS tile (coalesced both sides)
// TO_NHWC: src rows = channels (R = C_src), cols = pixels;  dst [pixel][C_dst], zero-filled past C_src.
template <bool TO_NHWC, class TI, class TO>
__global__ __launch_bounds__(256) void transpose_kernel(const TI* x, TO* y, int C_src, int HW, int C_dst) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  if (TO_NHWC) {
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int c = c0 + ty + 8 * j, p = p0 + tx;
      tile[ty + 8 * j][tx] = (c < C_src && p < HW) ? ldf(x + ((size_t)b * C_src + c) * HW + p) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int p = p0 + ty + 8 * j, c = c0 + tx;
      if (p < HW && c < C_dst) stf(y + ((size_t)b * HW + p) * C_dst + c, tile[tx][ty + 8 * j]);
    }
  } else {
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int p = p0 + ty + 8 * j, c = c0 + tx;
      tile[ty + 8 * j][tx] = (p < HW && c < C_src) ? ldf(x + ((size_t)b * HW + p) * C_src + c) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int c = c0 + ty + 8 * j, p = p0 + tx;
      if (c < C_dst && p < HW) stf(y + ((size_t)b * C_dst + c) * HW + p, tile[tx][ty + 8 * j]);
    }
  }
}

// NCHW float32 -> NHWC (float32 / bf16) for C_src % 64 == 0, HW % 4 == 0: 64 channels x 64 pixels per workgroup,
// 16-byte loads along the pixel axis and 16-byte (bf16: 8 channels) / 2 x 16-byte (f32) stores along the
// channel axis.  The cached ego map of the update path (1.3 GB per update) goes through this once.
template <class TO>
__global__ __launch_bounds__(256) void nchw_to_nhwc64_kernel(const float* __restrict__ x, TO* __restrict__ y, int C_src, int HW,
                                                             int C_dst) {
  __shared__ float tile[64][65];
  const int b = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int id = tid + 256 * j;         // 1024 float4 pieces: 16 per channel row
    const int c = id >> 4, pq = (id & 15) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (p0 + pq < HW) v = *reinterpret_cast<const f32x4*>(x + ((size_t)b * C_src + c0 + c) * HW + p0 + pq);
    tile[c][pq] = v[0]; tile[c][pq + 1] = v[1]; tile[c][pq + 2] = v[2]; tile[c][pq + 3] = v[3];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int id = tid + 256 * j;         // 512 pieces of 8 channels: 8 per pixel
    const int p = id >> 3, cs = (id & 7) * 8;
    if (p0 + p < HW) {
      f32x4 lo = {tile[cs][p], tile[cs + 1][p], tile[cs + 2][p], tile[cs + 3][p]};
      f32x4 hi = {tile[cs + 4][p], tile[cs + 5][p], tile[cs + 6][p], tile[cs + 7][p]};
      TO* dst = y + ((size_t)b * HW + p0 + p) * C_dst + c0 + cs;
      st4(dst, lo);
      st4(dst + 4, hi);
    }
  }
}

// flat index of an OHWI tensor [O][KH][KW][I_pad] -> its four coordinates
struct OhwiPos { int o, kh, kw, i; };
__device__ __forceinline__ OhwiPos ohwi_decode(int64_t idx, int KH, int KW, int I_pad) {
  OhwiPos p;
  p.i = (int)(idx % I_pad);
  int64_t r = idx / I_pad;
  p.kw = (int)(r % KW); r /= KW;
  p.kh = (int)(r % KH);
  p.o = (int)(r / KH);
  return p;
}

// ---- conv weight layouts in one launch: OIHW float32 parameter -> OHWI (forward / weight-gradient operand) and IHWO
// (backward-data operand) in the compute dtype, input channels zero-padded to I_pad.  Replaces per layer and update a
// permute copy, a dtype cast, a second permute copy (and an F.pad when the engine pads channels).  One parameter's pass, a
// grid-stride loop over blockIdx.x:
template <class T>
__device__ __forceinline__ void weight_relayout_body(const float* __restrict__ w, int O, int I, int KH, int KW, int I_pad,
                                                     T* __restrict__ ohwi, T* __restrict__ ihwo) {
  const int64_t n = (int64_t)O * KH * KW * I_pad;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const OhwiPos p = ohwi_decode(idx, KH, KW, I_pad);
    const float v = p.i < I ? w[(((int64_t)p.o * I + p.i) * KH + p.kh) * KW + p.kw] : 0.f;
    stf(ohwi + idx, v);
    if (ihwo) stf(ihwo + (((int64_t)p.i * KH + p.kh) * KW + p.kw) * O + p.o, v);
  }
}
template <class T>
__global__ __launch_bounds__(256) void weight_relayout_kernel(const float* __restrict__ w, int O, int I, int KH, int KW, int I_pad,
                                                              T* __restrict__ ohwi, T* __restrict__ ihwo) {
  weight_relayout_body<T>(w, O, I, KH, KW, I_pad, ohwi, ihwo);
}
// the same for up to WSMG_RELAYOUT_MAX parameters in ONE launch (blockIdx.y = parameter): the map stack has 20 convolutions,
// and 20 five-microsecond launches in front of them were 0.1 ms of the forward pass's critical path
struct RelayoutBatch { WsmgRelayoutDesc d[WSMG_RELAYOUT_MAX]; };
template <class T>
__global__ __launch_bounds__(256) void weight_relayout_multi_kernel(RelayoutBatch b) {
  const WsmgRelayoutDesc& d = b.d[blockIdx.y];
  weight_relayout_body<T>(d.w_oihw, d.O, d.I, d.KH, d.KW, d.I_pad, (T*)d.w_ohwi, (T*)d.w_ihwo);
}
// dW [O][KH][KW][I_pad] float32 -> the parameter's OIHW gradient (padded channels dropped); the loop runs over the OIHW index
__global__ __launch_bounds__(256) void weight_grad_to_oihw_kernel(const float* __restrict__ dw, int O, int I, int KH, int KW,
                                                                  int I_pad, float* __restrict__ out) {
  const int64_t n = (int64_t)O * I * KH * KW;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * 256) {
    const int kw = (int)(idx % KW);
    int64_t r = idx / KW;
    const int kh = (int)(r % KH); r /= KH;
    const int i = (int)(r % I);
    const int o = (int)(r / I);
    out[idx] = dw[(((int64_t)o * KH + kh) * KW + kw) * I_pad + i];
  }
}

// The deterministic weight gradient's last step: dW[o][i][kh][kw] (OIHW, i < I) = sum over z < nsplit of ws[z][o][kh][kw][i]
// (OHWI slabs of I_pad channels, written whole by the weight-gradient kernels' workgroups — wsmg_conv2d_bwd_weight*_slabs).
// The order of the additions depends on nsplit only — four z ranges summed in z order by four threads, their results added
// in range order — so dW is bit-identical from run to run (float atomics add in arrival order).  A thread owns 4 consecutive
// input channels (one 16-byte load per slab); the OIHW stores are 4-byte, KH*KW apart: dW is 10-40x smaller than the slabs.
__global__ __launch_bounds__(256) void weight_grad_reduce_oihw_kernel(const float* __restrict__ ws, int nsplit, int64_t slab4, int I,
                                                                      int KH, int KW, int I_pad, float* __restrict__ out) {
  __shared__ f32x4 part[3][64];
  const int ql = threadIdx.x & 63, zp = threadIdx.x >> 6;
  const int64_t q = (int64_t)blockIdx.x * 64 + ql;
  const int per = (nsplit + 3) >> 2;
  const int z0 = zp * per, z1 = z0 + per < nsplit ? z0 + per : nsplit;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (q < slab4) {
    const f32x4* p = reinterpret_cast<const f32x4*>(ws) + (int64_t)z0 * slab4 + q;
    int z = z0;
    for (; z + 4 <= z1; z += 4, p += 4 * slab4) {     // four loads in flight, added in z order
      const f32x4 a = p[0], b = p[slab4], c = p[2 * slab4], d = p[3 * slab4];
      acc += a; acc += b; acc += c; acc += d;
    }
    for (; z < z1; ++z, p += slab4) acc += p[0];
  }
  if (zp) part[zp - 1][ql] = acc;
  __syncthreads();
  if (zp || q >= slab4) return;
  acc += part[0][ql]; acc += part[1][ql]; acc += part[2][ql];
  const OhwiPos p = ohwi_decode(q * 4, KH, KW, I_pad);       // the first of the thread's 4 channels
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p.i + j < I) out[(((int64_t)p.o * I + p.i + j) * KH + p.kh) * KW + p.kw] = acc[j];
}

template <bool TO_NHWC, class TI, class TO>
int transpose_t(const TI* x, TO* y, int B, int C_src, int H, int W, int C_dst, wsmg_stream_t stream) {
  if (B <= 0 || C_src <= 0 || C_dst <= 0 || H <= 0 || W <= 0 || B > 65535) return WSMG_EINVAL;
  int HW = H * W;
  if constexpr (TO_NHWC && std::is_same<TI, float>::value) {
    if (C_src == C_dst && C_src % 64 == 0 && HW % 4 == 0) {
      dim3 g64((unsigned)wsmg_cdiv(HW, 64), (unsigned)(C_src / 64), (unsigned)B);
      hipLaunchKernelGGL((nchw_to_nhwc64_kernel<TO>), g64, dim3(256), 0, wsmg_s(stream), x, y, C_src, HW, C_dst);
      WSMG_RETURN_LAUNCH();
    }
  }
  dim3 grid((unsigned)wsmg_cdiv(HW, 32), (unsigned)wsmg_cdiv(TO_NHWC ? C_dst : (C_dst > C_src ? C_dst : C_src), 32), (unsigned)B);
  hipLaunchKernelGGL((transpose_kernel<TO_NHWC, TI, TO>), grid, dim3(256), 0, wsmg_s(stream), x, y, C_src, HW, C_dst);
  WSMG_RETURN_LAUNCH();
}

// what every weight layout call asks of its shape
bool weight_shape_ok(int O, int I, int KH, int KW, int I_pad) { return O > 0 && I > 0 && KH > 0 && KW > 0 && I_pad >= I; }

template <class T>
int weight_relayout_t(const float* w_oihw, int O, int I, int KH, int KW, int I_pad, T* w_ohwi, T* w_ihwo, wsmg_stream_t s) {
  if (!weight_shape_ok(O, I, KH, KW, I_pad)) return WSMG_EINVAL;
  hipLaunchKernelGGL(weight_relayout_kernel<T>, dim3(wsmg_sgrid((int64_t)O * KH * KW * I_pad)), dim3(256), 0, wsmg_s(s), w_oihw, O, I, KH,
                     KW, I_pad, w_ohwi, w_ihwo);
  WSMG_RETURN_LAUNCH();
}

}  // namespace

#define B16(p) ((bf16_t*)(p))
#define CB16(p) ((const bf16_t*)(p))
extern "C" int wsmg_nchw_to_nhwc(const float* x, float* y, int B, int C_src, int H, int W, int C_dst, wsmg_stream_t s) { return transpose_t<true, float, float>(x, y, B, C_src, H, W, C_dst, s); }
extern "C" int wsmg_nchw_to_nhwc_bf16(const float* x, void* y, int B, int C_src, int H, int W, int C_dst, wsmg_stream_t s) { return transpose_t<true, float, bf16_t>(x, B16(y), B, C_src, H, W, C_dst, s); }
extern "C" int wsmg_nhwc_to_nchw(const float* x, float* y, int B, int C_src, int H, int W, int C_dst, wsmg_stream_t s) { return transpose_t<false, float, float>(x, y, B, C_src, H, W, C_dst, s); }
extern "C" int wsmg_nhwc_to_nchw_bf16(const void* x, float* y, int B, int C_src, int H, int W, int C_dst, wsmg_stream_t s) { return transpose_t<false, bf16_t, float>(CB16(x), y, B, C_src, H, W, C_dst, s); }

extern "C" int wsmg_weight_relayout(const float* w_oihw, int O, int I, int KH, int KW, int I_pad, float* w_ohwi, float* w_ihwo, wsmg_stream_t s) { return weight_relayout_t<float>(w_oihw, O, I, KH, KW, I_pad, w_ohwi, w_ihwo, s); }
extern "C" int wsmg_weight_relayout_bf16(const float* w_oihw, int O, int I, int KH, int KW, int I_pad, void* w_ohwi, void* w_ihwo, wsmg_stream_t s) { return weight_relayout_t<bf16_t>(w_oihw, O, I, KH, KW, I_pad, B16(w_ohwi), B16(w_ihwo), s); }
extern "C" int wsmg_weight_relayout_multi(const WsmgRelayoutDesc* descs, int n, int bf16, wsmg_stream_t s) {
  if (!descs || n <= 0) return WSMG_EINVAL;
  for (int i0 = 0; i0 < n; i0 += WSMG_RELAYOUT_MAX) {
    RelayoutBatch b;
    const int m = n - i0 < WSMG_RELAYOUT_MAX ? n - i0 : WSMG_RELAYOUT_MAX;
    for (int i = 0; i < m; ++i) {
      const WsmgRelayoutDesc& d = b.d[i] = descs[i0 + i];
      if (!weight_shape_ok(d.O, d.I, d.KH, d.KW, d.I_pad) || !d.w_oihw || !d.w_ohwi) return WSMG_EINVAL;
    }
    if (bf16) hipLaunchKernelGGL(weight_relayout_multi_kernel<bf16_t>, dim3(48, (unsigned)m), dim3(256), 0, wsmg_s(s), b);
    else hipLaunchKernelGGL(weight_relayout_multi_kernel<float>, dim3(48, (unsigned)m), dim3(256), 0, wsmg_s(s), b);
  }
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_weight_grad_reduce_oihw(const float* ws, int nsplit, int O, int I, int KH, int KW, int I_pad, float* dw_oihw,
                                            wsmg_stream_t s) {
  if (!ws || !dw_oihw || nsplit <= 0 || !weight_shape_ok(O, I, KH, KW, I_pad) || (I_pad & 3)) return WSMG_EINVAL;
  const int64_t slab4 = (int64_t)O * KH * KW * I_pad / 4;
  hipLaunchKernelGGL(weight_grad_reduce_oihw_kernel, dim3((unsigned)wsmg_cdiv(slab4, 64)), dim3(256), 0, wsmg_s(s), ws, nsplit, slab4, I,
                     KH, KW, I_pad, dw_oihw);
  WSMG_RETURN_LAUNCH();
}
extern "C" int wsmg_weight_grad_to_oihw(const float* dw_ohwi, int O, int I, int KH, int KW, int I_pad, float* dw_oihw, wsmg_stream_t s) {
  if (!weight_shape_ok(O, I, KH, KW, I_pad)) return WSMG_EINVAL;
  hipLaunchKernelGGL(weight_grad_to_oihw_kernel, dim3(wsmg_sgrid((int64_t)O * I * KH * KW)), dim3(256), 0, wsmg_s(s), dw_ohwi, O, I, KH, KW,
                     I_pad, dw_oihw);
  WSMG_RETURN_LAUNCH();
}
