// Backward of the shared-set e4m3 attention of wsmg_attn_fp8_mfma.hip (BASELINE configs[4], mg_map_policy.py:173-178) on the matrix
// cores.  With q^, K^_u, V^_u the de-quantised operands (code * per-tensor scale), p the attention weights the forward wrote:
//     dp   = dout V^_u^T + dattn             [R_u x L]    contraction over the 256 channels
//     dl   = p o (dp - sum_l p o dp)                      float32
//     dq   = scale * dl K^_u                 [R_u x 256]  contraction over the L tokens
//     dK_u = scale * sum_{b in u} dl_b^T q^_b   [L x 256] contraction over the rows of the set
//     dV_u =         sum_{b in u} p_b^T dout_b  [L x 256]
// All four run on v_mfma_f32_32x32x16_bf16.  Operands that come from e4m3 codes convert to bf16 exactly and get their scale in float32
// afterwards; the float32 operands (dout, p, dl) go in as bf16 (hi, lo) pairs — hi = bf16(x), lo = bf16(x - hi), 16 significant bits —
// as the forward treats P.  p o dout, a product of two pairs, takes all four partial products.
//
// Two launches:
//   rows kernel: one workgroup per (set, tile of 32 of its rows), rows addressed through the forward's row_ids / set_start; dp into an
//                LDS tile, the softmax gradient, dl to the [B][L] scratch, dq.
//   sets kernel: one workgroup per (set, block of 32 tokens).  It walks ALL rows of its set, 32 at a time, in ascending row index (a
//                ranked scan of `inverse`, as the fused forward finds its rows: row_ids orders the rows inside a set arbitrarily), so the
//                reduction over the rows is inside one workgroup, in one order: dK_u and dV_u are bit-reproducible, no float atomics, no
//                partial blocks.  A set no row uses gets zeros; tokens at or past lengths[u] have p = 0 exactly, hence dl = 0 and zero
//                gradient rows; rows past the end of a partial chunk are staged as zeros.
// No [B][L][256] or [U][B][L] tensor exists.
#include "wsmg_attn_common.h"
#include "wsmg_conv_tile.h"

namespace {

struct F8bArgs {
  const uint8_t* q;        // [B][256] e4m3
  const uint8_t* k;        // [U][L][256]
  const uint8_t* v;        // [U][L][256]
  const float* q_scale;    // device scalars
  const float* k_scale;
  const float* v_scale;
  const int* row_ids;      // [B] row indices grouped by set
  const int* set_start;    // [U + 1]
  const int64_t* inverse;  // [B]
  const float* attn;       // [B][L] the forward's weights
  const float* dout;       // [B][256] or null
  const float* dattn;      // [B][L] or null
  float scale;
  int B, U, L;
  float* dq;               // [B][256]
  float* dk;               // [U][L][256]
  float* dv;               // [U][L][256]
  float* dl;               // [B][L] scratch: d logits
};

__device__ __forceinline__ void split8(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const unsigned short h = f2bf_bits(x[s]);
    hi[s] = (short)h;
    lo[s] = (short)f2bf_bits(x[s] - bf2f(h));
  }
}
// MFMA 32x32x16 operand layout, as the forward uses it: A lane (r, h) = row r, k = 8 h .. 8 h + 7; B lane (r, h) = column r, k likewise;
// D lane (r = column, h), register g -> row (g & 3) + 8 (g >> 2) + 4 h.
__global__ __launch_bounds__(256) void attn_fp8_mfma_bwd_rows_kernel(F8bArgs a) {
  __shared__ __attribute__((aligned(16))) float S[32][F8_MAX_L + 4];
  __shared__ __attribute__((aligned(16))) uint8_t K8[2][32][AC + 16];      // two chunks of 32 tokens x 256 key bytes
  __shared__ int rows[32];
  const int u = blockIdx.x, tile = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int s0 = a.set_start[u], nrows_set = a.set_start[u + 1] - s0;
  const int first = tile * 32;
  if (first >= nrows_set) return;
  const int nr = nrows_set - first < 32 ? nrows_set - first : 32;
  if (tid < 32) rows[tid] = tid < nr ? a.row_ids[s0 + first + tid] : -1;
  __syncthreads();
  const int LP = (a.L + 31) & ~31;
  const float sk = *a.k_scale, sv = *a.v_scale;

  // ---- dp = dout V^T: A = dout rows as a bf16 pair, B = token r's value codes (8 consecutive channels per lane)
  if (a.dout) {
    const int my_row = rows[r];
    const float* dp_ = a.dout + (size_t)(my_row < 0 ? 0 : my_row) * AC + 8 * h;
    bf16x8 ahi[16], alo[16];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (my_row >= 0) {
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(dp_ + 16 * ks), x1 = *reinterpret_cast<const f32x4*>(dp_ + 16 * ks + 4);
        x[0] = x0[0]; x[1] = x0[1]; x[2] = x0[2]; x[3] = x0[3]; x[4] = x1[0]; x[5] = x1[1]; x[6] = x1[2]; x[7] = x1[3];
      }
      split8(x, ahi[ks], alo[ks]);
    }
    for (int tt = wave; tt * 32 < LP; tt += 4) {
      const int tok = tt * 32 + r;
      const uint8_t* vp = a.v + ((size_t)u * a.L + (tok < a.L ? tok : 0)) * AC + 8 * h;
      long vb8[16];
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) vb8[ks] = tok < a.L ? *reinterpret_cast<const long*>(vp + 16 * ks) : 0l;
      f32x16 acc_hi, acc_lo;
#pragma unroll
      for (int g = 0; g < 16; ++g) { acc_hi[g] = 0.f; acc_lo[g] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const bf16x8 vb = e4m3_dec8_bf(vb8[ks]);
        acc_hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi[ks], vb, acc_hi, 0, 0, 0);
        acc_lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo[ks], vb, acc_lo, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int m = (g & 3) + 8 * (g >> 2) + 4 * h;
        S[m][tok] = (acc_hi[g] + acc_lo[g]) * sv;
      }
    }
  }
  __syncthreads();

  // ---- softmax gradient in float32, 8 lanes per row; dl to the scratch and, in LDS, as the A operand of dq
  {
    const int row = tid >> 3, sub = tid & 7;
    const int gr = rows[row];
    if (gr >= 0) {
      const float* pr = a.attn + (size_t)gr * a.L;
      float sum = 0.f;
      for (int l = sub; l < a.L; l += 8) {
        float dp = a.dout ? S[row][l] : 0.f;
        if (a.dattn) dp += a.dattn[(size_t)gr * a.L + l];
        S[row][l] = dp;
        sum += pr[l] * dp;
      }
      sum += __shfl_xor(sum, 4, 64);
      sum += __shfl_xor(sum, 2, 64);
      sum += __shfl_xor(sum, 1, 64);
      for (int l = sub; l < LP; l += 8) {
        float dl = 0.f;
        if (l < a.L) {
          dl = pr[l] * (S[row][l] - sum);
          a.dl[(size_t)gr * a.L + l] = dl;
        }
        S[row][l] = dl;
      }
    } else {
      for (int l = sub; l < LP; l += 8) S[row][l] = 0.f;
    }
  }
  __syncthreads();

  // ---- dq = scale * dl K^: dl as a bf16 pair, the key codes in chunks of 32 tokens through LDS (the forward's O = P V with K for V).
  // Wave w owns channels 64 w .. 64 w + 63.
  f32x16 o[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) o[t][g] = 0.f;
  const int nchunk = LP / 32;
  auto stage = [&](int c, int buf) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int idx = tid + 256 * half;            // 512 pieces of 16 bytes
      const int tk = idx >> 4, piece = idx & 15;
      const int l = 32 * c + tk;
      u32x4 val = {0u, 0u, 0u, 0u};
      if (l < a.L) val = *reinterpret_cast<const u32x4*>(a.k + ((size_t)u * a.L + l) * AC + 16 * piece);
      *reinterpret_cast<u32x4*>(&K8[buf][tk][16 * piece]) = val;
    }
  };
  stage(0, 0);
  __syncthreads();
  for (int c = 0; c < nchunk; ++c) {
    if (c + 1 < nchunk) stage(c + 1, (c + 1) & 1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int ks = 2 * c + kk;
      float x[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) x[s] = S[r][16 * ks + 8 * h + s];
      bf16x8 dhi, dlo;
      split8(x, dhi, dlo);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ch = 64 * wave + 32 * t + r;
        bf16x8 kb;
#pragma unroll
        for (int s = 0; s < 8; ++s) kb[s] = e4m3_dec_bf(K8[c & 1][16 * kk + 8 * h + s][ch]);
        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dhi, kb, o[t], 0, 0, 0);
        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dlo, kb, o[t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const float f = sk * a.scale;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int m = (g & 3) + 8 * (g >> 2) + 4 * h;
      const int gr = rows[m];
      if (gr >= 0) a.dq[(size_t)gr * AC + 64 * wave + 32 * t + r] = o[t][g] * f;
    }
}

constexpr int PEND = 512;        // ring of row indices waiting for their chunk: < 32 left over + 256 found per scan step

__global__ __launch_bounds__(256) void attn_fp8_mfma_bwd_sets_kernel(F8bArgs a) {
  __shared__ __attribute__((aligned(16))) float Dl[32][36];                // [row of the chunk][token of the block]
  __shared__ __attribute__((aligned(16))) float Pw[32][36];
  __shared__ __attribute__((aligned(16))) uint8_t Q8[32][AC + 16];
  __shared__ __attribute__((aligned(16))) float Do[32][AC + 4];
  __shared__ int pend[PEND];
  __shared__ int wtot[4];
  const int u = blockIdx.x, l0 = blockIdx.y * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) { dk[t][g] = 0.f; dv[t][g] = 0.f; }

  // one chunk of n <= 32 rows, pend[head ..): M = the block's 32 tokens, N = channels, K = the chunk's rows
  auto process = [&](int head, int n) {
    {   // dl and p: thread = (row tid / 8, 4 tokens)
      const int i = tid >> 3, j = (tid & 7) * 4;
      const int b = i < n ? pend[(head + i) & (PEND - 1)] : -1;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int l = l0 + j + jj;
        const bool ok = b >= 0 && l < a.L;
        Dl[i][j + jj] = ok ? a.dl[(size_t)b * a.L + l] : 0.f;
        Pw[i][j + jj] = ok ? a.attn[(size_t)b * a.L + l] : 0.f;
      }
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {       // query codes: 512 pieces of 16 bytes
      const int idx = tid + 256 * half;
      const int i = idx >> 4, piece = idx & 15;
      u32x4 val = {0u, 0u, 0u, 0u};
      if (i < n) val = *reinterpret_cast<const u32x4*>(a.q + (size_t)pend[(head + i) & (PEND - 1)] * AC + 16 * piece);
      *reinterpret_cast<u32x4*>(&Q8[i][16 * piece]) = val;
    }
#pragma unroll
    for (int it = 0; it < 8; ++it) {             // dout: 2048 pieces of 4 floats
      const int idx = tid + 256 * it;
      const int i = idx >> 6, c4 = idx & 63;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (i < n && a.dout) val = *reinterpret_cast<const f32x4*>(a.dout + (size_t)pend[(head + i) & (PEND - 1)] * AC + 4 * c4);
      *reinterpret_cast<f32x4*>(&Do[i][4 * c4]) = val;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (16 * kk >= n) break;                   // (uniform) the second half of a short chunk holds zeros only
      float x[8];
      bf16x8 dhi, dlo, phi, plo;
#pragma unroll
      for (int s = 0; s < 8; ++s) x[s] = Dl[16 * kk + 8 * h + s][r];
      split8(x, dhi, dlo);
#pragma unroll
      for (int s = 0; s < 8; ++s) x[s] = Pw[16 * kk + 8 * h + s][r];
      split8(x, phi, plo);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int ch = 64 * wave + 32 * t + r;
        bf16x8 qb, ghi, glo;
#pragma unroll
        for (int s = 0; s < 8; ++s) qb[s] = e4m3_dec_bf(Q8[16 * kk + 8 * h + s][ch]);
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dhi, qb, dk[t], 0, 0, 0);
        dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dlo, qb, dk[t], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 8; ++s) x[s] = Do[16 * kk + 8 * h + s][ch];
        split8(x, ghi, glo);
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(phi, ghi, dv[t], 0, 0, 0);
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(phi, glo, dv[t], 0, 0, 0);
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(plo, ghi, dv[t], 0, 0, 0);
        dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(plo, glo, dv[t], 0, 0, 0);
      }
    }
    __syncthreads();
  };

  // the set's rows in ascending row index: ranked scan of `inverse`, 256 rows per step (an index outside [0, U) is clamped as the
  // grouping of wsmg_attn_fp8_prep clamps it)
  int head = 0, tail = 0;
  for (int base = 0; base < a.B; base += 256) {
    const int b = base + tid;
    bool mine = false;
    if (b < a.B) {
      const int64_t su = a.inverse[b];
      mine = (int)(su < 0 ? 0 : su >= a.U ? a.U - 1 : su) == u;
    }
    const unsigned long long bal = __ballot(mine);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int off = tail;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (mine) pend[(off + before) & (PEND - 1)] = b;
    tail += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
    while (tail - head >= 32) {
      process(head, 32);
      head += 32;
    }
  }
  if (tail > head) process(head, tail - head);

  const float fk = *a.q_scale * a.scale;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int l = l0 + (g & 3) + 8 * (g >> 2) + 4 * h;
      if (l < a.L) {
        const size_t at = ((size_t)u * a.L + l) * AC + 64 * wave + 32 * t + r;
        a.dk[at] = dk[t][g] * fk;
        a.dv[at] = dv[t][g];
      }
    }
}

}  // namespace

extern "C" int wsmg_attn_fp8_mfma_bwd(const uint8_t* q_codes, const float* q_scale, const uint8_t* k_codes, const float* k_scale,
                                      const uint8_t* v_codes, const float* v_scale, const int* row_ids, const int* set_start,
                                      const int64_t* inverse, const float* attn, const float* dout, const float* dattn, float scale,
                                      int B, int U, int L, int C, float* dq, float* dk, float* dv, float* dl_scratch,
                                      wsmg_stream_t stream) {
  // every argument is checked before the first launch
  if (!q_codes || !q_scale || !k_codes || !k_scale || !v_codes || !v_scale || !row_ids || !set_start || !inverse || !attn)
    return WSMG_EINVAL;
  if (!dq || !dk || !dv || !dl_scratch) return WSMG_EINVAL;
  if (B <= 0 || U <= 0 || U > 1024 || L <= 0 || L > F8_MAX_L || C != AC) return WSMG_EINVAL;
  F8bArgs a{q_codes, k_codes, v_codes, q_scale, k_scale, v_scale, row_ids, set_start, inverse, attn, dout, dattn, scale, B, U, L,
            dq, dk, dv, dl_scratch};
  hipLaunchKernelGGL(attn_fp8_mfma_bwd_rows_kernel, dim3((unsigned)U, (unsigned)wsmg_cdiv(B, 32)), dim3(256), 0, wsmg_s(stream), a);
  hipLaunchKernelGGL(attn_fp8_mfma_bwd_sets_kernel, dim3((unsigned)U, (unsigned)wsmg_cdiv(L, 32)), dim3(256), 0, wsmg_s(stream), a);
  WSMG_RETURN_LAUNCH();
}
