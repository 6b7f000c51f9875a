// gemm_epilogue.h -- the fused epilogues: the per-element and 8-column generic forms (epilogue_store,
// epilogue_store8), the compile-time fast kinds (EF_*, epi_rows_fast) and the staged tile epilogue of the
// LDS-DMA, warp-specialised and fp32 kernels (tile_epilogue_g).
#pragma once
#include "gemm_params.h"

namespace {

// zs: the launch's batch x split-K slice index (selects the split-K slab)
__device__ __forceinline__ void epilogue_store(const GemmP& p, int z, int zs, int m, int n, float acc) {
  if (m >= p.M || n >= p.N) return;
  const long cidx = (long)z * p.sc + out_row(p, m) * p.ldc + n;
  float v = acc * p.alpha;
  if (p.split_k > 1) {
    if (p.slab) {
      p.slab[(long)zs * p.M * p.N + (long)m * p.N + n] = v;
      return;
    }
    if (p.bias && zs % p.split_k == 0) v += p.bias[n];
    atomicAdd(reinterpret_cast<float*>(p.C) + cidx, v);
    return;
  }
  if (p.bias) v += p.bias[n];
  if (p.act_grad) v *= silu_grad_f(ld_dyn(p.pre, p.dtpre, cidx));
  if (p.act == CFM_ACT_SILU) {
    if (p.pre) st_dyn(p.pre, p.dtpre, cidx, v);
    v = silu_f(v);
  }
  if (p.drop_p > 0.f) v *= dropout_scale(p.drop_p, p.seed, p.doff + (uint64_t)((long)z * p.M * p.N + (long)m * p.N + n));
  v *= p.out_scale;
  if (p.res) v += ld_dyn(p.res, p.dtr, (long)z * p.sc + (long)m * p.ldr + n);
  st_dyn(p.C, p.dtc, cidx, v);
}

// split-K partial of one element: the whole epilogue a split-K launch may carry (cfm_gemm requires a plain fp32
// epilogue for split_k > 1): alpha, the bias on the first slice, atomic accumulation -- a small body, so the
// 64-element loops over an accumulator tile unroll fully (epilogue_store's general body did not)
__device__ __forceinline__ void splitk_atomic_store(const GemmP& p, int z, int zs, int m, int n, float acc) {
  if (m >= p.M || n >= p.N) return;
  float v = acc * p.alpha;
  if (p.bias && zs % p.split_k == 0) v += p.bias[n];
  atomicAdd(reinterpret_cast<float*>(p.C) + (long)z * p.sc + out_row(p, m) * p.ldc + n, v);
}

constexpr int EP_STRIDE = 128 + 4;   // f32 staging row stride: rows r and r+4 land 16 banks apart
static_assert(128 * EP_STRIDE * 4 <= 4 * TILE16 * 2, "epilogue staging fits in the K-loop LDS");

// the epilogue of cfm_gemm_desc on 8 consecutive columns (vectorised when legal)
__device__ __forceinline__ void epilogue_store8(const GemmP& p, int z, int zs, int m, int n, float (&v)[8]) {
  if (m >= p.M || n >= p.N) return;
  if (p.split_k > 1 && p.slab && n + 8 <= p.N && (p.N & 3) == 0) {
    float* dst = p.slab + (long)zs * p.M * p.N + (long)m * p.N + n;
    *reinterpret_cast<float4*>(dst) = make_float4(v[0] * p.alpha, v[1] * p.alpha, v[2] * p.alpha, v[3] * p.alpha);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4] * p.alpha, v[5] * p.alpha, v[6] * p.alpha, v[7] * p.alpha);
    return;
  }
  if (!p.vec_c || n + 8 > p.N || p.split_k > 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (n + e < p.N) epilogue_store(p, z, zs, m, n + e, v[e]);
    return;
  }
  const long cidx = (long)z * p.sc + out_row(p, m) * p.ldc + n;
  if (p.alpha != 1.f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= p.alpha;
  }
  if (p.bias) {
    const float4 a = *reinterpret_cast<const float4*>(p.bias + n);
    const float4 c = *reinterpret_cast<const float4*>(p.bias + n + 4);
    v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += c.x; v[5] += c.y; v[6] += c.z; v[7] += c.w;
  }
  if (p.act_grad) {
    float pr[8];
    ld8_dyn(p.pre, p.dtpre, cidx, pr);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= silu_grad_f(pr[e]);
  }
  if (p.act == CFM_ACT_SILU) {
    if (p.pre) st8_dyn(p.pre, p.dtpre, cidx, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
  }
  if (p.drop_p > 0.f) {
    const uint64_t base = p.doff + (uint64_t)((long)z * p.M * p.N + (long)m * p.N + n);
    float ds[8];
    const uint64_t j0 = base >> 1;
    if ((j0 >> 32) == 0 && (uint32_t)j0 <= 0xFFFFFFFBu && !(p.dbg & 2)) {   // (always, below 2^33 elements)
      uint32_t h[5];
      const int odd = (int)(base & 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) h[q] = attn_mix((uint32_t)j0 + q + p.dkey0);
      h[4] = odd ? attn_mix((uint32_t)j0 + 4 + p.dkey0) : 0u;   // (an even base needs 4 pair hashes)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int q = (odd + e) >> 1;
        const uint32_t b = ((odd + e) & 1) ? (h[q] >> 16) : (h[q] & 0xFFFFu);
        ds[e] = b >= p.dthr ? p.dkeep : 0.f;
      }
    } else {
      dropout_scale8(p.drop_p, p.seed, base, ds);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= ds[e];
  }
  if (p.out_scale != 1.f) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] *= p.out_scale;
  }
  if (p.res) {
    float r[8];
    ld8_dyn(p.res, p.dtr, (long)z * p.sc + (long)m * p.ldr + n, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += r[e];
  }
  st8_dyn(p.C, p.dtc, cidx, v);
}

// Epilogue of one tile held as WM x WN waves of FM x FN 32x32 accumulators (wave band = FM*32
// rows).  Rows are staged through LDS in chunks of CHB bands (<= 128 rows), then every thread
// finishes 8 consecutive columns of a row (16-B / 32-B vector stores).  The caller guarantees every
// wave is done reading the staging LDS (`st`, >= 128 x EP_STRIDE floats).
// (row, col) inside a 32x32 accumulator block of register r: the 32x32x16 MFMA layout, or (M16) four 16x16x32
// blocks packed as r = 4 (2a + b) + q -> block (a, b) of the 32x32, register q
template <bool M16> __device__ __forceinline__ int accr(int r, int lane) {
  return M16 ? 16 * ((r >> 3) & 1) + 4 * (lane >> 4) + (r & 3) : (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
template <bool M16> __device__ __forceinline__ int accc(int r, int lane) {
  return M16 ? 16 * ((r >> 2) & 1) + (lane & 15) : (lane & 31);
}

// Staged-epilogue fast path (the encoder's launches; host-side selection in epi_fast_kind): split-K 1, vectorised
// C with N % 8 == 0, bf16 pre-activation, f32 residual, the 32-bit dropout hash range, and a feature set fixed
// at compile time per kind (EK, a kernel template parameter: each kernel carries one epilogue body -- the generic
// body's registers spilled in the 128-register two-per-CU kernels, one accumulator inside the MFMA loop):
//   EF_BF16      bf16 C, nothing else (the d-wide data gradients)
//   EF_BF16_BIAS bf16 C; bias (QKV, pointwise-conv-1 forward)
//   EF_BF16_SILU bf16 C; bias, SiLU + bf16 pre-activation store, dropout (FFN-up forward)
//   EF_BF16_ACTG bf16 C; silu'(pre) * dropout (FFN-down data gradient)
//   EF_BF16_RD   bf16 C; rowdot with rd_with (attention out-projection data gradient)
//   EF_F32       f32 C; alpha, bias, SiLU (+ pre), dropout, out_scale as run-time options
//   EF_F32_RES   f32 C; bias, dropout, out_scale, f32 residual (the d-wide residual-stream outputs)
//   EF_BF16_SILU_MX  EF_BF16_SILU + the MX e4m3 copy of the bf16 C (fp8 FFN-up forward: the FFN-down GEMM's
//                operand; the 4 threads of a 32-column block exchange maxima by two xor shuffles)
// Every option a kind does not list is absent by construction (epi_fast_kind checks): a run-time test on a
// uniform kernel argument is flattened by the compiler into per-lane selects with BOTH sides computed (the SiLU
// of the bias-only QKV rows, the alpha and out_scale products), so the encoder's kinds carry no such tests.
// A thread's 8-column chunk is the same on every row it finishes, so its bias is loaded once, and each row's global
// input (the bf16 pre-activation / rd_with, or the f32 residual) is issued ahead of the previous rows' stores:
// vmcnt counts loads and stores in one in-order queue, and the generic rows, which load bias / pre / residual
// between the previous row's stores, waited for every previous row's write acknowledgements (bias-only FFN-up
// epilogue without the main loop: 49 MB in 21.9 us = 2.2 TB/s).  Arithmetic and its order are epilogue_store8's
// (bit-identical outputs).
// residual-stream kinds: EF_F32_RES (fp32 residual in, fp32 out: the parity mode), EF_BF16_RES (bf16 in, bf16 out: the
// bf16 mode's bf16 residual stream), EF_F32R_BF16 (fp32 in, bf16 out: a layer's first residual add, whose input is the
// previous layer's fp32 LayerNorm output); EF_BF16_DELTA: a residual module's output without the residual (bias,
// dropout, out_scale, bf16) -- the add happens in the next LayerNorm (cfm_layernorm_fwd_res)
enum { EF_GENERIC = 0, EF_BF16 = 1, EF_BF16_BIAS = 2, EF_BF16_SILU = 3, EF_BF16_ACTG = 4, EF_BF16_RD = 5, EF_F32 = 6,
       EF_F32_RES = 7, EF_BF16_SILU_MX = 8, EF_BF16_RES = 9, EF_F32R_BF16 = 10, EF_BF16_DELTA = 11 };
static_assert(EF_GENERIC == CFM_GEMM_EPI_GENERIC && EF_BF16 == CFM_GEMM_EPI_BF16 && EF_BF16_BIAS == CFM_GEMM_EPI_BF16_BIAS &&
                  EF_BF16_SILU == CFM_GEMM_EPI_BF16_SILU && EF_BF16_ACTG == CFM_GEMM_EPI_BF16_ACTG &&
                  EF_BF16_RD == CFM_GEMM_EPI_BF16_RD && EF_F32 == CFM_GEMM_EPI_F32 && EF_F32_RES == CFM_GEMM_EPI_F32_RES &&
                  EF_BF16_SILU_MX == CFM_GEMM_EPI_BF16_SILU_MX && EF_BF16_RES == CFM_GEMM_EPI_BF16_RES &&
                  EF_F32R_BF16 == CFM_GEMM_EPI_F32R_BF16 && EF_BF16_DELTA == CFM_GEMM_EPI_BF16_DELTA,
              "cfm_gemm_epilogue (cfm.h) reports these kinds");

// e8m0 block exponent of an MX block (fp8.hip mx_k): the largest k with amax * 2^k <= 448
__device__ __forceinline__ int epi_mx_k(float a) {
  if (!(a > 0.f) || !(a < INFINITY)) return 0;
  int e;
  const float m = 2.f * frexpf(a, &e);
  const int k = (m <= 1.75f ? 8 : 7) - (e - 1);
  return k < 126 ? (k > -126 ? k : -126) : 126;
}

__device__ __forceinline__ void epi_bias8(const GemmP& p, int n, float (&b)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) b[e] = 0.f;
  if (p.efast && p.bias && n < p.N) {
    const float4 a = *reinterpret_cast<const float4*>(p.bias + n);
    const float4 c = *reinterpret_cast<const float4*>(p.bias + n + 4);
    b[0] = a.x; b[1] = a.y; b[2] = a.z; b[3] = a.w; b[4] = c.x; b[5] = c.y; b[6] = c.z; b[7] = c.w;
  }
}

// dropout of 8 consecutive elements starting at an index of parity ODD whose pair index is j0 (epilogue_store8's
// hash path: element i draws the (i & 1) half of attn_mix(i / 2 + key))
template <bool ODD>
__device__ __forceinline__ void drop8_fast(float (&v)[8], uint32_t j0, const GemmP& p) {
  constexpr int NH = ODD ? 5 : 4;
  uint32_t h[NH];
#pragma unroll
  for (int q = 0; q < NH; ++q) h[q] = attn_mix(j0 + q + p.dkey0);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q = (ODD + e) >> 1;
    const uint32_t bits = ((ODD + e) & 1) ? (h[q] >> 16) : (h[q] & 0xFFFFu);
    v[e] *= bits >= p.dthr ? p.dkeep : 0.f;
  }
}

// per-row global inputs of a fast epilogue kind: dwords per row, and the holder (IT rows of one thread)
template <int EK> constexpr int epi_nw() {
  return (EK == EF_F32_RES || EK == EF_F32R_BF16) ? 8 : (EK == EF_BF16_ACTG || EK == EF_BF16_RD || EK == EF_BF16_RES) ? 4
                                                                                                                     : 0;
}
template <int EK, int IT> struct EpiIn { uint4 v[IT][epi_nw<EK>() == 8 ? 2 : 1]; };

template <int EK, int IT, int NTt, int CPW>
__device__ __forceinline__ void epi_load_row(const GemmP& p, int z, int mbase, int n0, int tid, int it,
                                             EpiIn<EK, IT>& in) {
  const int n = n0 + (tid % CPW) * 8, m = mbase + it * (NTt / CPW) + tid / CPW;
  if (m < p.M && n < p.N) {
    if constexpr (EK == EF_F32_RES || EK == EF_F32R_BF16) {
      const uint4* s = reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(p.res) + (long)z * p.sc +
                                                      (long)m * p.ldr + n);
      in.v[it][0] = s[0];
      in.v[it][1] = s[1];
    } else if constexpr (EK == EF_BF16_RES) {
      in.v[it][0] = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(p.res) + (long)z * p.sc +
                                                    (long)m * p.ldr + n);
    } else if constexpr (EK == EF_BF16_ACTG) {
      in.v[it][0] = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(p.pre) + (long)z * p.sc +
                                                    (long)m * p.ldc + n);
    } else if constexpr (EK == EF_BF16_RD) {
      in.v[it][0] = *reinterpret_cast<const uint4*>(p.rd_with + (long)m * p.ldc + n);
    }
  }
}

// every row's input, issued up front (the warp-specialised kernel: before its main loop, which hides the latency)
template <int EK, int IT, int NTt, int CPW>
__device__ __forceinline__ void epi_load_all(const GemmP& p, int z, int mbase, int n0, int tid, EpiIn<EK, IT>& in) {
  if constexpr (epi_nw<EK>() > 0) {
#pragma unroll
    for (int it = 0; it < IT; ++it) epi_load_row<EK, IT, NTt, CPW>(p, z, mbase, n0, tid, it, in);
  }
}

// PRE: `in` already holds every row's input (epi_load_all); otherwise row it's input is issued PD rows ahead,
// before the stores of row it - PD (two rows ahead: the 128-register two-per-CU kernels)
template <int EK, int IT, int NTt, int CPW, int EPS, bool PRE = false>
__device__ __forceinline__ void epi_rows_fast(const GemmP& p, const float* st, int z, int mbase, int n0, int tid,
                                              const float (&b)[8], EpiIn<EK, IT>& in) {
  static_assert(EK > EF_GENERIC && EK <= EF_BF16_DELTA, "fast epilogue kind");
  constexpr bool CF32 = EK == EF_F32 || EK == EF_F32_RES, ACTG = EK == EF_BF16_ACTG, RD = EK == EF_BF16_RD;
  constexpr bool RESB = EK == EF_BF16_RES;                      // bf16 residual operand
  constexpr bool RES = EK == EF_F32_RES || RESB || EK == EF_F32R_BF16, GEN = EK == EF_F32;   // GEN: EF_F32's options
  constexpr bool MXO = EK == EF_BF16_SILU_MX, DLT = EK == EF_BF16_DELTA;
  constexpr bool SILU = EK == EF_BF16_SILU || MXO, BIAS = EK == EF_BF16_BIAS || SILU || RES || DLT;
  constexpr bool DROP = SILU || ACTG || RES || GEN || DLT;
  constexpr int NW = epi_nw<EK>();
  constexpr int RPI = NTt / CPW;                       // rows per pass
  const int c8 = (tid % CPW) * 8, n = n0 + c8, r0 = tid / CPW;
  const bool nok = n < p.N;
  constexpr int PD = PRE ? IT : (IT < 2 ? IT : 2);
  if constexpr (NW > 0 && !PRE) {
#pragma unroll
    for (int it = 0; it < PD; ++it) epi_load_row<EK, IT, NTt, CPW>(p, z, mbase, n0, tid, it, in);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    if constexpr (NW > 0 && !PRE) {
      if (it + PD < IT) epi_load_row<EK, IT, NTt, CPW>(p, z, mbase, n0, tid, it + PD, in);
    }
    const int row = it * RPI + r0, m = mbase + row;
    const float4 lo = *reinterpret_cast<const float4*>(st + row * EPS + c8);
    const float4 hi = *reinterpret_cast<const float4*>(st + row * EPS + c8 + 4);
    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const bool ok = m < p.M && nok;
    if (ok) {
      const long cidx = (long)z * p.sc + (long)m * p.ldc + n;   // (no row remap: epi_fast_kind)
      if constexpr (GEN) {
        if (p.alpha != 1.f) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= p.alpha;
        }
        if (p.bias) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += b[e];
        }
      }
      if constexpr (BIAS) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += b[e];
      }
      if constexpr (ACTG) {
        const bf16x8 pr = __builtin_bit_cast(bf16x8, in.v[it][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= silu_grad_f((float)pr[e]);
      }
      if constexpr (SILU || GEN) {
        if (SILU || p.act == CFM_ACT_SILU) {
          if (SILU || p.pre) {
            bf16x8 q;
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = (bf16)v[e];
            *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(p.pre) + cidx) = __builtin_bit_cast(uint4, q);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = silu_f(v[e]);
        }
      }
      if constexpr (DROP) {
        if (p.drop_p > 0.f) {
          // n and N are multiples of 8: the element index's parity is the offset's (uniform), so the hash-half
          // selection is static in each branch (a per-lane parity cost ~48 selects per row)
          const uint32_t j0 = (uint32_t)((p.doff + (uint64_t)(((long)z * p.M + m) * p.N + n)) >> 1);
          if (p.doff & 1) drop8_fast<true>(v, j0, p);
          else drop8_fast<false>(v, j0, p);
        }
      }
      if constexpr (RES || DLT) {   // (unconditional: x * 1.0f == x, and no per-lane select for the 1.0 launches)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= p.out_scale;
      } else if constexpr (GEN) {
        if (p.out_scale != 1.f) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] *= p.out_scale;
        }
      }
      if constexpr (RESB) {
        const bf16x8 r = __builtin_bit_cast(bf16x8, in.v[it][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)r[e];
      } else if constexpr (RES) {
        const float4 ra = __builtin_bit_cast(float4, in.v[it][0]), rb = __builtin_bit_cast(float4, in.v[it][1]);
        v[0] += ra.x; v[1] += ra.y; v[2] += ra.z; v[3] += ra.w; v[4] += rb.x; v[5] += rb.y; v[6] += rb.z; v[7] += rb.w;
      }
      if constexpr (CF32) {
        float* d = reinterpret_cast<float*>(p.C) + cidx;
        *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
      } else {
        bf16x8 q;
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (bf16)v[e];
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(p.C) + cidx) = __builtin_bit_cast(uint4, q);
        if constexpr (MXO) {   // (N % 32 == 0: a block's 4 threads share the row, so all four are here)
          float mx = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf((float)q[e]));
          mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
          mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
          const int k = epi_mx_k(mx);
          const float sc = ldexpf(1.f, k);
          int lo = 0, hi = 0;
          lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)q[0] * sc, (float)q[1] * sc, lo, false);
          lo = __builtin_amdgcn_cvt_pk_fp8_f32((float)q[2] * sc, (float)q[3] * sc, lo, true);
          hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)q[4] * sc, (float)q[5] * sc, hi, false);
          hi = __builtin_amdgcn_cvt_pk_fp8_f32((float)q[6] * sc, (float)q[7] * sc, hi, true);
          *reinterpret_cast<uint2*>(p.mxo8 + (long)m * p.N + n) = make_uint2((unsigned)lo, (unsigned)hi);
          if ((tid & 3) == 0) p.mxos[(long)m * (p.N / 32) + n / 32] = (uint8_t)(127 - k);
        }
      }
    }
    if constexpr (RD) {   // 8-lane group = 64 columns (as tile_epilogue_g's generic rows)
      float t = 0.f;
      if (ok) {
        const bf16x8 w = __builtin_bit_cast(bf16x8, in.v[it][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) t += (float)(bf16)v[e] * (float)w[e];
      }
      t += __shfl_xor(t, 1, 64);
      t += __shfl_xor(t, 2, 64);
      t += __shfl_xor(t, 4, 64);
      if ((tid & 7) == 0 && ok) {
        const int bb = m / p.rd_T, tt = m - bb * p.rd_T, g = n >> 6;
        p.rd_out[((long)bb * (p.N >> 6) + g) * p.rd_T + tt] = t;
      }
    }
  }
}

template <int FM, int FN, int WM, int WN, int NTt, int BNt = BN, bool M16 = false, int ROWS = 128, int EK = EF_GENERIC>
__device__ __forceinline__ void tile_epilogue_g(const GemmP& p, f32x16 (&acc)[FM][FN], float* st, int z, int zs,
                                                int m0, int n0, int wm, int wn, int lane, int tid) {
  // ROWS: the staging rows `st` holds (ROWS x (BNt + 4) floats)
  constexpr int BAND = FM * 32, CHB = (ROWS / BAND) >= 1 && WM % (ROWS / BAND) == 0 ? ROWS / BAND : 1;
  static_assert(BAND <= ROWS, "one wave band fits the staging");
  constexpr int RC = CHB * BAND;
  constexpr int EPS = BNt + 4;         // staging row stride (floats): = 4 mod 32 for both widths
  constexpr int CPW = BNt / 8;         // 8-column chunks per row
  static_assert(WN * FN * 32 == BNt, "tile width");
  if (EK == EF_GENERIC && p.split_k > 1 && !p.slab) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * BAND + i * 32 + accr<M16>(r, lane);
          const int n = n0 + wn * FN * 32 + j * 32 + accc<M16>(r, lane);
          splitk_atomic_store(p, z, zs, m, n, acc[i][j][r]);
        }
    return;
  }
  float bias8[8];
  if constexpr (EK != EF_GENERIC) epi_bias8(p, n0 + (tid % CPW) * 8, bias8);
  // (one pass per band chunk; not unrolled -- the epilogue body is large and nothing in it is indexed by hf)
#pragma nounroll
  for (int hf = 0; hf < WM / CHB; ++hf) {
    // fast kinds with a per-row global input (pre-activation, residual, rowdot operand): every row of this pass is
    // issued here, before the accumulators are staged -- the loads' latency hides under the staging and its barrier
    // (issued two rows ahead of the stores instead, the FFN-down data gradient's pre-activation reads exposed ~4
    // round trips per pass)
    EpiIn<EK == EF_GENERIC ? EF_BF16 : EK, RC * CPW / NTt> ein;
    if constexpr (EK != EF_GENERIC) epi_load_all<EK, RC * CPW / NTt, NTt, CPW>(p, z, m0 + RC * hf, n0, tid, ein);
    if (wm / CHB == hf) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (wm % CHB) * BAND + i * 32 + accr<M16>(r, lane);
            const int col = wn * FN * 32 + j * 32 + accc<M16>(r, lane);
            st[row * EPS + col] = acc[i][j][r];
          }
    }
    __syncthreads();
    static_assert((RC * CPW) % NTt == 0 && NTt % CPW == 0, "whole rows per pass");
    if constexpr (EK != EF_GENERIC) {
      epi_rows_fast<EK, RC * CPW / NTt, NTt, CPW, EPS, true>(p, st, z, m0 + RC * hf, n0, tid, bias8, ein);
      if (hf + 1 < WM / CHB) __syncthreads();
      continue;
    }
#pragma unroll 2
    for (int it = 0; it < RC * CPW / NTt; ++it) {
      const int row = it * (NTt / CPW) + tid / CPW, c8 = (tid % CPW) * 8;
      const float4 lo = *reinterpret_cast<const float4*>(st + row * EPS + c8);
      const float4 hi = *reinterpret_cast<const float4*>(st + row * EPS + c8 + 4);
      float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      const int m = m0 + RC * hf + row;
      epilogue_store8(p, z, zs, m, n0 + c8, v);
      if (p.rd_out) {   // (vectorised bf16 epilogue: v now holds the stored values) 8-lane group = 64 columns
        float t = 0.f;
        if (m < p.M && n0 + c8 < p.N) {
          const uint4 u = *reinterpret_cast<const uint4*>(p.rd_with + (long)m * p.ldc + n0 + c8);
          const bf16x8 w = __builtin_bit_cast(bf16x8, u);
#pragma unroll
          for (int e = 0; e < 8; ++e) t += (float)(bf16)v[e] * (float)w[e];
        }
        t += __shfl_xor(t, 1, 64);
        t += __shfl_xor(t, 2, 64);
        t += __shfl_xor(t, 4, 64);
        if ((tid & 7) == 0 && m < p.M && n0 + c8 < p.N) {
          const int b = m / p.rd_T, tt = m - b * p.rd_T, g = (n0 + c8) >> 6;
          p.rd_out[((long)b * (p.N >> 6) + g) * p.rd_T + tt] = t;
        }
      }
    }
    if (hf + 1 < WM / CHB) __syncthreads();
  }
}

}  // namespace
