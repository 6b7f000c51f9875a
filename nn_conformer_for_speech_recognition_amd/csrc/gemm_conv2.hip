// gemm_conv2.hip -- the second subsampling convolution (3x3, stride 2) as implicit GEMMs, no im2col in HBM: the
// gathered-A forms of the LDS-DMA pipeline (kConv2Fwd, kConv2Dgrad) and the register-staged kernels with the conv2
// gather loaders (instantiated here).
#include "gemm_launch.h"
#include "gemm_staged.h"
#include "gemm_variants.h"

// ---------------------------------------------------------------------------- conv2 (3x3, s2)
static Conv2Geo conv2_geo(int B, int F1, int T1, int C1, int C2) {
  Conv2Geo g{B, F1, T1, C1, (F1 - 3) / 2 + 1, (T1 - 3) / 2 + 1, C2};
  return g;
}

CFM_EXPORT int cfm_conv2_fwd(const void* h1, const void* w2r, const float* b2, void* h2, int dtype_h2, int dtype,
                             int B, int F1, int T1, int C1, int C2, void* stream) {
  CFM_REQUIRE(h1 && w2r && h2, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(C1 % 8 == 0 && F1 >= 3 && T1 >= 3 && B > 0 && C2 > 0, CFM_ERR_SHAPE, "conv2: C1 % 8, F1/T1 >= 3");
  CFM_REQUIRE((uintptr_t)h1 % 16 == 0 && (uintptr_t)w2r % 16 == 0, CFM_ERR_ALIGN, "16-B aligned operands");
  const Conv2Geo g = conv2_geo(B, F1, T1, C1, C2);
  GemmP p = plain_params(B * g.T2 * g.F2, C2, 9 * C1, h2, C2, dtype_h2);
  p.bias = b2;
  hipStream_t s = cfm::as_stream(stream);
  const long h1_bytes = (long)B * F1 * T1 * C1 * 2;
  if (dtype == CFM_BF16 && (cfm::g_gemm_mode & CFM_GEMM_MODE_PIPE) && C1 % 64 == 0 && h1_bytes < (1L << 31) - 4096 &&
      cdiv(p.M, 256) <= 65535) {
    // LDS-DMA pipeline with h1 rows gathered per tap: rows m = (b, t2, f2), tap (kh, kw) reads h1 row
    // (b F1 + 2 f2 + kh) T1 + 2 t2 + kw -- every tap in range (no padding)
    GatherA ga{};
    ga.Jn = g.F2; ga.In = g.T2;
    ga.sB = (long)F1 * T1; ga.sI = 2; ga.sJ = 2 * T1; ga.Cr = C1; ga.Ck = C1;
    ga.Ilim = 0x7FFFFFFF; ga.Jlim = 0x7FFFFFFF;
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw) ga.dR[kh * 3 + kw] = kh * T1 + kw;
    p.split_k = 1;
    p.k_per_split = 9 * C1;
    p.vec_c = vec_epilogue_ok(p);
    const PipeOp oa{(const bf16*)h1, C1, 0, p.M, (unsigned)h1_bytes};
    const PipeOp ob{(const bf16*)w2r, 9L * C1, 0, C2, (unsigned)((long)C2 * 9 * C1 * 2)};
    hipLaunchKernelGGL((kConv2Fwd<>), dim3(cdiv(C2, BN), cdiv(p.M, 256), 1),
                       dim3(512), 0, s, p, oa, ob, ga);
    return cfm::check_launch("cfm_conv2_fwd");
  }
  int rc;
  if (dtype == CFM_BF16)
    rc = launch_typed<true, true>(p, Conv2FwdA<bf16>{(const bf16*)h1, g},
                                  StridedOp<bf16>{(const bf16*)w2r, 9L * C1, 0, true}, 1, s);
  else
    rc = launch_typed<true, true>(p, Conv2FwdA<float>{(const float*)h1, g},
                                  StridedOp<float>{(const float*)w2r, 9L * C1, 0, true}, 1, s);
  if (rc != CFM_OK) return rc;
  return cfm::check_launch("cfm_conv2_fwd");
}

// conv2 weight gradient dW2r (C2 x 9*C1, fp32) = dh2^T im2col(h1) over M = B*T2*F2 tokens.  Split-K over the
// tokens into DETERMINISTIC slabs (ws: split x C2 x 9*C1 floats, each slab written whole by its K slice) summed in
// slice order by splitk_reduce_kernel -- no atomics and no memset: the round-2 form zeroed dW with
// hipMemsetAsync and accumulated with atomics, and inside a replayed HIP graph that left part of dW unzeroed /
// stale (the round-2 NaN losses: nan_hunt showed this gradient alone going non-finite under poisoned memory).
static int conv2_wgrad_split(int B, int F1, int T1, int C1, int C2) {
  const Conv2Geo g = conv2_geo(B, F1, T1, C1, C2);
  const int Mrows = B * g.T2 * g.F2;
  const int tiles = cdiv(C2, BM) * cdiv(9 * C1, BN);
  // ~1024 workgroups (4 per CU: the register-staged 128 x 128 kernel needs them to hide its loads; 512 measured
  // 609 vs 485 us for the atomics form at L15), each slice >= 512 tokens
  int split = 1024 / (tiles > 0 ? tiles : 1);
  split = split < 1 ? 1 : (split > 32 ? 32 : split);
  if (Mrows / 512 < split) split = Mrows / 512 > 1 ? Mrows / 512 : 1;
  return split;
}

CFM_EXPORT size_t cfm_conv2_bwd_weight_ws_bytes(int B, int F1, int T1, int C1, int C2) {
  const int split = conv2_wgrad_split(B, F1, T1, C1, C2);
  return split > 1 ? (size_t)split * C2 * 9 * C1 * sizeof(float) : 0;
}

CFM_EXPORT int cfm_conv2_bwd_weight_ws(const void* dh2, const void* h1, float* dw2r, int dtype, int B, int F1, int T1,
                                       int C1, int C2, float* ws, void* stream) {
  CFM_REQUIRE(dh2 && h1 && dw2r, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(C1 % 8 == 0 && C2 % 8 == 0, CFM_ERR_SHAPE, "conv2: C1 and C2 must be multiples of 8");
  const Conv2Geo g = conv2_geo(B, F1, T1, C1, C2);
  const int Mrows = B * g.T2 * g.F2;
  GemmP p = plain_params(C2, 9 * C1, Mrows, dw2r, 9L * C1, CFM_F32);
  const int split = ws ? conv2_wgrad_split(B, F1, T1, C1, C2) : 1;
  p.split_k = split;
  p.k_per_split = split_k_for(p, dtype == CFM_BF16 ? BK16 : BK32);
  const int used = cdiv(Mrows, p.k_per_split);       // slices that hold tokens (each writes its whole slab)
  p.split_k = used;
  if (used > 1) {
    CFM_REQUIRE((long)C2 * 9 * C1 < (1L << 31), CFM_ERR_SHAPE, "conv2 wgrad: slab too large");
    p.slab = ws;
  }
  hipStream_t s = cfm::as_stream(stream);
  int rc;
  if (dtype == CFM_BF16)
    rc = launch_typed<false, false>(p, StridedOp<bf16>{(const bf16*)dh2, C2, 0, C2 % 8 == 0},
                                    Conv2WgradB<bf16>{(const bf16*)h1, g}, 1, s);
  else
    rc = launch_typed<false, false>(p, StridedOp<float>{(const float*)dh2, C2, 0, C2 % 4 == 0},
                                    Conv2WgradB<float>{(const float*)h1, g}, 1, s);
  if (rc != CFM_OK) return rc;
  if (used > 1) {
    const long n4 = (long)C2 * 9 * C1 / 4;
    cfm::gemm_splitk_reduce((unsigned)((n4 + 255) / 256), 1, p.slab, used, C2, 9 * C1, dw2r, 9L * C1, 0L, nullptr, nullptr,
                            nullptr, s);
  }
  return cfm::check_launch("cfm_conv2_bwd_weight");
}

// (workspace-free form: one K slice, no split -- kept for the C ABI; the host path passes a workspace)
CFM_EXPORT int cfm_conv2_bwd_weight(const void* dh2, const void* h1, float* dw2r, int dtype, int B, int F1, int T1,
                                    int C1, int C2, void* stream) {
  return cfm_conv2_bwd_weight_ws(dh2, h1, dw2r, dtype, B, F1, T1, C1, C2, nullptr, stream);
}

namespace {
// Per-class K-major data-gradient weights: wt[koff(class) + c1 * K_class + ti * C2 + c2] =
// w2r[c2][kh_ti][kw_ti][c1] for the class's taps (classes (pf, pt) in order (0,0) (0,1) (1,0) (1,1):
// 4, 2, 2, 1 taps -> 9 * C1 * C2 elements in all)
__global__ __launch_bounds__(256) void conv2_dgrad_pack(const bf16* __restrict__ w2r, bf16* __restrict__ wt, int C1,
                                                        int C2) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)C1 * C2;
  if (e >= 9 * per) return;
  // which class / tap of the class does slab e / per belong to
  const int slab = (int)(e / per);        // 0..8: class (0,0) taps 0-3, (0,1) 4-5, (1,0) 6-7, (1,1) 8
  const int cls = slab < 4 ? 0 : (slab < 6 ? 1 : (slab < 8 ? 2 : 3));
  const int first = cls == 0 ? 0 : (cls == 1 ? 4 : (cls == 2 ? 6 : 8));
  const int ntaps = cls == 0 ? 4 : (cls == 3 ? 1 : 2);
  const int pf = cls >> 1, pt = cls & 1;
  const long r = e - (long)first * per;   // offset inside the class block (C1 x ntaps*C2)
  const int K = ntaps * C2;
  const int c1 = (int)(r / K), k = (int)(r % K), ti = k / C2, c2 = k % C2;
  // taps of the class in (kh, kw) order, kh = pf (+2), kw = pt (+2)
  const int nkw = pt == 0 ? 2 : 1;
  const int kh = pf + 2 * (ti / nkw), kw = pt + 2 * (ti % nkw);
  wt[e] = w2r[((long)c2 * 9 + kh * 3 + kw) * C1 + c1];
}
}  // namespace

CFM_EXPORT int cfm_conv2_bwd_data(const void* dh2, const void* w2r, void* dh1, int dtype, int B, int F1, int T1,
                                  int C1, int C2, void* stream);

CFM_EXPORT size_t cfm_conv2_bwd_data_ws_bytes(int C1, int C2) { return (size_t)9 * C1 * C2 * sizeof(bf16); }

// conv2 data-gradient on the LDS-DMA pipeline (bf16): per parity class, A rows gathered straight from
// dh2 by the DMA (GatherA), B = the class's packed K-major weights (from `ws`, written by
// conv2_dgrad_pack on the same stream), output rows scattered to the class's dh1 pixels (cmap).
// Falls back to the register-staged gather kernel when ws is NULL or the shape does not qualify.
CFM_EXPORT int cfm_conv2_bwd_data_ws(const void* dh2, const void* w2r, void* dh1, int dtype, int B, int F1, int T1,
                                     int C1, int C2, void* ws, void* stream) {
  CFM_REQUIRE(dh2 && w2r && dh1, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(C1 % 8 == 0 && C2 % 8 == 0, CFM_ERR_SHAPE, "conv2: C1 and C2 must be multiples of 8");
  const Conv2Geo g = conv2_geo(B, F1, T1, C1, C2);
  const long dh2_bytes = (long)B * g.T2 * g.F2 * C2 * 2;
  const bool fast = ws && dtype == CFM_BF16 && C2 % 32 == 0 && C1 % 8 == 0 && (cfm::g_gemm_mode & CFM_GEMM_MODE_PIPE) &&
                    dh2_bytes < (1L << 31) - 4096 && ((uintptr_t)dh2 % 16) == 0 && ((uintptr_t)dh1 % 16) == 0;
  if (!fast) return cfm_conv2_bwd_data(dh2, w2r, dh1, dtype, B, F1, T1, C1, C2, stream);
  hipStream_t s = cfm::as_stream(stream);
  bf16* wt = (bf16*)ws;
  const long per = (long)C1 * C2;
  hipLaunchKernelGGL(conv2_dgrad_pack, dim3((unsigned)cdiv(9 * per, 256)), dim3(256), 0, s, (const bf16*)w2r, wt, C1,
                     C2);
  long koff = 0;
  for (int pf = 0; pf < 2; ++pf)
    for (int pt = 0; pt < 2; ++pt) {
      GatherA ga{};
      const int F1c = (F1 - pf + 1) / 2, T1c = (T1 - pt + 1) / 2;
      // rows (b, i, j) of the class; source dh2 rows (b, t2, f2) = b T2 F2 + t2 F2 + f2 with f2 = i - di, t2 = j - dj
      ga.Jn = T1c; ga.In = F1c;
      ga.sB = (long)g.T2 * g.F2; ga.sI = 1; ga.sJ = g.F2; ga.Cr = C2; ga.Ck = C2; ga.Ilim = g.F2; ga.Jlim = g.T2;
      int nt = 0;
      for (int kh = pf; kh < 3; kh += 2)
        for (int kw = pt; kw < 3; kw += 2) {
          ga.di[nt] = (kh - pf) / 2;
          ga.dj[nt] = (kw - pt) / 2;
          ga.dR[nt] = -(ga.dj[nt] * g.F2 + ga.di[nt]);
          ++nt;
        }
      const int K = nt * C2;
      const bf16* wc = wt + koff;
      koff += (long)nt * per;
      if (F1c <= 0 || T1c <= 0) continue;
      GemmP p = plain_params(B * F1c * T1c, C1, K, dh1, C1, dtype);
      p.cmap = 1; p.cm_F1c = F1c; p.cm_T1c = T1c; p.cm_pf = pf; p.cm_pt = pt; p.cm_F1 = F1; p.cm_T1 = T1;
      p.split_k = 1;
      p.k_per_split = K;
      p.vec_c = vec_epilogue_ok(p);
      const PipeOp oa{(const bf16*)dh2, C2, 0, p.M, (unsigned)dh2_bytes};
      const PipeOp ob{wc, K, 0, C1, (unsigned)(per * nt * 2)};
      const dim3 grid(cdiv(C1, BN), cdiv(p.M, 256), 1);
      CFM_REQUIRE(grid.y <= 65535, CFM_ERR_SHAPE, "conv2 dgrad: grid too large");
      hipLaunchKernelGGL((kConv2Dgrad<>), grid, dim3(512), 0, s, p, oa, ob,
                         ga);
    }
  return cfm::check_launch("cfm_conv2_bwd_data_ws");
}

CFM_EXPORT int cfm_conv2_bwd_data(const void* dh2, const void* w2r, void* dh1, int dtype, int B, int F1, int T1,
                                  int C1, int C2, void* stream) {
  CFM_REQUIRE(dh2 && w2r && dh1, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(C1 % 8 == 0 && C2 % 8 == 0, CFM_ERR_SHAPE, "conv2: C1 and C2 must be multiples of 8");
  const Conv2Geo g = conv2_geo(B, F1, T1, C1, C2);
  hipStream_t s = cfm::as_stream(stream);
  for (int pf = 0; pf < 2; ++pf)
    for (int pt = 0; pt < 2; ++pt) {
      Conv2Class c{};
      c.pf = pf; c.pt = pt;
      c.F1c = (F1 - pf + 1) / 2;
      c.T1c = (T1 - pt + 1) / 2;
      for (int kh = pf; kh < 3; kh += 2)
        for (int kw = pt; kw < 3; kw += 2) {
          c.kh[c.ntaps] = kh;
          c.kw[c.ntaps] = kw;
          ++c.ntaps;
        }
      if (c.F1c <= 0 || c.T1c <= 0) continue;
      GemmP p = plain_params(B * c.F1c * c.T1c, C1, c.ntaps * C2, dh1, C1, dtype);
      p.cmap = 1; p.cm_F1c = c.F1c; p.cm_T1c = c.T1c; p.cm_pf = pf; p.cm_pt = pt; p.cm_F1 = F1; p.cm_T1 = T1;
      int rc;
      if (dtype == CFM_BF16)
        rc = launch_typed<true, false>(p, Conv2DgradA<bf16>{(const bf16*)dh2, g, c},
                                       Conv2DgradB<bf16>{(const bf16*)w2r, g, c}, 1, s);
      else
        rc = launch_typed<true, false>(p, Conv2DgradA<float>{(const float*)dh2, g, c},
                                       Conv2DgradB<float>{(const float*)w2r, g, c}, 1, s);
      if (rc != CFM_OK) return rc;
    }
  return cfm::check_launch("cfm_conv2_bwd_data");
}
