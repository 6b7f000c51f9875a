// gemm.hip -- cfm_gemm: validation, kernel selection and dispatch.  The kernels live in the gemm_*.h headers and
// are instantiated by gemm_staged.hip / gemm_pipe.hip / gemm_ws.hip / gemm_fp8.hip ("GEMM source map");
// this object holds the rules.  gemm_prepare is the one routine behind both cfm_gemm and cfm_gemm_plan: it validates
// the descriptor, builds the kernel parameter block and selects the kernel, so a plan can never disagree with a launch.
#include "gemm_launch.h"
#include "gemm_staged.h"

namespace cfm {
int g_gemm_mode = CFM_GEMM_MODE_DEFAULT;
}

namespace {

// C[z][m][n] = sum_s slab[z*split + s][m][n] + bias[n]   (fp32 C, 4 columns per thread)
// grid (ceil(M*N/4 / 256), batch): 32-bit index math (M*N < 2^31), the split slabs summed in order
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, int split, int M, int N,
                                                            float* __restrict__ C, long ldc, long sc,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ acs_slab, float* __restrict__ acs) {
  if (acs_slab && blockIdx.y == 0) {   // A column sums: out[m] = sum_s acs_slab[s][m] (in order)
    const unsigned m = blockIdx.x * 256u + threadIdx.x;
    if (m < (unsigned)M) {
      float t = acs_slab[m];
      for (int k = 1; k < split; ++k) t += acs_slab[(long)k * M + m];
      acs[m] = t;
    }
  }
  const unsigned per = (unsigned)M * (unsigned)N;
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q * 4u >= per) return;
  const unsigned w = q * 4u;
  const int z = blockIdx.y;
  const unsigned m = w / (unsigned)N, n = w - m * (unsigned)N;
  const float* src = slab + ((long)z * split) * per + w;
  float4 s = *reinterpret_cast<const float4*>(src);
  for (int k = 1; k < split; ++k) {
    const float4 a = *reinterpret_cast<const float4*>(src + (long)k * per);
    s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
  }
  if (bias) {
    s.x += bias[n]; s.y += bias[n + 1]; s.z += bias[n + 2]; s.w += bias[n + 3];
  }
  float* dst = C + (long)z * sc + (long)m * ldc + n;
  if (((uintptr_t)dst & 15) == 0) *reinterpret_cast<float4*>(dst) = s;
  else { dst[0] = s.x; dst[1] = s.y; dst[2] = s.z; dst[3] = s.w; }
}


// The LDS-DMA kernel takes plain strided bf16 operands whose 16-B chunks never straddle the
// reduction edge: K-major operands need K % 64 == 0, MN-major ones M (N) % 8 == 0, and every
// batch must fit the 32-bit range of a buffer resource.
bool pipe_ok(const cfm_gemm_desc& d, const GemmP& p, bool va, bool vb) {
  if (!va || !vb || p.cmap) return false;
  if (p.k_per_split % BK16) return false;
  auto fits = [](long bytes) { return bytes > 0 && bytes < (1L << 31); };
  const long ea = pipe_extent(d.a_kmajor, d.M, d.K, d.lda), eb = pipe_extent(d.b_kmajor, d.N, d.K, d.ldb);
  if (!fits(ea * 2) || !fits(eb * 2)) return false;
  // K-major: whole 16-B chunks along K; a partial last K tile reads zero past K (the kernels' tail stage), so K need
  // not be a multiple of the tile depth -- Conformer-S's K = 144 / 432 / 288 (d 144) take the pipeline too
  const int kq = p.split_k == 1 ? 8 : BK16;
  if (d.a_kmajor ? d.K % kq != 0 : d.M % 8 != 0) return false;
  if (d.b_kmajor ? d.K % kq != 0 : d.N % 8 != 0) return false;
  return true;
}

// the staged-epilogue fast path a launch can take (EF_*, epi_rows_fast; EF_GENERIC: the epilogue_store8 rows)
int epi_fast_kind(const GemmP& p, int batch, int mode) {
  if (p.split_k != 1 || !p.vec_c || p.N % 8 || p.cmap || (p.dbg & 2) || (mode & CFM_GEMM_MODE_GENERIC_EPILOGUE))
    return EF_GENERIC;
  if (p.drop_p > 0.f && (p.doff + (uint64_t)batch * p.M * p.N) / 2 + 8 > 0xFFFFFFFBull) return EF_GENERIC;
  const bool f32 = p.dtc == CFM_F32, bf = p.dtc == CFM_BF16, silu = p.act == CFM_ACT_SILU;
  const bool a1 = p.alpha == 1.f, s1 = p.out_scale == 1.f;
  if (!f32 && !bf) return EF_GENERIC;
  if (p.res) {
    if (!p.bias || !a1 || silu || p.act_grad || p.rd_out) return EF_GENERIC;
    if (f32) return p.dtr == CFM_F32 ? EF_F32_RES : EF_GENERIC;
    return p.dtr == CFM_BF16 ? EF_BF16_RES : p.dtr == CFM_F32 ? EF_F32R_BF16 : EF_GENERIC;
  }
  if (p.act_grad)
    return bf && p.dtpre == CFM_BF16 && !p.bias && a1 && s1 && !silu && !p.rd_out ? EF_BF16_ACTG : EF_GENERIC;
  if (p.rd_out)
    return bf && !p.bias && a1 && s1 && !silu && p.drop_p <= 0.f ? EF_BF16_RD : EF_GENERIC;
  if (f32) return silu && p.pre && p.dtpre != CFM_BF16 ? EF_GENERIC : EF_F32;
  if (silu) return p.pre && p.dtpre == CFM_BF16 && p.bias && a1 && s1 ? (p.mxo8 ? EF_BF16_SILU_MX : EF_BF16_SILU)
                                                                        : EF_GENERIC;
  if (p.drop_p > 0.f || !s1)
    return bf && p.bias && a1 && p.act == CFM_ACT_NONE && !p.pre ? EF_BF16_DELTA : EF_GENERIC;
  if (!a1) return EF_GENERIC;
  return p.bias ? EF_BF16_BIAS : EF_BF16;
}

void set_choice(cfm_gemm_choice* c, int variant, int ek, int bm, int bn, const GemmP& p, int batch, unsigned block) {
  c->variant = variant;
  c->epilogue = ek;
  c->grid_x = cdiv(p.N, bn);
  c->grid_y = cdiv(p.M, bm);
  c->grid_z = batch * p.split_k;
  c->block = block;
}

// The bf16 LDS-DMA rules (p.efast: the kind epi_fast_kind allows; only the K-major x K-major kernels carry one, and
// of those not PIPE192 / PIPE256, which exist with the generic epilogue alone).  The variants and what was measured
// for each rule: gemm_variants.h.
int pipe_choice(const cfm_gemm_desc& d, const GemmP& p, int mode, int cus, cfm_gemm_choice* c) {
  if (cdiv(p.M, 128) > 65535 || (long)d.batch * p.split_k > 65535)
    return cfm::fail(CFM_ERR_SHAPE, "gemm: grid too large");
  const bool ak = d.a_kmajor != 0, bkm = d.b_kmajor != 0;
  const int batch = d.batch, ek = ak && bkm ? p.efast : EF_GENERIC;
  const int sel = (mode & CFM_GEMM_MODE_SEL_MASK) >> CFM_GEMM_MODE_SEL_SHIFT;
  int v = sel;
  // auto: 129..160-column outputs (Conformer-S's d = 144) on 64 x 160 tiles: ONE column tile (the 128-wide tiles
  // took two, the second 16 columns wide -- 126 workgroups for 256 CUs with 44 % of the MFMA work padding); these
  // K <= 576 GEMMs are bandwidth-bound, so the tile's 187 row blocks each stream their A rows once
  if (ak && bkm && v == CFM_GEMM_SEL_AUTO && p.N > 128 && p.N <= 160 && p.split_k == 1 &&
      !(mode & CFM_GEMM_MODE_KEEP_128WIDE)) {
    set_choice(c, CFM_GEMM_V_PIPE64X160, ek, 64, 160, p, batch, 320);
    return CFM_OK;
  }
  if (ak) {
    // auto: outputs <= 512 columns (the encoder's d-wide outputs) take the 192-row tiles: 63 x 4 = 252
    // tiles fill 256 CUs in one round where 256-row tiles leave 68 CUs idle (A/B: 9-18 % faster)
    if (v == CFM_GEMM_SEL_192 ||
        (v == CFM_GEMM_SEL_AUTO && p.N <= 512 && p.split_k == 1 && (long)p.M * batch >= 4096)) {
      // warp-specialised loading: d-wide layer family 266.6 -> 240.2 us same box (4 compute waves of 96 x 64: 244.4 us)
      if (bkm && !(mode & CFM_GEMM_MODE_KEEP_SHARED_DMA) && p.split_k == 1) {
        // outputs narrow enough that 192-row tiles leave most CUs idle (Conformer-M's d = 256: 63 x 2 = 126 tiles
        // for 256 CUs) take 96-row tiles -- 125 x 2 = 250, one round
        const long tiles192 = (long)cdiv(p.N, BN) * cdiv(p.M, 192) * batch * p.split_k;
        if (tiles192 * 5 <= (long)cus * 3 && !(mode & CFM_GEMM_MODE_KEEP_WS192))
          set_choice(c, CFM_GEMM_V_WS96, ek, 96, BN, p, batch, 768);
        else
          set_choice(c, CFM_GEMM_V_WS192, ek, 192, BN, p, batch, 768);
        return CFM_OK;
      }
      // 4-deep ring: FFN-up data gradient 34.2 -> 32.5 us same-box
      set_choice(c, CFM_GEMM_V_PIPE192, EF_GENERIC, 192, BN, p, batch, 512);
      return CFM_OK;
    }
    // auto: 1024- / 1536-wide outputs of short reductions (QKV, pointwise-conv-1 forward) take 192-row tiles
    // two per CU: 504 / 756 tiles fill the 512 slots in whole rounds where 256-row tiles leave a sliver
    // (A/B, profiles/r02/gemm_v192s8_ab.txt: QKV 41.1 -> 36.1 us, pw1 27.7 -> 24.8 us)
    if (v == CFM_GEMM_SEL_AUTO && p.N > 512 && p.N <= 1536 && p.k_per_split <= 512 && p.split_k == 1 && p.M >= 4096 &&
        !(mode & CFM_GEMM_MODE_NO_192S8_RULE))
      v = CFM_GEMM_SEL_PIPE192S8;
    // the same outputs, K-major x K-major, on the warp-specialised kernel: QKV 32.41 -> 30.97 us, pw1 22.53 ->
    // 21.41 us same box, bit-identical (the 2048-wide ones stay on the two-per-CU 256-row tiles: 45.5 vs 57.3 us).
    // Short reductions, K <= 256 -- Conformer-S's FFN up / down-gradient at K 144: three K tiles -- keep the
    // two-per-CU pipeline: S15 step 8.27 -> 8.07 ms same box
    if (bkm && v == CFM_GEMM_SEL_PIPE192S8 && sel == CFM_GEMM_SEL_AUTO && !(mode & CFM_GEMM_MODE_KEEP_PIPE192) &&
        p.k_per_split > 256) {
      set_choice(c, CFM_GEMM_V_WS192, ek, 192, BN, p, batch, 768);
      return CFM_OK;
    }
    if (v == CFM_GEMM_SEL_PIPE192S8) {
      set_choice(c, CFM_GEMM_V_PIPE192S8, ek, 192, BN, p, batch, 512);
      return CFM_OK;
    }
  }
  // auto: short reductions (K <= 512: the epilogue is a large share of the tile's time) run two
  // 256-row workgroups per CU so one's epilogue hides under the other's MFMAs; long ones keep BK 64
  // (V128S measured no faster for N = 512 outputs)
  if (v != CFM_GEMM_SEL_PIPE256 && v != CFM_GEMM_SEL_PIPE256S)
    v = p.k_per_split <= 512 ? CFM_GEMM_SEL_PIPE256S : CFM_GEMM_SEL_PIPE256;
  if (v == CFM_GEMM_SEL_PIPE256) set_choice(c, CFM_GEMM_V_PIPE256, EF_GENERIC, 256, BN, p, batch, 512);
  else set_choice(c, CFM_GEMM_V_PIPE256S, ek, 256, BN, p, batch, 512);
  return CFM_OK;
}

// fp8 e4m3 x e4m3 (K-major both), p.K in bf16 pairs.  MX: d-wide outputs, and any K > 512 (the 2048-deep scale rows
// -- 20 KiB -- do not fit beside a two-per-CU ring) take the 192-row tile; K <= 512 (FFN up, QKV: 6 KiB of scale
// rows beside the 72 KiB ring) two 256-row workgroups per CU.  Per-tensor scales: by the output width alone.
void fp8_choice(const cfm_gemm_desc& d, const GemmP& p, cfm_gemm_choice* c) {
  if (d.mx_a) {
    if (p.N <= 512 || d.K > 512) set_choice(c, CFM_GEMM_V_MX192, p.efast, 192, BN, p, 1, 512);
    else set_choice(c, CFM_GEMM_V_MX256S, p.efast, 256, BN, p, 1, 512);
  } else {
    if (p.N <= 512) set_choice(c, CFM_GEMM_V_FP8_192, EF_GENERIC, 192, BN, p, 1, 512);
    else set_choice(c, CFM_GEMM_V_FP8_256S, EF_GENERIC, 256, BN, p, 1, 512);
  }
}

#define GEMM_REQUIRE(cond, code, msg)                                          \
  do {                                                                         \
    if (!(cond)) return cfm::fail((code), std::string("cfm_gemm: ") + (msg)); \
  } while (0)

// Validate d, build the kernel parameter block and select the kernel (c->variant CFM_GEMM_V_NONE: an empty output,
// nothing to launch).  Pure host arithmetic on the descriptor's values: no GPU API, no pointer dereferenced.
int gemm_prepare(const cfm_gemm_desc* d, int mode, int cus, GemmP* pp, cfm_gemm_choice* c) {
  GEMM_REQUIRE(d != nullptr, CFM_ERR_ARG, "null descriptor");
  GEMM_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0 && d->batch >= 1, CFM_ERR_SHAPE, "bad M/N/K/batch");
  GEMM_REQUIRE(d->dtype_ab == CFM_F32 || d->dtype_ab == CFM_BF16 || d->dtype_ab == CFM_FP8, CFM_ERR_DTYPE, "dtype_ab");
  GEMM_REQUIRE(d->A && d->B && d->C, CFM_ERR_ARG, "null operand");
  GEMM_REQUIRE(d->act == CFM_ACT_NONE || d->act == CFM_ACT_SILU, CFM_ERR_ARG, "act");
  GEMM_REQUIRE(!d->act_grad || d->pre, CFM_ERR_ARG, "act_grad needs pre");
  const int split = d->split_k < 1 ? 1 : d->split_k;
  GEMM_REQUIRE(split == 1 || (d->dtype_c == CFM_F32 && d->act == CFM_ACT_NONE && !d->act_grad &&
                              !d->residual && d->drop_p <= 0.f),
               CFM_ERR_ARG, "split_k needs a plain fp32 epilogue");
  // A and B are read-only: rows may overlap (ld below the row length -- the folded front-end's windowed view
  // of the packed mels, frontfold.hip) when the caller says so (allow_overlap); C rows may not
  GEMM_REQUIRE(d->lda >= 1 && d->ldb >= 1, CFM_ERR_SHAPE, "lda / ldb");
  GEMM_REQUIRE(d->allow_overlap || (d->lda >= (d->a_kmajor ? d->K : d->M) && d->ldb >= (d->b_kmajor ? d->K : d->N)),
               CFM_ERR_SHAPE, "lda / ldb below the row length (overlapping rows need allow_overlap)");
  GEMM_REQUIRE(d->ldc >= d->N, CFM_ERR_SHAPE, "ldc");
  *c = cfm_gemm_choice{};
  if (d->M == 0 || d->N == 0) return CFM_OK;

  GemmP& p = *pp;
  p = plain_params(d->M, d->N, d->K, d->C, d->ldc, d->dtype_c);
  p.sc = d->stride_c;
  p.alpha = d->alpha; p.bias = d->bias; p.act = d->act; p.act_grad = d->act_grad;
  p.pre = d->pre; p.dtpre = d->dtype_pre;
  p.drop_p = d->drop_p; p.seed = d->drop_seed; p.doff = d->drop_offset; p.salt = cfm::g_rng_salt;
  p.out_scale = d->out_scale; p.res = d->residual; p.ldr = d->ldr; p.dtr = d->dtype_r;
  p.split_k = split;
  p.probe = d->probe;
  p.vec_c = vec_epilogue_ok(p);
  GEMM_REQUIRE(!d->mx_out || d->dtype_ab == CFM_FP8, CFM_ERR_UNSUPPORTED, "mx_out: fp8 MX launches only");
  if (d->dtype_ab == CFM_FP8) {
    GEMM_REQUIRE(d->a_kmajor && d->b_kmajor && d->K % 128 == 0 && d->lda % 16 == 0 && d->ldb % 16 == 0 &&
                     (uintptr_t)d->A % 16 == 0 && (uintptr_t)d->B % 16 == 0 && split == 1 && d->batch == 1 &&
                     !d->rowdot_out && !d->a_colsum && (long)d->M * d->lda < (1L << 31) &&
                     (long)d->N * d->ldb < (1L << 31),
                 CFM_ERR_UNSUPPORTED, "fp8: K-major A and B, K % 128 == 0, 16-B aligned rows, no split-K / batch");
    GEMM_REQUIRE(!d->mx_a == !d->mx_b && (!d->mx_a || (d->K <= 2048 && !d->alpha_a_dev && !d->alpha_b_dev)),
                 CFM_ERR_ARG, "fp8 MX: both scale tensors, K <= 2048, no per-tensor alpha");
    GEMM_REQUIRE(!d->mx_out || (d->mx_a && d->mx_out_scales && d->dtype_c == CFM_BF16 && d->ldc == d->N &&
                                d->N % 32 == 0 && (uintptr_t)d->mx_out % 8 == 0),
                 CFM_ERR_UNSUPPORTED, "mx_out: MX operands, bf16 C with ldc == N, N % 32 == 0");
    // operands viewed as bf16 pairs (K/2 "elements" per row), so DMA / swizzle / epilogue are the bf16 kernel's
    p.K = d->K / 2;
    p.k_per_split = p.K;
    p.alpha_a = d->alpha_a_dev;
    p.alpha_b = d->alpha_b_dev;
    if (d->mx_a) {
      // MX operands: block scales applied inside the MFMA, so alpha stays 1 and the fast epilogue kinds apply
      p.mxa = d->mx_a;
      p.mxb = d->mx_b;
      p.mxk = d->K / 32;
      p.mxo8 = (uint8_t*)d->mx_out;
      p.mxos = d->mx_out_scales;
      p.efast = epi_fast_kind(p, 1, mode);
      if (p.mxo8 && p.efast != EF_BF16_SILU_MX)
        return cfm::fail(CFM_ERR_UNSUPPORTED, "cfm_gemm: mx_out needs the FFN-up epilogue (bias + SiLU + bf16 pre, "
                                              "bf16 C, ldc == N, N % 32 == 0)");
    }
    fp8_choice(*d, p, c);
    return CFM_OK;
  }
  const bool bf = d->dtype_ab == CFM_BF16;
  p.k_per_split = split_k_for(p, bf ? BK16 : BK32);
  const bool va = strided_vec_ok(d->A, d->lda, d->stride_a, bf), vb = strided_vec_ok(d->B, d->ldb, d->stride_b, bf);
  const bool pipe = bf && (mode & CFM_GEMM_MODE_PIPE) && pipe_ok(*d, p, va, vb);
  if (split > 1 && d->workspace) {
    GEMM_REQUIRE(d->N % 4 == 0 && d->ldc % 4 == 0, CFM_ERR_SHAPE, "slab split-K needs N % 4 == 0");
    p.slab = d->workspace;
  }
  if (d->rowdot_out) {
    GEMM_REQUIRE(bf && d->dtype_c == CFM_BF16 && d->rowdot_with && d->N % 64 == 0 && d->rowdot_T > 0 &&
                     d->M % d->rowdot_T == 0 && split == 1 && d->batch == 1 && pipe &&
                     ((uintptr_t)d->rowdot_with % 16) == 0,
                 CFM_ERR_UNSUPPORTED, "rowdot needs bf16 C on the LDS-DMA path, N % 64 == 0, no split-K, batch 1");
    p.rd_with = (const bf16*)d->rowdot_with;
    p.rd_out = d->rowdot_out;
    p.rd_T = d->rowdot_T;
  }
  if (d->a_colsum) {
    GEMM_REQUIRE(bf && !d->a_kmajor && p.slab && d->batch == 1 && pipe, CFM_ERR_UNSUPPORTED,
                 "a_colsum needs the bf16 LDS-DMA path, MN-major A, slab split-K, batch 1");
    p.acs_slab = p.slab + (long)split * d->M * d->N;
  }
  int rc;
  if (pipe) {
    p.dbg = ((mode & CFM_GEMM_MODE_SKIP_STORES) ? 1 : 0) | ((mode & CFM_GEMM_MODE_GENERIC_DROPOUT) ? 2 : 0) |
            ((mode & CFM_GEMM_MODE_SKIP_MAINLOOP) ? 4 : 0);
    p.efast = d->a_kmajor && d->b_kmajor ? epi_fast_kind(p, d->batch, mode) : EF_GENERIC;
    rc = pipe_choice(*d, p, mode, cus, c);
  } else {
    rc = staged_choice(bf, p, d->batch, mode, c);
  }
  if (rc != CFM_OK) return rc;
  if (p.slab)
    GEMM_REQUIRE((long)d->M * d->N < (1L << 31) && d->batch <= 65535, CFM_ERR_SHAPE, "split-K slab too large");
  return CFM_OK;
}

}  // namespace

namespace cfm {
void gemm_splitk_reduce(unsigned grid_x, unsigned batch, const float* slab, int split, int M, int N, float* C, long ldc,
                        long sc, const float* bias, const float* acs_slab, float* acs, hipStream_t s) {
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(grid_x, batch), dim3(256), 0, s, slab, split, M, N, C, ldc, sc, bias,
                     acs_slab, acs);
}
}  // namespace cfm

CFM_EXPORT int cfm_gemm_set_mode(int mode) {
  cfm::g_gemm_mode = mode;
  return CFM_OK;
}

CFM_EXPORT int cfm_gemm_plan(const cfm_gemm_desc* d, int mode, int cus, cfm_gemm_choice* out) {
  CFM_REQUIRE(out != nullptr && cus > 0, CFM_ERR_ARG, "null out or cus <= 0");
  GemmP p;
  return gemm_prepare(d, mode < 0 ? cfm::g_gemm_mode : mode, cus, &p, out);
}

CFM_EXPORT int cfm_gemm(const cfm_gemm_desc* d, void* stream) {
  GemmP p;
  cfm_gemm_choice c;
  const int rc = gemm_prepare(d, cfm::g_gemm_mode, cfm::num_cus(), &p, &c);
  if (rc != CFM_OK) return rc;
  hipStream_t s = cfm::as_stream(stream);
  switch (c.variant) {
    case CFM_GEMM_V_NONE: return CFM_OK;
    case CFM_GEMM_V_STAGED_BF16_256:
    case CFM_GEMM_V_STAGED_BF16_128:
    case CFM_GEMM_V_STAGED_F32_128:
    case CFM_GEMM_V_STAGED_F32_64: cfm::gemm_launch_staged(c, *d, &p, s); break;
    case CFM_GEMM_V_WS192:
    case CFM_GEMM_V_WS96: cfm::gemm_launch_ws(c, *d, &p, s); break;
    case CFM_GEMM_V_FP8_192:
    case CFM_GEMM_V_FP8_256S:
    case CFM_GEMM_V_MX192:
    case CFM_GEMM_V_MX256S: cfm::gemm_launch_fp8(c, *d, &p, s); break;
    default: cfm::gemm_launch_pipe(c, *d, &p, s); break;
  }
  if (p.slab) {
    const long n4 = (long)d->M * d->N / 4;
    const unsigned gx = (unsigned)((n4 + 255) / 256) > (unsigned)cdiv(d->M, 256) ? (unsigned)((n4 + 255) / 256)
                                                                                : (unsigned)cdiv(d->M, 256);
    cfm::gemm_splitk_reduce(gx, d->batch, p.slab, p.split_k, d->M, d->N, (float*)d->C, d->ldc, d->stride_c, d->bias,
                            p.acs_slab, d->a_colsum, s);
  }
  return cfm::check_launch("cfm_gemm");
}
