// gemm_fp8.hip -- instantiates the fp8 e4m3 x e4m3 (K-major both) variants of the LDS-DMA pipeline on the block-scaled
// MFMA (2x the bf16 rate): MX operands (e8m0 block scales inside the MFMA, the fast epilogue kinds) and per-tensor
// scales (applied in the generic epilogue).
#include "gemm_launch.h"
#include "gemm_variants.h"

namespace cfm {

void gemm_launch_fp8(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* pv, hipStream_t s) {
  const GemmP& p = *static_cast<const GemmP*>(pv);
  // operands viewed as bf16 pairs (K/2 "elements" per row)
  const PipeOp oa{(const bf16*)d.A, d.lda / 2, 0, d.M, (unsigned)((long)d.M * d.lda)};
  const PipeOp ob{(const bf16*)d.B, d.ldb / 2, 0, d.N, (unsigned)((long)d.N * d.ldb)};
  const dim3 grid(c.grid_x, c.grid_y, c.grid_z), block(c.block);
  switch (c.variant) {
    case CFM_GEMM_V_MX192:
      ek_dispatch<true>(c.epilogue, [&](auto ek) {
        hipLaunchKernelGGL((kMx192<decltype(ek)::value>), grid, block, 0, s, p, oa, ob, GatherA{});
      });
      break;
    case CFM_GEMM_V_MX256S:
      ek_dispatch<true>(c.epilogue, [&](auto ek) {
        hipLaunchKernelGGL((kMx256S<decltype(ek)::value>), grid, block, 0, s, p, oa, ob, GatherA{});
      });
      break;
    case CFM_GEMM_V_FP8_192: hipLaunchKernelGGL((kFp8_192<>), grid, block, 0, s, p, oa, ob, GatherA{}); break;
    default: hipLaunchKernelGGL((kFp8_256S<>), grid, block, 0, s, p, oa, ob, GatherA{}); break;
  }
}

}  // namespace cfm
