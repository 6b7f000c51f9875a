// gemm_pipe.hip -- instantiates the bf16 LDS-DMA pipeline variants cfm_gemm selects (gemm_variants.h), for the four
// operand layouts.
#include "gemm_launch.h"
#include "gemm_variants.h"

namespace {

// (the `if constexpr`s only keep a layout from instantiating variants the selection never gives it)
template <bool AK, bool BKM, bool M16 = false>
void launch_pipe_t(const cfm_gemm_choice& c, const GemmP& p, const PipeOp& oa, const PipeOp& ob, hipStream_t s) {
  const dim3 grid(c.grid_x, c.grid_y, c.grid_z), block(c.block);
  switch (c.variant) {
    case CFM_GEMM_V_PIPE64X160:
      if constexpr (AK && BKM)
        ek_dispatch<true>(c.epilogue, [&](auto ek) {
          hipLaunchKernelGGL((kPipe64x160<M16, decltype(ek)::value>), grid, block, 0, s, p, oa, ob, GatherA{});
        });
      break;
    case CFM_GEMM_V_PIPE192:
      if constexpr (AK) hipLaunchKernelGGL((kPipe192<AK, BKM, M16>), grid, block, 0, s, p, oa, ob, GatherA{});
      break;
    case CFM_GEMM_V_PIPE192S8:
      if constexpr (AK)
        ek_dispatch<AK && BKM>(c.epilogue, [&](auto ek) {
          hipLaunchKernelGGL((kPipe192S8<AK, BKM, M16, decltype(ek)::value>), grid, block, 0, s, p, oa, ob, GatherA{});
        });
      break;
    case CFM_GEMM_V_PIPE256:
      hipLaunchKernelGGL((kPipe256<AK, BKM, M16>), grid, block, 0, s, p, oa, ob, GatherA{});
      break;
    case CFM_GEMM_V_PIPE256S:
      ek_dispatch<AK && BKM>(c.epilogue, [&](auto ek) {
        hipLaunchKernelGGL((kPipe256S<AK, BKM, M16, decltype(ek)::value>), grid, block, 0, s, p, oa, ob, GatherA{});
      });
      break;
    default: break;
  }
}

}  // namespace

namespace cfm {

void gemm_launch_pipe(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* pv, hipStream_t s) {
  const GemmP& p = *static_cast<const GemmP*>(pv);
  const PipeOp oa = pipe_op(d.A, d.a_kmajor, d.M, d.K, d.lda, d.stride_a);
  const PipeOp ob = pipe_op(d.B, d.b_kmajor, d.N, d.K, d.ldb, d.stride_b);
  const bool ak = d.a_kmajor != 0, bkm = d.b_kmajor != 0;
  // the K-major x K-major GEMMs (forward and data-gradient) run 16x16x32 MFMA main loops (L15 step 25.0 -> 24.7 ms
  // same-box A/B)
  if (ak && bkm) launch_pipe_t<true, true, true>(c, p, oa, ob, s);
  else if (ak) launch_pipe_t<true, false>(c, p, oa, ob, s);
  else if (bkm) launch_pipe_t<false, true>(c, p, oa, ob, s);
  else launch_pipe_t<false, false>(c, p, oa, ob, s);
}

}  // namespace cfm
