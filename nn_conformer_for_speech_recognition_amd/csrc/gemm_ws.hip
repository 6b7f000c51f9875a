// gemm_ws.hip -- instantiates the warp-specialised K-major x K-major kernels (kWs192, kWs96: gemm_variants.h).
#include "gemm_launch.h"
#include "gemm_variants.h"

namespace cfm {

void gemm_launch_ws(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* pv, hipStream_t s) {
  const GemmP& p = *static_cast<const GemmP*>(pv);
  const PipeOp oa = pipe_op(d.A, d.a_kmajor, d.M, d.K, d.lda, d.stride_a);
  const PipeOp ob = pipe_op(d.B, d.b_kmajor, d.N, d.K, d.ldb, d.stride_b);
  const dim3 grid(c.grid_x, c.grid_y, c.grid_z), block(c.block);
  ek_dispatch<true>(c.epilogue, [&](auto ek) {
    switch (c.variant) {
      case CFM_GEMM_V_WS96:
        hipLaunchKernelGGL((kWs96<decltype(ek)::value>), grid, block, 0, s, p, oa, ob);
        break;
      default: hipLaunchKernelGGL((kWs192<decltype(ek)::value>), grid, block, 0, s, p, oa, ob); break;
    }
  });
}

}  // namespace cfm
