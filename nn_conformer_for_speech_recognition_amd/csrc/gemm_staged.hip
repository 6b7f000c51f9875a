// gemm_staged.hip -- instantiates the register-staged kernels for plain strided operands (cfm_gemm's fallback when
// the LDS-DMA path does not apply, and the fp32 parity mode).  The conv2 gather loaders' instantiations are
// gemm_conv2.hip's.
#include "gemm_staged.h"

namespace cfm {

void gemm_launch_staged(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* pv, hipStream_t s) {
  const GemmP& p = *static_cast<const GemmP*>(pv);
  const bool bf = d.dtype_ab == CFM_BF16;
  const bool va = strided_vec_ok(d.A, d.lda, d.stride_a, bf), vb = strided_vec_ok(d.B, d.ldb, d.stride_b, bf);
  const bool ak = d.a_kmajor != 0, bkm = d.b_kmajor != 0;
  auto go = [&](auto tag) {
    typedef decltype(tag) T;
    StridedOp<T> oa{(const T*)d.A, d.lda, d.stride_a, va};
    StridedOp<T> ob{(const T*)d.B, d.ldb, d.stride_b, vb};
    if (ak && bkm) launch_staged<true, true>(c, p, oa, ob, s);
    else if (ak) launch_staged<true, false>(c, p, oa, ob, s);
    else if (bkm) launch_staged<false, true>(c, p, oa, ob, s);
    else launch_staged<false, false>(c, p, oa, ob, s);
  };
  if (bf) go(bf16{});
  else go(float{});
}

}  // namespace cfm
