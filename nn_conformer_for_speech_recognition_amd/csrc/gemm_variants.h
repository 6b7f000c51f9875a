// gemm_variants.h -- one name per kernel variant.  Each alias spells a positional template argument list once and
// leaves open what a launch site chooses: the operand layouts (AK / BKM: A / B K-major), the 16x16x32 main loop
// (M16) and the epilogue kind (EK, EF_* of gemm_epilogue.h).  An alias is the kernel's address: it names the same
// instantiation as the spelled-out list and adds no symbol.  cfm_gemm_variant (cfm.h) numbers the ones cfm_gemm
// selects; cfm_gemm_set_mode's selector field (CFM_GEMM_SEL_*) forces one for A/B measurements.
//
// gemm_pipe_kernel<BMt, BKt, NST, OCC, AK, BKM, NWV, WN, GA, GROUP, F8, BNt, M16, EK, MXK>: BMt x BNt tile, BKt-deep K
// steps, NST-stage ring, OCC workgroups per CU, NWV waves (block = 64 NWV) as NWV / WN x WN.
// gemm_ws_kernel<BMt, WM, WN, NL, NST, EK>: BMt x 128 tile, BK 64, WM x WN compute waves + NL loader waves.
//
// (measured slower and removed in round 4, A/B records in DESIGN.md §8: 128-row tiles, 96-row pipeline tiles, a
//  persistent register-deferred epilogue, an interleaved-epilogue persistent kernel, a tail-balanced row split,
//  32x32x16 main loops for K-major operands, a 3-deep 192-row ring; for the grouped weight gradients 256 x 128 BK 32
//  two per CU, 256 x 128 BK 64, plain dispatch order, a 256 x 256 BK 64 double-buffered form -- it spilled, 2.4x
//  slower --, a 5-deep ring and a warp-specialised 256 x 128 form)
#pragma once
#include "gemm_pipe.h"
#include "gemm_ws.h"

namespace {

// ---- bf16 pipeline, cfm_gemm (gemm_pipe.hip)
// 64 x 160 tile, BK 64, 4-deep ring (84 KiB: one workgroup per CU), 5 waves of 64 x 32, block 320: the 129..160-column
// outputs (Conformer-S's d = 144) in ONE column tile
template <bool M16, int EK>
constexpr auto kPipe64x160 = gemm_pipe_kernel<64, 64, 4, 1, true, true, 5, 5, false, false, false, 160, M16, EK>;
// V192: 192 x 128 tile, BK 64, 4-deep ring (4 x 40 KiB = the whole 160 KiB LDS: one per CU), 8 waves of 96 x 32,
// block 512: d-wide outputs whose operands are not both K-major (K-major x K-major ones: kWs192), generic epilogue
template <bool AK, bool BKM, bool M16>
constexpr auto kPipe192 = gemm_pipe_kernel<192, 64, 4, 1, AK, BKM, 8, 4, false, false, false, BN, M16>;
// V192S8: 192 x 128 tile, BK 32 (uneven A DMA split), 3-deep ring (60 KiB: two per CU), 8 waves of 96 x 32, block 512
template <bool AK, bool BKM, bool M16, int EK>
constexpr auto kPipe192S8 = gemm_pipe_kernel<192, 32, 3, 2, AK, BKM, 8, 4, false, false, false, BN, M16, EK>;
// V256: 256 x 128 tile, BK 64, 3-deep ring (144 KiB: one per CU), 8 waves of 64 x 64, block 512, generic epilogue
template <bool AK, bool BKM, bool M16>
constexpr auto kPipe256 = gemm_pipe_kernel<256, 64, 3, 1, AK, BKM, 8, 2, false, false, false, BN, M16>;
// V256S: 256 x 128 tile, BK 32, 3-deep ring (72 KiB: two per CU, one's epilogue under the other's main loop), 8 waves
// of 64 x 64, block 512
template <bool AK, bool BKM, bool M16, int EK>
constexpr auto kPipe256S = gemm_pipe_kernel<256, 32, 3, 2, AK, BKM, 8, 2, false, false, false, BN, M16, EK>;

// ---- warp-specialised, K-major x K-major (gemm_ws.hip): BK 64, 4-deep ring, 2 x 4 compute waves + 4 loader waves,
// block 768, one workgroup per CU
template <int EK> constexpr auto kWs192 = gemm_ws_kernel<192, 2, 4, 4, 4, EK>;   // 192 x 128 tile: d-wide and QKV-wide outputs
template <int EK> constexpr auto kWs96 = gemm_ws_kernel<96, 2, 4, 4, 4, EK>;     // 96 x 128 tile: outputs too narrow for 192 rows

// ---- fp8 e4m3, K-major x K-major (gemm_fp8.hip): the pipeline on the block-scaled MFMA, 8 waves, block 512
// 192 x 128 tile, BK 64 (bf16 pairs: 128 fp8), 3-deep ring, one per CU; MX: 64 scale bytes per row (K <= 2048)
template <int EK>
constexpr auto kMx192 = gemm_pipe_kernel<192, 64, 3, 1, true, true, 8, 4, false, false, true, BN, false, EK, 64>;
// 256 x 128 tile, BK 32, 3-deep ring, two per CU; MX: 16 scale bytes per row (K <= 512: 6 KiB beside the 72 KiB ring)
template <int EK>
constexpr auto kMx256S = gemm_pipe_kernel<256, 32, 3, 2, true, true, 8, 2, false, false, true, BN, false, EK, 16>;
// the same two tiles with per-tensor scales (generic epilogue)
template <int EK = EF_GENERIC>
constexpr auto kFp8_192 = gemm_pipe_kernel<192, 64, 3, 1, true, true, 8, 4, false, false, true, BN, false, EK>;
template <int EK = EF_GENERIC>
constexpr auto kFp8_256S = gemm_pipe_kernel<256, 32, 3, 2, true, true, 8, 2, false, false, true, BN, false, EK>;

// ---- fixed launches outside cfm_gemm's selection (templates only so that including this header instantiates nothing)
// conv2 forward (gemm_conv2.hip): V256's geometry with the gathered A operand
template <bool GA = true> constexpr auto kConv2Fwd = gemm_pipe_kernel<256, 64, 3, 1, true, true, 8, 2, GA>;
// conv2 data gradient, one parity class per launch: V256S's geometry with the gathered A operand
template <bool GA = true> constexpr auto kConv2Dgrad = gemm_pipe_kernel<256, 32, 3, 2, true, true, 8, 2, GA>;
// grouped weight gradients (gemm_wgrad.hip): 256 x 256 tile (half the dY panel re-reads of 256 x 128), BK 32, 4-deep
// ring (128 KiB: one per CU), MN-major x MN-major, 8 waves, block 512; 17 layers 5.46 -> 4.89 ms, L15 step -0.8 ms
constexpr int WG_BN = 256;
template <bool GROUP = true>
constexpr auto kWgradGroup = gemm_pipe_kernel<256, 32, 4, 1, false, false, 8, 2, false, GROUP, false, WG_BN>;

// f(std::integral_constant<int, EK>) for the launch's epilogue kind (K-major x K-major launches only: the other
// operand layouts keep the generic epilogue, so their kernels are instantiated once)
template <bool KK, class F>
void ek_dispatch(int ek, F&& f) {
  if constexpr (KK) {
    switch (ek) {
      case EF_BF16: f(std::integral_constant<int, EF_BF16>{}); return;
      case EF_BF16_BIAS: f(std::integral_constant<int, EF_BF16_BIAS>{}); return;
      case EF_BF16_SILU: f(std::integral_constant<int, EF_BF16_SILU>{}); return;
      case EF_BF16_ACTG: f(std::integral_constant<int, EF_BF16_ACTG>{}); return;
      case EF_BF16_RD: f(std::integral_constant<int, EF_BF16_RD>{}); return;
      case EF_F32: f(std::integral_constant<int, EF_F32>{}); return;
      case EF_F32_RES: f(std::integral_constant<int, EF_F32_RES>{}); return;
      case EF_BF16_RES: f(std::integral_constant<int, EF_BF16_RES>{}); return;
      case EF_F32R_BF16: f(std::integral_constant<int, EF_F32R_BF16>{}); return;
      case EF_BF16_DELTA: f(std::integral_constant<int, EF_BF16_DELTA>{}); return;
      case EF_BF16_SILU_MX: f(std::integral_constant<int, EF_BF16_SILU_MX>{}); return;
      default: break;
    }
  }
  f(std::integral_constant<int, EF_GENERIC>{});
}

}  // namespace
