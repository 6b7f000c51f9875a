// gemm_launch.h -- what the GEMM translation units call across object boundaries.  Each kernel family is
// instantiated by one object; the others reach it through these functions.
//
// The kernels' parameter block (GemmP, gemm_params.h) lives in an unnamed namespace -- its name is part of every
// kernel's device symbol -- so it cannot appear in a signature with external linkage: it crosses as `const void*`
// (the same header-defined POD on both sides).  The launch functions are a switch over c.variant with no rule of
// their own; the choice comes from gemm.hip's selection (cfm_gemm_plan).
#pragma once
#include "cfm_common.h"

namespace cfm {

extern int g_gemm_mode;   // cfm_gemm_set_mode's word (CFM_GEMM_MODE_*; gemm.hip)

// p: the prepared GemmP of the call (efast, vec_c, dbg, ... set)
void gemm_launch_staged(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* p, hipStream_t s);   // gemm_staged.hip
void gemm_launch_pipe(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* p, hipStream_t s);     // gemm_pipe.hip
void gemm_launch_ws(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* p, hipStream_t s);       // gemm_ws.hip
void gemm_launch_fp8(const cfm_gemm_choice& c, const cfm_gemm_desc& d, const void* p, hipStream_t s);      // gemm_fp8.hip

// C[z] = sum of the split-K slabs (+ bias; + the A column sums), splitk_reduce_kernel (gemm.hip)
void gemm_splitk_reduce(unsigned grid_x, unsigned batch, const float* slab, int split, int M, int N, float* C, long ldc,
                        long sc, const float* bias, const float* acs_slab, float* acs, hipStream_t s);

}  // namespace cfm
