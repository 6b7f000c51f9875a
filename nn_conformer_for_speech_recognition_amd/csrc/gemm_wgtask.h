// gemm_wgtask.h -- one task of a grouped weight-gradient launch (WgTask) and the workgroup -> (task, tile, K slice)
// lookup the GROUP form of gemm_pipe_kernel runs (group_task).
#pragma once
#include "gemm_params.h"

namespace {

// All weight-gradient GEMMs dW_i = dY_iᵀ X_i (+ bias gradient sum_rows dY_i) of a backward pass in ONE
// launch: every task reduces over the same token dimension, so each 256x128 output tile is one
// workgroup running the whole K loop (no split-K slabs, no reduce pass), and the ~3000 tiles of the
// encoder's 17 layers fill the chip in whole rounds.  Workgroup -> (task, tile): XCD-contiguous ids
// (xcd_tile order), tasks back to back (tile0 ascending), tiles row-major inside a task.
// Planned form (cfm_wgrad_group_plan, GatherA.group_sched): one schedule word per workgroup -- task, tile, K slice
// -- laid out so that each XCD (workgroups b, b + 8, ... under round-robin placement) runs whole tasks in rounds of
// one tile per CU, i.e. every tile that shares a dY or X column slice with another is co-resident on that XCD and
// streams the slice through its L2 once; the tiles that do not fill whole rounds run split over K slices into fp32
// slabs (the task's p.split_k / k_per_split / slab / acs_slab), summed by wgrad_split_reduce_kernel.
struct WgTask {
  GemmP p;
  PipeOp oa, ob;
  long tile0;
  int tiles_n;
  int red_blocks;      // split task: blocks of wgrad_split_reduce_kernel (0: not split)
  long red0;           // first reduce block of this task
  float* dw;           // split task: the destinations the reduce writes (p.C / p.acs_slab point into the workspace)
  float* db;
};
static_assert(sizeof(WgTask) % 4 == 0, "word-copied task");
constexpr unsigned WG_SCHED_EMPTY = 0xFFFFFFFFu;   // padding workgroup of a planned launch
__host__ __device__ constexpr unsigned wg_sched_word(int task, int ks, int tile) {
  return ((unsigned)task << 20) | ((unsigned)ks << 16) | (unsigned)tile;
}

__device__ __forceinline__ bool group_task(const GatherA& ga, GemmP& p, PipeOp& oa, PipeOp& ob, int& tm, int& tn,
                                           int& zz) {
  const WgTask* tab = reinterpret_cast<const WgTask*>(ga.group_tab);
  int lo, local;
  zz = 0;
  if (ga.group_sched) {
    const unsigned w = __builtin_amdgcn_readfirstlane(ga.group_sched[blockIdx.x]);
    if (w == WG_SCHED_EMPTY) return false;
    lo = (int)(w >> 20);
    zz = (int)((w >> 16) & 15u);
    local = (int)(w & 0xFFFFu);
  } else {
    const int nwg = gridDim.x, L = blockIdx.x;
    int id = L;
    if (nwg > 8) {
      const int xcd = L & 7, q = nwg >> 3, r = nwg & 7;
      id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    }
    lo = 0;
    int hi = ga.group_n - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (__builtin_amdgcn_readfirstlane((int)tab[mid].tile0) <= id) lo = mid; else hi = mid - 1;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    local = id - (int)__builtin_amdgcn_readfirstlane((int)tab[lo].tile0);
  }
  // copy the task word by word through readfirstlane: the compiler then knows every field (buffer
  // descriptors, loop bounds) is wave-uniform -- SGPRs, no waterfall loops around the buffer loads
  WgTask t;
  const int* src = reinterpret_cast<const int*>(tab + lo);
  int* dst = reinterpret_cast<int*>(&t);
#pragma unroll
  for (int w = 0; w < (int)(sizeof(WgTask) / 4); ++w) dst[w] = __builtin_amdgcn_readfirstlane(src[w]);
  p = t.p;
  oa = t.oa;
  ob = t.ob;
  tm = local / t.tiles_n;
  tn = local % t.tiles_n;
  return true;
}

}  // namespace
