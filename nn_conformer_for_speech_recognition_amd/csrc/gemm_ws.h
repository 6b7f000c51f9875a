// gemm_ws.h -- gemm_ws_kernel: the warp-specialised K-major x K-major bf16 kernel.
#pragma once
#include "gemm_pipe.h"

namespace {

// ---------------------------------------------------------------- warp-specialised K-major GEMM
// For the encoder's d-wide outputs (one BMt x 128 tile per CU, K up to 2048): NL loader waves only issue the
// LDS-DMA of the ring's stages, wait for it (their vmcnt counts nothing else) and join the one barrier per K step;
// the WM x WN compute waves never touch vector memory in the main loop, so no stage wait ever stalls an MFMA wave
// and no DMA issue sits between its MFMAs.  The compute waves read the next half-step's fragments (16x16x32 MFMA,
// conflict-free ds_read_b128 from the source-swizzled image) while the current half-step's MFMAs run; the barrier
// sits where the next stage must become visible, and the slot of stage kt - 1 is refilled right after it (NST - 1
// stages issued ahead).  Gemm lab (benchmarks/gemm_lab, M 11,936 N 512 K 2048, naive stores): 33.9 -> 27.0 us.
// Epilogue: the whole f32 tile staged in the ring's LDS, then every wave (loaders included) finishes 8-column
// chunks through epilogue_store8 (+ rowdot), as tile_epilogue_g does.
template <int BMt, int WM, int WN, int NL, int NST, int EK = EF_GENERIC>
__global__ __launch_bounds__((WM * WN + NL) * 64) void gemm_ws_kernel(GemmP p, PipeOp oa, PipeOp ob) {
  constexpr int BKt = 64, BNt = BN, NC = WM * WN, NTt = (NC + NL) * 64;
  constexpr int ABYTES = BMt * BKt * 2, BBYTES = BNt * BKt * 2, STAGE = ABYTES + BBYTES;
  constexpr int AP = ABYTES / 1024, BP = BBYTES / 1024, PW = (AP + BP) / NL;
  static_assert(PW * NL == AP + BP && AP * 1024 == ABYTES && BP * 1024 == BBYTES, "whole DMA pieces per loader");
  constexpr int FM = BMt / WM / 16, FN = BNt / WN / 16;
  static_assert(FM * WM * 16 == BMt && FN * WN * 16 == BNt, "wave tiling");
  constexpr int EPS = BNt + 4, CPW = BNt / 8;
  constexpr int RING = NST * STAGE, EPI = BMt * EPS * 4;
  static_assert(NST >= 3 && NST <= 5, "ring depth");
  __shared__ __attribute__((aligned(1024))) char lds[RING > EPI ? RING : EPI];
  probe_begin(p.probe);
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tm, tn, zz;
  xcd_tile3(tm, tn, zz);
  const int m0 = tm * BMt, n0 = tn * BNt;
  const int z = zz;                       // split_k == 1: the batch index
  const int nk = (p.dbg & 4) ? 0 : (p.K + BKt - 1) / BKt;   // (dbg 4: epilogue only; a partial last tile: below)
  // the epilogue rows' global inputs (f32 residual / bf16 rd_with / pre-activation), issued before the main loop
  // so their latency hides under it (the loaders' counted stage waits see them as older, completed first)
  constexpr int EIT = BMt * CPW / NTt;
  EpiIn<EK == EF_GENERIC ? EF_BF16 : EK, EIT> ein;
  if constexpr (EK != EF_GENERIC) epi_load_all<EK, EIT, NTt, CPW>(p, z, m0, n0, tid, ein);
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (wid >= NC) {
    // ---- loader waves
    const int lw = wid - NC;
    const __amdgpu_buffer_rsrc_t ra = pipe_rsrc(oa, z), rb = pipe_rsrc(ob, z);
    unsigned off[PW];
    int ldo[PW], kc[PW];
    bool isa[PW];
#pragma unroll
    for (int i = 0; i < PW; ++i) {
      const int q = lw + NL * i;
      isa[i] = q < AP;
      const int qq = isa[i] ? q : q - AP;
      off[i] = isa[i] ? pipe_src<true, BMt, BKt>(oa, qq * 64 + lane, m0, 0)
                      : pipe_src<true, BNt, BKt>(ob, qq * 64 + lane, n0, 0);
      ldo[i] = (isa[i] ? 0 : ABYTES) + qq * 1024;
      kc[i] = pipe_kchunk<BKt>(qq * 64 + lane);
    }
    // K % BKt != 0 (K % 8 == 0): the last tile's chunks at k >= K read zero (out-of-range offset), not the next row
    const int klast = p.K - (nk - 1) * BKt;
    auto issue = [&](int kt) {
      if (kt == nk - 1 && klast < BKt) {   // wave-uniform
#pragma unroll
        for (int i = 0; i < PW; ++i)
          dma16(isa[i] ? ra : rb, lds + (kt % NST) * STAGE + ldo[i], kc[i] < klast ? off[i] + kt * (BKt * 2) : 0xFFFFFF00u);
        return;
      }
#pragma unroll
      for (int i = 0; i < PW; ++i)
        dma16(isa[i] ? ra : rb, lds + (kt % NST) * STAGE + ldo[i], off[i] + kt * (BKt * 2));
    };
    // stage s has landed once only the stages issued after it (up to `last`) are outstanding
    auto wait_stage = [&](int s, int last) {
      const int younger = min(NST - 2, last - s);
      if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PW) : "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PW) : "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    for (int s = 0; s < NST - 1 && s < nk; ++s) issue(s);
    int last = min(NST - 2, nk - 1);
    wait_stage(0, last);
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt + 1 < nk; ++kt) {
      wait_stage(kt + 1, last);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const int kn = kt + NST - 1;          // refills the slot of stage kt - 1 (every wave is past its reads)
      if (kn < nk) {
        issue(kn);
        last = kn;
      }
    }
  } else {
    // ---- compute waves
    const int wm = wid / WN, wn = wid % WN;
    bf16x8 af[2][FM], bfr[2][FN];
    auto read = [&](bf16x8 (&fa)[FM], bf16x8 (&fb)[FN], int kt, int sub) {
      const char* sa = lds + (kt % NST) * STAGE;
      const char* sb = sa + ABYTES;
#pragma unroll
      for (int j = 0; j < FN; ++j) fb[j] = pipe_frag16k<BKt>(sb, wn * FN * 16 + 16 * j, 32 * sub, lane);
#pragma unroll
      for (int i = 0; i < FM; ++i) fa[i] = pipe_frag16k<BKt>(sa, wm * FM * 16 + 16 * i, 32 * sub, lane);
    };
    auto mma = [&](const bf16x8 (&fa)[FM], const bf16x8 (&fb)[FN]) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    };
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    read(af[0], bfr[0], 0, 0);
    for (int kt = 0; kt < nk; ++kt) {
      read(af[1], bfr[1], kt, 1);
      mma(af[0], bfr[0]);
      if (kt + 1 < nk) {
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        read(af[0], bfr[0], kt + 1, 0);
      }
      mma(af[1], bfr[1]);
    }
  }
  if (p.dbg & 1) {   // timing experiment: keep the accumulators live, store nothing
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) t += acc[i][j][0] + acc[i][j][3];
    if (t == -1234.5f) reinterpret_cast<float*>(p.C)[tid] = t;
    return;
  }
  gemm_drop_prep(p);   // (here, not at the top: its counter load would hold back the loaders' first stage)
  float bias8[8];
  if constexpr (EK != EF_GENERIC) epi_bias8(p, n0 + (tid % CPW) * 8, bias8);
  __syncthreads();   // every DMA landed (the loaders' last wait was vmcnt(0)), every fragment read consumed
  float* st = reinterpret_cast<float*>(lds);
  if (wid < NC) {
    const int wm = wid / WN, wn = wid % WN;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          st[(wm * FM * 16 + 16 * i + 4 * (lane >> 4) + e) * EPS + wn * FN * 16 + 16 * j + (lane & 15)] = acc[i][j][e];
  }
  __syncthreads();
  static_assert((BMt * CPW) % NTt == 0 && NTt % CPW == 0, "whole rows per pass");
  if constexpr (EK != EF_GENERIC) {
    epi_rows_fast<EK, EIT, NTt, CPW, EPS, true>(p, st, z, m0, n0, tid, bias8, ein);
    probe_end(p.probe);
    return;
  }
#pragma unroll 2
  for (int it = 0; it < BMt * CPW / NTt; ++it) {
    const int row = it * (NTt / CPW) + tid / CPW, c8 = (tid % CPW) * 8;
    const float4 lo = *reinterpret_cast<const float4*>(st + row * EPS + c8);
    const float4 hi = *reinterpret_cast<const float4*>(st + row * EPS + c8 + 4);
    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const int m = m0 + row;
    epilogue_store8(p, z, zz, m, n0 + c8, v);
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
  probe_end(p.probe);
}

}  // namespace
