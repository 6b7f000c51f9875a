// gemm_pipe.h -- gemm_pipe_kernel: the LDS-DMA pipelined bf16 / fp8 / MX kernel (plain, gathered-A and grouped forms).
#pragma once
#include "gemm_epilogue.h"
#include "gemm_wgtask.h"

namespace {

// ---------------------------------------------------------------- bf16 pipelined kernel
// The fast path for plain strided bf16 operands.  Staging is LDS-DMA (buffer_load_dwordx4 ... lds:
// no VGPR round trip, no per-element predicates) into a PS-deep ring of LDS stages: two K tiles
// are in flight while the waves compute on a third, with one raw s_barrier and a counted
// vmcnt per K tile (a __syncthreads would drain the DMA queue every step).
//
// LDS-DMA writes a wave's 64 x 16 B contiguously, so bank-conflict-free images come from
// permuting the *source* chunks:
//   K-major [R][64] image (128-B rows, read by ds_read_b128 along k):
//       chunk c of row r lives at slot c ^ ((r >> 1) & 7)
//   MN-major [64][R] image (R*2-B k-rows, read by ds_read_b64_tr_b16):
//       chunk c of k-row k lives at slot c ^ (4 * (k & 3))
// Rows past M/N are clamped to the last valid row (their outputs are never stored); k-rows past K
// of an MN-major operand read as zero through the buffer resource's range check.
// BMt x 128 tile, BKt-deep K steps, NST-stage ring, NWV waves; the f32 epilogue staging aliases the ring
template <int BMt, int BKt, int NST, int NWV, int BNt = BN>
struct PipeGeo {
  static constexpr int NTt = NWV * 64, NW = NWV;
  static constexpr int ABYTES = BMt * BKt * 2, BBYTES = BNt * BKt * 2;
  static constexpr int STAGE = ABYTES + BBYTES;
  static constexpr int RING = NST * STAGE, EPI = (BMt < 128 ? BMt : 128) * (BNt + 4) * 4;
  static constexpr int LDS = RING > EPI ? RING : EPI;
  // 1-KiB DMA pieces per stage, spread over the waves: wave w issues pieces w, w + NW, ... (AI / BI rounds;
  // when a count is not a multiple of NW the first waves issue one more piece, and their counted waits say so)
  static constexpr int AP = ABYTES / 1024, BP = BBYTES / 1024;
  static constexpr int AI = (AP + NW - 1) / NW, BI = (BP + NW - 1) / NW;
  static_assert(AP * 1024 == ABYTES && BP * 1024 == BBYTES, "whole wave-instructions per stage");
  static constexpr bool EVEN = AI * NW == AP && BI * NW == BP;
};

// s_waitcnt vmcnt(n) for a wave-uniform run-time n (switch over the immediates a ring can need)
__device__ __forceinline__ void wait_vm_rt(int n) {
  switch (n) {
#define W(k) case k: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(k) : "memory"); break;
    W(0) W(1) W(2) W(3) W(4) W(5) W(6) W(7) W(8) W(9) W(10) W(11) W(12) W(13) W(14) W(15) W(16)
    W(17) W(18) W(19) W(20) W(21) W(22) W(23) W(24)
#undef W
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// the descriptor is wave-uniform by construction; readfirstlane makes that visible to the compiler even
// when the operand comes from memory (grouped launches), so no waterfall loop wraps the buffer loads
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pipe_rsrc(const PipeOp& o, int z) {
  const uint64_t a = (uint64_t)(uintptr_t)(o.base + (long)z * o.bstride);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), (short)0,
                                           __builtin_amdgcn_readfirstlane((int)o.bytes), 0x00020000);
}

// buffer resource over `bytes` bytes at p (MX block-scale rows; reads past the range return zero)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mx_rsrc(const uint8_t* p, long bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)hi << 32) | lo), (short)0,
                                           __builtin_amdgcn_readfirstlane((int)(bytes > 0 ? bytes : 0)), 0x00020000);
}

// one wave-instruction of LDS-DMA: lane l's 16 B from rsrc + voff land at lds_base + 16 l.
// Issued through inline asm: the compiler then does not know that it writes LDS, and does not put a
// conservative `s_waitcnt vmcnt(0)` in front of the next LDS read it cannot prove disjoint (it did so in the
// grouped weight-gradient loop, where every K step then waited for the DMA it had just issued).  Every
// consumer waits with its own counted vmcnt + barrier, so no compiler-inserted wait is needed.
// (m0 is declared clobbered -- the asm does overwrite it -- which clang reports as a reserved register once per
// instantiation; the warning is silenced here only)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t r, char* lds_base, unsigned voff) {
  const unsigned l = __builtin_amdgcn_readfirstlane(
      (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)lds_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds"
               :: "s"(l), "v"(voff), "s"(r) : "memory", "m0");
}
#pragma clang diagnostic pop

// K-major [R][BKt] image: BKt*2-B rows, RPB rows per 256-B bank row, CPR 16-B chunks per row;
// chunk c of row r sits in slot c ^ ((r / RPB) % CPR): 16 consecutive rows read at one k hit 16
// distinct 16-B bank groups (conflict-free ds_read_b128)
template <int BKt>
struct KmSw {
  static constexpr int RB = BKt * 2, CPR = BKt / 8, RPB = 256 / RB;
  __device__ static __forceinline__ int slot(int r, int c) { return c ^ ((r / RPB) & (CPR - 1)); }
};

// byte offset (in the operand) of the 16-B chunk that lands in LDS slot `lc` of an R-row image
template <bool KM, int R, int BKt>
__device__ __forceinline__ unsigned pipe_src(const PipeOp& o, int lc, int row0, int k0) {
  if constexpr (KM) {
    typedef KmSw<BKt> S;
    const int r = lc / S::CPR, c = S::slot(r, lc % S::CPR);
    const int row = row0 + r < o.lim ? row0 + r : o.lim - 1;
    return (unsigned)(((long)row * o.ld + k0 + 8 * c) * 2);
  } else {
    constexpr int CPR = R / 8;
    const int k = lc / CPR, c = (lc % CPR) ^ (4 * (k & 3));
    const int col = row0 + 8 * c < o.lim - 8 ? row0 + 8 * c : o.lim - 8;
    return (unsigned)(((long)(k0 + k) * o.ld + col) * 2);
  }
}

// k offset (elements, within the BKt-deep tile) of the 16-B chunk that lands in K-major LDS slot `lc`
template <int BKt>
__device__ __forceinline__ int pipe_kchunk(int lc) {
  typedef KmSw<BKt> S;
  const int r = lc / S::CPR;
  return 8 * S::slot(r, lc % S::CPR);
}

// one 32x32x16 operand fragment from a swizzled stage image
template <bool KM, int R, int BKt>
__device__ __forceinline__ bf16x8 pipe_frag(const char* img, int row0, int kk, int lane) {
  if constexpr (KM) {
    typedef KmSw<BKt> S;
    const int r = row0 + (lane & 31), c = (kk >> 3) + (lane >> 5);
    return *reinterpret_cast<const bf16x8*>(img + r * S::RB + 16 * S::slot(r, c));
  } else {
    const int h = lane >> 5, g1 = (lane >> 4) & 1, q = (lane & 15) >> 2, p4 = lane & 3;
    const int col = row0 + 16 * g1 + 4 * p4, k = kk + 8 * h + q;   // k & 3 == q for both halves
    const int off = 16 * ((col >> 3) ^ (4 * q)) + (col & 7) * 2;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + k * (R * 2) + off));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + (k + 4) * (R * 2) + off));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
}

// one 16x16x32 operand fragment (rows row0 .. row0+15, k = kk + 8 (lane >> 4) .. +7) from a K-major swizzled
// stage image: conflict-free ds_read_b128 on the 64-deep images (kk a multiple of 16)
template <int BKt>
__device__ __forceinline__ bf16x8 pipe_frag16k(const char* img, int row0, int kk, int lane) {
  typedef KmSw<BKt> S;
  const int r = row0 + (lane & 15), c = (kk >> 3) + (lane >> 4);
  return *reinterpret_cast<const bf16x8*>(img + r * S::RB + 16 * S::slot(r, c));
}

// wait until at most `younger` stages (of PER DMA instructions each) are still in flight
template <int PER>
__device__ __forceinline__ void wait_stages(int younger) {
  if (younger >= 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * PER) : "memory");
  else if (younger == 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory");
  else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
  else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// NWV waves as WM x WN, each owning FM x FN 32x32 accumulators: (BMt, NWV, WN) = (256, 8, 2) ->
// 64x64 per wave; (192, 8, 4) -> 96x32 per wave (192-row tiles: 63 x N/128 tiles of the encoder's
// M = 11,936 fill the 256 CUs in whole rounds); (128, 4, 2) -> 64x64.

// F8: A and B are fp8 e4m3 (OCP), K-major, viewed as bf16 PAIRS by everything up to the LDS image (K, ld and
// the tile geometry in 2-byte units, so DMA, swizzle and ring are byte-identical to the bf16 kernel); each
// 64-fp8 k-step (4 16-B chunks of a row) feeds one v_mfma_scale_f32_32x32x64_f8f6f4: lane (r, h) holds chunks h
// and h + 2 (the instruction's k order, see frag8).  Per-tensor fp8: unit block scales, the dequantisation
// (alpha_a * alpha_b) applied in the epilogue; MX: the e8m0 block scales below.
// M16: the main loop on v_mfma_f32_16x16x32_bf16 (each 32x32 block of a wave's tile as four 16x16 blocks; same
// LDS images, fragments per k and accumulator registers) -- K-major plain operands only.  On random data the
// chip holds a higher clock under the 16x16 shape than under 32x32x16 (MI355X_MICROARCH.md, DVFS item 7).
// MXK > 0 (F8 only): MX operands -- the tile's e8m0 block-scale rows (A rows m0.., B rows n0..: contiguous runs of
// mxk bytes each, mxk <= MXK) are DMA'd into LDS once, before the ring's first stage (so every stage wait covers
// them), and each fragment row's scales of a stage are read as one dword (BKt 64: 4 blocks) / short (BKt 32: 2);
// lane (r, h) of a 64-fp8 k-step q covers block 2q + h of the stage, shifted into the scale register's low byte.
template <int BMt, int BKt, int NST, int OCC, bool AK, bool BKM, int NWV = BMt / 32, int WN = 2, bool GA = false,
          bool GROUP = false, bool F8 = false, int BNt = BN, bool M16 = false, int EK = EF_GENERIC, int MXK = 0>
__global__ __launch_bounds__(NWV * 64) __attribute__((amdgpu_waves_per_eu(OCC * NWV / 4)))
void gemm_pipe_kernel(GemmP p, PipeOp oa, PipeOp ob, GatherA ga) {
  static_assert(!F8 || (AK && BKM && !GA && !GROUP && BKt % 32 == 0), "fp8: K-major plain operands");
  static_assert(MXK == 0 || (F8 && (BKt == 64 || BKt == 32) && ((BMt + BNt) * MXK) % 1024 == 0), "MX: fp8 only");
  static_assert(!M16 || (AK && BKM && !GA && !GROUP && !F8 && BKt % 32 == 0), "16x16x32: K-major plain bf16");
  typedef PipeGeo<BMt, BKt, NST, NWV, BNt> G;
  constexpr int WM = NWV / WN, FM = BMt / WM / 32, FN = BNt / WN / 32;
  static_assert(WM * FM * 32 == BMt && WN * FN * 32 == BNt, "wave tiling");
  static_assert(G::EVEN || (!GA && !GROUP), "uneven DMA split: plain operands only");
  probe_begin(p.probe);
  // (the dropout constants are prepared right before the epilogue: gemm_drop_prep loads the bound step counter,
  // and waiting for that load at the top held back the first DMA stage by one memory round trip)
  static_assert(NST >= 3 && NST <= 6, "ring depth");
  __shared__ __attribute__((aligned(1024))) char lds[G::LDS + (BMt + BNt) * MXK];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  int tm, tn, zz;
  if constexpr (GROUP) {
    unsigned long long* const probe = p.probe;   // the launch's timing slot survives the task's parameters
    // this workgroup's GEMM, tile and K slice of a grouped launch (a planned launch's padding workgroups exit)
    if (!group_task(ga, p, oa, ob, tm, tn, zz)) return;
    p.probe = probe;
    gemm_drop_prep(p);
  } else {
    xcd_tile3(tm, tn, zz);
  }
  const int m0 = tm * BMt, n0 = tn * BNt;
  const int z = zz / p.split_k, ks = zz % p.split_k;
  const __amdgpu_buffer_rsrc_t ra = pipe_rsrc(oa, z), rb = pipe_rsrc(ob, z);
  const int kbeg = __builtin_amdgcn_readfirstlane(ks * p.k_per_split);
  const int kend = __builtin_amdgcn_readfirstlane(min(p.K, kbeg + p.k_per_split));
  const int nk = kend > kbeg && !(p.dbg & 4) ? (kend - kbeg + BKt - 1) / BKt : 0;   // (dbg 4: epilogue only)

  // per-lane source offsets of stage 0; later stages add k0 * (row stride) (MN-major) or k0 * 2
  unsigned offa[G::AI], offb[G::BI];
  int gi[GA ? G::AI : 1], gj[GA ? G::AI : 1];   // gathered rows: class coordinates (i, j); gi < 0: past M
  if constexpr (GA) {
    static_assert(AK, "gathered A is K-major");
    typedef KmSw<BKt> S;
#pragma unroll
    for (int i = 0; i < G::AI; ++i) {
      const int lc = (i * G::NW + wid) * 64 + lane;
      const int r = lc / S::CPR, c = S::slot(r, lc % S::CPR), m = m0 + r;
      if (m < p.M) {
        const int j = m % ga.Jn, q = m / ga.Jn, ii = q % ga.In, b = q / ga.In;
        gi[i] = ii; gj[i] = j;
        offa[i] = (unsigned)((((long)b * ga.sB + (long)ii * ga.sI + (long)j * ga.sJ) * ga.Cr + 8 * c) * 2);
      } else {
        gi[i] = -1000; gj[i] = -1000; offa[i] = 0;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < G::AI; ++i)
      offa[i] = pipe_src<AK, BMt, BKt>(oa, ((i * G::NW + wid) % G::AP) * 64 + lane, m0, kbeg);
  }
#pragma unroll
  for (int i = 0; i < G::BI; ++i)
    offb[i] = pipe_src<BKM, BNt, BKt>(ob, ((i * G::NW + wid) % G::BP) * 64 + lane, n0, kbeg);
  // K tail (K-major operands, K % BKt != 0, K % 8 == 0): the last stage's chunks at k >= kend read zero through an
  // out-of-range offset (a K-major row's tail would otherwise read the next row's head); MN-major operands already
  // read zero past K (their extent ends at row K - 1).  kca / kcb: the k offset of each piece's chunk in its tile
  const bool ktail = ((kend - kbeg) % BKt) != 0;
  int kca[G::AI], kcb[G::BI];
#pragma unroll
  for (int i = 0; i < G::AI; ++i) kca[i] = AK ? pipe_kchunk<BKt>(((i * G::NW + wid) % G::AP) * 64 + lane) : 0;
#pragma unroll
  for (int i = 0; i < G::BI; ++i) kcb[i] = BKM ? pipe_kchunk<BKt>(((i * G::NW + wid) % G::BP) * 64 + lane) : 0;
  // this wave's DMA pieces per stage (all waves alike unless the piece counts do not divide evenly)
  const int per_w = G::EVEN ? G::AI + G::BI
                            : (G::AP / G::NW + (wid < G::AP % G::NW)) + (G::BP / G::NW + (wid < G::BP % G::NW));
  const unsigned stepa = AK ? BKt * 2 : (unsigned)(BKt * oa.ld * 2);
  const unsigned stepb = BKM ? BKt * 2 : (unsigned)(BKt * ob.ld * 2);
  char* const sca = lds + G::LDS;        // MX: the tile's A / B block-scale rows
  char* const scb = sca + BMt * MXK;
  if constexpr (MXK > 0) {
    const int mk = p.mxk;
    const __amdgpu_buffer_rsrc_t rsa = mx_rsrc(p.mxa + (long)m0 * mk, (long)(p.M - m0) * mk);
    const __amdgpu_buffer_rsrc_t rsb = mx_rsrc(p.mxb + (long)n0 * mk, (long)(p.N - n0) * mk);
    const int pa = (BMt * mk + 1023) / 1024, pb = (BNt * mk + 1023) / 1024;
    for (int q = wid; q < pa + pb; q += NWV) {   // (rows past M / N read zero through the range check)
      if (q < pa) dma16(rsa, sca + 1024 * q, (unsigned)(1024 * q + 16 * lane));
      else dma16(rsb, scb + 1024 * (q - pa), (unsigned)(1024 * (q - pa) + 16 * lane));
    }
  }

  auto issue = [&](int kt) {
    char* sa = lds + (kt % NST) * G::STAGE;
    char* sb = sa + G::ABYTES;
    if constexpr (GA) {
      const int k0 = kbeg + kt * BKt, ti = k0 / ga.Ck, c0 = k0 - ti * ga.Ck;
      const int di = ga.di[ti], dj = ga.dj[ti];
      const unsigned shift = (unsigned)((ga.dR[ti] * ga.Cr + c0) * 2);   // mod 2^32: negative row shifts wrap
#pragma unroll
      for (int i = 0; i < G::AI; ++i) {
        const int ii = gi[i] - di, jj = gj[i] - dj;
        const bool ok = ii >= 0 && jj >= 0 && ii < ga.Ilim && jj < ga.Jlim;
        dma16(ra, sa + (i * G::NW + wid) * 1024, ok ? offa[i] + shift : 0xFFFFFF00u);
      }
    } else if (ktail && kt == nk - 1) {   // wave-uniform: the last, partial K tile
      const int lim = kend - kbeg - kt * BKt;
#pragma unroll
      for (int i = 0; i < G::AI; ++i)
        if (G::EVEN || i * G::NW + wid < G::AP)
          dma16(ra, sa + (i * G::NW + wid) * 1024, !AK || kca[i] < lim ? offa[i] + kt * stepa : 0xFFFFFF00u);
#pragma unroll
      for (int i = 0; i < G::BI; ++i)
        if (G::EVEN || i * G::NW + wid < G::BP)
          dma16(rb, sb + (i * G::NW + wid) * 1024, !BKM || kcb[i] < lim ? offb[i] + kt * stepb : 0xFFFFFF00u);
      return;
    } else {
#pragma unroll
      for (int i = 0; i < G::AI; ++i)
        if (G::EVEN || i * G::NW + wid < G::AP) dma16(ra, sa + (i * G::NW + wid) * 1024, offa[i] + kt * stepa);
    }
#pragma unroll
    for (int i = 0; i < G::BI; ++i)
      if (G::EVEN || i * G::NW + wid < G::BP) dma16(rb, sb + (i * G::NW + wid) * 1024, offb[i] + kt * stepb);
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x16){0};
  f32x4 acc4[M16 ? 2 * FM : 1][M16 ? 2 * FN : 1];
#pragma unroll
  for (int i = 0; i < (M16 ? 2 * FM : 1); ++i)
#pragma unroll
    for (int j = 0; j < (M16 ? 2 * FN : 1); ++j) acc4[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // bias gradient of a weight-gradient GEMM: column sums of the staged MN-major A tile ([k][BMt],
  // chunk c of k-row k at slot c ^ 4(k&3)); thread = one 8-column chunk x every RGth k-row
  constexpr int ACH = BMt / 8, RG = G::NTt / ACH;
  const bool acs = !AK && p.acs_slab != nullptr && tn == 0;
  float csum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int acs_c = tid % ACH, acs_r = tid / ACH;

#pragma unroll
  for (int s = 0; s < NST - 1; ++s)
    if (s < nk) issue(s);
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt has landed once only the younger issued stages are outstanding
    const int younger = min(NST - 2, nk - 1 - kt);
    if constexpr (G::EVEN) wait_stages<G::AI + G::BI>(younger);
    else wait_vm_rt(per_w * younger);
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (kt + NST - 1 < nk) issue(kt + NST - 1);   // refills the stage every wave finished reading at kt-1
    const char* sa = lds + (kt % NST) * G::STAGE;
    const char* sb = sa + G::ABYTES;
    if constexpr (F8) {
      typedef KmSw<BKt> S;
      typedef int i32x8 __attribute__((ext_vector_type(8)));
      constexpr int KS8 = BKt / 32;    // 64-fp8 k-steps per stage
      i32x8 a8[KS8][FM], b8[KS8][FN];
      unsigned sA[FM], sB[FN];           // MX: this stage's block scales of each fragment row
      if constexpr (MXK > 0) {
        const int mk = p.mxk, kb0 = kt * (BKt / 16);
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const char* a = sca + (wm * FM * 32 + i * 32 + (lane & 31)) * mk + kb0;
          sA[i] = BKt == 64 ? *reinterpret_cast<const unsigned*>(a) : *reinterpret_cast<const unsigned short*>(a);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const char* b = scb + (wn * FN * 32 + j * 32 + (lane & 31)) * mk + kb0;
          sB[j] = BKt == 64 ? *reinterpret_cast<const unsigned*>(b) : *reinterpret_cast<const unsigned short*>(b);
        }
      }
      // v_mfma_scale_f32_32x32x64_f8f6f4's k order (measured, benchmarks/mx_probe.hip): lane (r, h) bytes 0-15 hold
      // k = 16h .. 16h+15 and bytes 16-31 k = 32+16h .. 32+16h+15 of the 64-step; the scale of lane r covers k 0..31
      // (bytes 0-15 of both halves), that of lane r+32 k 32..63 -- so lane (r, h) loads 16-B chunks h and h + 2 of
      // the step, and MX block 2q + h's scale sits in lane (r, h)
      auto frag8 = [&](const char* img, int row0, int q) {
        const int r = row0 + (lane & 31), c = 4 * q + (lane >> 5);
        const uint4 lo = *reinterpret_cast<const uint4*>(img + r * S::RB + 16 * S::slot(r, c));
        const uint4 hi = *reinterpret_cast<const uint4*>(img + r * S::RB + 16 * S::slot(r, c + 2));
        i32x8 v;
        v[0] = (int)lo.x; v[1] = (int)lo.y; v[2] = (int)lo.z; v[3] = (int)lo.w;
        v[4] = (int)hi.x; v[5] = (int)hi.y; v[6] = (int)hi.z; v[7] = (int)hi.w;
        return v;
      };
#pragma unroll
      for (int q = 0; q < KS8; ++q) {
#pragma unroll
        for (int j = 0; j < FN; ++j) b8[q][j] = frag8(sb, wn * FN * 32 + j * 32, q);
#pragma unroll
        for (int i = 0; i < FM; ++i) a8[q][i] = frag8(sa, wm * FM * 32 + i * 32, q);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < KS8; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const int sh = 8 * (2 * q + (lane >> 5));
            const int sa = MXK > 0 ? (int)(sA[i] >> sh) : 127, sb = MXK > 0 ? (int)(sB[j] >> sh) : 127;
            acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8[q][i], b8[q][j], acc[i][j], 0, 0, 0,
                                                                        sa, 0, sb);
          }
      continue;
    }
    if constexpr (M16) {
      constexpr int KS32 = BKt / 32;
      bf16x8 a16[KS32][2 * FM], b16[KS32][2 * FN];
#pragma unroll
      for (int q = 0; q < KS32; ++q) {
#pragma unroll
        for (int j = 0; j < 2 * FN; ++j) b16[q][j] = pipe_frag16k<BKt>(sb, wn * FN * 32 + 16 * j, 32 * q, lane);
#pragma unroll
        for (int i = 0; i < 2 * FM; ++i) a16[q][i] = pipe_frag16k<BKt>(sa, wm * FM * 32 + 16 * i, 32 * q, lane);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < KS32; ++q)
#pragma unroll
        for (int i = 0; i < 2 * FM; ++i)
#pragma unroll
          for (int j = 0; j < 2 * FN; ++j)
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a16[q][i], b16[q][j], acc4[i][j], 0, 0, 0);
      continue;
    }
    // every fragment of the stage is read up front (the stage is complete after the barrier), so the
    // LDS latency of later k-steps hides under the MFMAs of earlier ones
    constexpr int KST = BKt / 16;
    bf16x8 af[KST][FM], bfr[KST][FN];
#pragma unroll
    for (int q = 0; q < KST; ++q) {
#pragma unroll
      for (int j = 0; j < FN; ++j) bfr[q][j] = pipe_frag<BKM, BNt, BKt>(sb, wn * FN * 32 + j * 32, 16 * q, lane);
#pragma unroll
      for (int i = 0; i < FM; ++i) af[q][i] = pipe_frag<AK, BMt, BKt>(sa, wm * FM * 32 + i * 32, 16 * q, lane);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs (the scheduler would sink them)
#pragma unroll
    for (int q = 0; q < KST; ++q)
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[q][i], bfr[q][j], acc[i][j], 0, 0, 0);
    if constexpr (!AK) {
      if (acs) {
#pragma unroll
        for (int kq = 0; kq < BKt / RG; ++kq) {
          const int k = acs_r + kq * RG;
          const bf16x8 v = *reinterpret_cast<const bf16x8*>(sa + k * (BMt * 2) + 16 * (acs_c ^ (4 * (k & 3))));
#pragma unroll
          for (int e = 0; e < 8; ++e) csum[e] += (float)v[e];
        }
      }
    }
  }
  if constexpr (!AK) {
    if (acs) {   // combine the RG row groups in LDS (every wave is past its last ring read after this barrier)
      __syncthreads();
      float* red = reinterpret_cast<float*>(lds);
#pragma unroll
      for (int e = 0; e < 8; ++e) red[acs_r * BMt + acs_c * 8 + e] = csum[e];
      __syncthreads();
      if (tid < BMt && m0 + tid < p.M) {
        float t = 0.f;
        for (int g = 0; g < RG; ++g) t += red[g * BMt + tid];
        p.acs_slab[(long)zz * p.M + m0 + tid] = t;
      }
    }
  }
  if constexpr (M16) {   // pack the 16x16 blocks into the 32x32 accumulator registers (accr / accc<true>)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = acc4[2 * i + ((r >> 3) & 1)][2 * j + ((r >> 2) & 1)][r & 3];
  }
  if (p.dbg & 1) {   // timing experiment: keep the accumulators live, store nothing
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) t += acc[i][j][r];
    if (t == -1234.5f) reinterpret_cast<float*>(p.C)[tid] = t;
    return;
  }
  if constexpr (!GROUP) gemm_drop_prep(p);
  __syncthreads();   // every wave done with the ring (no DMA outstanding) -> reuse it for the epilogue
  if constexpr (F8) {   // per-tensor dequantisation of the fp8 operands (device scalars)
    if (p.alpha_a) p.alpha *= p.alpha_a[0];
    if (p.alpha_b) p.alpha *= p.alpha_b[0];
  }
  tile_epilogue_g<FM, FN, WM, WN, G::NTt, BNt, M16, 128, EK>(p, acc, reinterpret_cast<float*>(lds), z, zz, m0, n0, wm, wn, lane,
                                                      tid);
  probe_end(p.probe);
}

}  // namespace
