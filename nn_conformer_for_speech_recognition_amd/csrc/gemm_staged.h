// gemm_staged.h -- the register-staged kernels (any loader type: strided or the conv2 gathers): gemm_bf16_kernel,
// gemm_f32_kernel, and their launch (launch_typed).
#pragma once
#include "gemm_epilogue.h"
#include "gemm_launch.h"

#include <type_traits>

namespace {

// ---------------------------------------------------------------- bf16 kernel
// BMt x 128 output tile, BMt*2 threads (BMt/64 x 2 waves of 64x64): BMt = 128 (80 KiB LDS, 2
// workgroups/CU) for narrow or split-K shapes, BMt = 256 (112 KiB, 1 workgroup/CU of 8 waves: 1.5x
// the FLOP per staged byte) for the wide token-major GEMMs.
template <int BMt>
struct Geo16 {
  static constexpr int NTt = BMt * 2;
  static constexpr int NVA = BMt * BK16 / 8 / NTt;      // A vectors per thread (4)
  static constexpr int NVB = BN * BK16 / 8 / NTt;       // B vectors per thread (4 or 2)
  static constexpr int MNSA = BMt + 32;                  // MN-major A row stride
  static constexpr int TILEA = (BMt * KM_STRIDE > BK16 * MNSA) ? BMt * KM_STRIDE : BK16 * MNSA;
  static constexpr int TILEB = TILE16;
  static constexpr int LDS = 2 * (TILEA + TILEB);        // elements
};

template <int BMt>
__device__ __forceinline__ void tile_epilogue(const GemmP& p, f32x16 (&acc)[2][2], float* st, int z, int zs, int m0,
                                              int n0, int wm, int wn, int lane, int tid);

template <int BMt, bool AK, bool BKM, class OA, class OB>
__global__ __launch_bounds__(BMt * 2) void gemm_bf16_kernel(GemmP p, OA oa, OB ob) {
  typedef Geo16<BMt> G;
  probe_begin(p.probe);
  gemm_drop_prep(p);
  constexpr int NTt = G::NTt, NVA = G::NVA, NVB = G::NVB, TILEA = G::TILEA;
  __shared__ __attribute__((aligned(16))) bf16 lds[G::LDS];   // [buf][A,B]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  int tm, tn;
  xcd_tile(tm, tn);
  const int m0 = tm * BMt, n0 = tn * BN;
  const int z = blockIdx.z / p.split_k, ks = blockIdx.z % p.split_k;
  oa.batch(z);
  ob.batch(z);
  const int kbeg = ks * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  const int nk = kend > kbeg ? (kend - kbeg + BK16 - 1) / BK16 : 0;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};

  constexpr int AV = BMt / 8;     // MN-major A: vectors per k-row
  uint4 ra[NVA], rb[NVB];
  auto gload = [&](int kt) {
    const int k0 = kbeg + kt * BK16;
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int v = tid + NTt * i;
      if constexpr (AK) ra[i] = oa.load(m0 + v / KV16, k0 + (v % KV16) * 8, p.M, kend);
      else ra[i] = oa.load(k0 + v / AV, m0 + (v % AV) * 8, kend, p.M);
    }
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int v = tid + NTt * i;
      if constexpr (BKM) rb[i] = ob.load(n0 + v / KV16, k0 + (v % KV16) * 8, p.N, kend);
      else rb[i] = ob.load(k0 + (v >> 4), n0 + (v & 15) * 8, kend, p.N);
    }
  };
  auto sstore = [&](int buf) {
    bf16* ta = lds + buf * (TILEA + TILE16);
    bf16* tb = ta + TILEA;
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int v = tid + NTt * i;
      bf16* da = AK ? ta + (v / KV16) * KM_STRIDE + (v % KV16) * 8 : ta + (v / AV) * G::MNSA + (v % AV) * 8;
      *reinterpret_cast<uint4*>(da) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int v = tid + NTt * i;
      bf16* db = BKM ? tb + (v / KV16) * KM_STRIDE + (v % KV16) * 8 : tb + (v >> 4) * MN_STRIDE + (v & 15) * 8;
      *reinterpret_cast<uint4*>(db) = rb[i];
    }
  };

  if (nk > 0) {
    gload(0);
    sstore(0);
    __syncthreads();
  }
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const bf16* ta = lds + cur * (TILEA + TILE16);
    const bf16* tb = ta + TILEA;
#pragma unroll
    for (int kk = 0; kk < BK16; kk += 16) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = frag16<AK, G::MNSA>(ta, wm * 64 + i * 32, kk, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = frag16<BKM>(tb, wn * 64 + j * 32, kk, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }

  tile_epilogue<BMt>(p, acc, reinterpret_cast<float*>(lds), z, blockIdx.z, m0, n0, wm, wn, lane, tid);
  probe_end(p.probe);
}

// Epilogue of one BMt x 128 tile (4-wave rows x 2-wave columns of 64x64 accumulators).  The
// caller guarantees every wave is done reading the staging LDS (`st`, >= 128 x EP_STRIDE floats).
template <int BMt>
__device__ __forceinline__ void tile_epilogue(const GemmP& p, f32x16 (&acc)[2][2], float* st, int z, int zs, int m0,
                                              int n0, int wm, int wn, int lane, int tid) {
  constexpr int NTt = BMt * 2;
  if (p.split_k > 1 && !p.slab) {
    // split-K partials: atomics straight from the accumulators (32 consecutive columns per
    // half-wave = two 128-B segments per instruction, the fast atomic shape)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int n = n0 + wn * 64 + j * 32 + (lane & 31);
          splitk_atomic_store(p, z, zs, m, n, acc[i][j][r]);
        }
    return;
  }
  // stage 128-row halves of the f32 tile in LDS, then every thread finishes 8 consecutive
  // columns of a row -> 16-B / 32-B vector stores.
#pragma unroll
  for (int hf = 0; hf < BMt / 128; ++hf) {
    if ((wm >> 1) == hf) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (wm & 1) * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int col = wn * 64 + j * 32 + (lane & 31);
            st[row * EP_STRIDE + col] = acc[i][j][r];
          }
    }
    __syncthreads();
#pragma unroll 2
    for (int it = 0; it < 128 * 16 / NTt; ++it) {
      const int row = it * (NTt / 16) + (tid >> 4), c8 = (tid & 15) * 8;
      const float4 lo = *reinterpret_cast<const float4*>(st + row * EP_STRIDE + c8);
      const float4 hi = *reinterpret_cast<const float4*>(st + row * EP_STRIDE + c8 + 4);
      float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      epilogue_store8(p, z, zs, m0 + 128 * hf + row, n0 + c8, v);
    }
    if (hf + 1 < BMt / 128) __syncthreads();
  }
}

// ---------------------------------------------------------------- fp32 kernel (exact-f32 MFMA)
// exact-f32 MFMA GEMM (v_mfma_f32_32x32x2f32), register-staged K tiles of 16; TBM x TBM output tile, 4 waves
// of (TBM/2)^2: TBM = 128 for the large shapes, 64 (4x the workgroups) when the 128-tile grid would leave the
// chip mostly idle (the folded front-end's small contractions, frontfold.hip)
template <bool AK, bool BKM, class OA, class OB, int TBM = 128>
__global__ __launch_bounds__(NT) void gemm_f32_kernel(GemmP p, OA oa, OB ob) {
  constexpr int FR = TBM / 64, FS = TBM + 4, TT = BK32 * FS, NV = TBM / 64;
  gemm_drop_prep(p);
  __shared__ __attribute__((aligned(16))) float lds[4 * TT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int m0 = blockIdx.y * TBM, n0 = blockIdx.x * TBM;
  const int z = blockIdx.z / p.split_k, ks = blockIdx.z % p.split_k;
  oa.batch(z);
  ob.batch(z);
  const int kbeg = ks * p.k_per_split;
  const int kend = min(p.K, kbeg + p.k_per_split);
  const int nk = kend > kbeg ? (kend - kbeg + BK32 - 1) / BK32 : 0;

  f32x16 acc[FR][FR];
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) acc[i][j] = (f32x16){0};

  float4 ra[NV], rb[NV];
  // tile = 16 k x TBM rows = 4 * TBM float4
  auto gload = [&](int kt) {
    const int k0 = kbeg + kt * BK32;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + NT * i;
      if constexpr (AK) ra[i] = oa.load(m0 + (v >> 2), k0 + (v & 3) * 4, p.M, kend);
      else ra[i] = oa.load(k0 + v / (TBM / 4), m0 + (v % (TBM / 4)) * 4, kend, p.M);
      if constexpr (BKM) rb[i] = ob.load(n0 + (v >> 2), k0 + (v & 3) * 4, p.N, kend);
      else rb[i] = ob.load(k0 + v / (TBM / 4), n0 + (v % (TBM / 4)) * 4, kend, p.N);
    }
  };
  auto put = [&](float* t, bool kmaj, int v, float4 r) {
    if (kmaj) {
      const int row = v >> 2, kc = (v & 3) * 4;
      t[(kc + 0) * FS + row] = r.x;
      t[(kc + 1) * FS + row] = r.y;
      t[(kc + 2) * FS + row] = r.z;
      t[(kc + 3) * FS + row] = r.w;
    } else {
      *reinterpret_cast<float4*>(t + (v / (TBM / 4)) * FS + (v % (TBM / 4)) * 4) = r;
    }
  };
  auto sstore = [&](int buf) {
    float* ta = lds + buf * 2 * TT;
    float* tb = ta + TT;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + NT * i;
      put(ta, AK, v, ra[i]);
      put(tb, BKM, v, rb[i]);
    }
  };

  if (nk > 0) {
    gload(0);
    sstore(0);
    __syncthreads();
  }
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) gload(kt + 1);
    const float* ta = lds + cur * 2 * TT;
    const float* tb = ta + TT;
#pragma unroll
    for (int kk = 0; kk < BK32; kk += 2) {
      const int kr = kk + (lane >> 5);
      float af[FR], bfr[FR];
#pragma unroll
      for (int i = 0; i < FR; ++i) af[i] = ta[kr * FS + wm * (TBM / 2) + i * 32 + (lane & 31)];
#pragma unroll
      for (int j = 0; j < FR; ++j) bfr[j] = tb[kr * FS + wn * (TBM / 2) + j * 32 + (lane & 31)];
#pragma unroll
      for (int i = 0; i < FR; ++i)
#pragma unroll
        for (int j = 0; j < FR; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(cur ^ 1);
    __syncthreads();
  }
  // (the K loop ends on a barrier: the staging may reuse the operand LDS) one wave band (TBM / 2 rows) of the
  // f32 tile at a time through LDS, then 8-column chunks through epilogue_store8 (was a per-element epilogue the
  // compiler could not unroll, leaving the accumulators run-time indexed)
  static_assert((TBM / 2) * (TBM + 4) <= 4 * TT, "one band of the tile fits the staging");
  tile_epilogue_g<FR, FR, 2, 2, NT, TBM, false, TBM / 2>(p, acc, lds, z, blockIdx.z, m0, n0, wm, wn, lane, tid);
}

// The register-staged rule (bf: bf16 operands, else fp32): the variant, grid and block of a launch of p.
//   bf16: 256-row tiles when the grid still fills the chip (>= ~2 tiles per CU) without split-K, else 128-row ones
//   fp32: 64-row tiles when 128-row tiles would give fewer workgroups than CUs (small fp32 contractions)
inline int staged_choice(bool bf, const GemmP& p, int batch, int mode, cfm_gemm_choice* c) {
  int bm, bn = BN;
  if (bf) {
    const bool wide = p.split_k == 1 && (long)cdiv(p.M, 256) * cdiv(p.N, BN) * batch >= 512 &&
                      (mode & CFM_GEMM_MODE_STAGED256);
    c->variant = wide ? CFM_GEMM_V_STAGED_BF16_256 : CFM_GEMM_V_STAGED_BF16_128;
    bm = wide ? 256 : BM;
    c->block = 2 * bm;
  } else {
    const bool small = (long)cdiv(p.N, BN) * cdiv(p.M, BM) * batch * p.split_k < 256;
    c->variant = small ? CFM_GEMM_V_STAGED_F32_64 : CFM_GEMM_V_STAGED_F32_128;
    bm = bn = small ? 64 : BM;
    c->block = NT;
  }
  c->epilogue = EF_GENERIC;
  c->grid_x = cdiv(p.N, bn);
  c->grid_y = cdiv(p.M, bm);
  c->grid_z = batch * p.split_k;
  if (c->grid_y > 65535 || c->grid_z > 65535) return cfm::fail(CFM_ERR_SHAPE, "gemm: grid too large");
  return CFM_OK;
}

// launch the staged variant c chose (the loaders' element type says which pair of variants is meant)
template <bool AK, bool BKM, class OA, class OB>
void launch_staged(const cfm_gemm_choice& c, const GemmP& p, OA oa, OB ob, hipStream_t s) {
  const dim3 grid(c.grid_x, c.grid_y, c.grid_z), block(c.block);
  typedef decltype(oa.load(0, 0, 0, 0)) V;
  if constexpr (std::is_same<V, uint4>::value) {
    switch (c.variant) {
      case CFM_GEMM_V_STAGED_BF16_256:
        hipLaunchKernelGGL((gemm_bf16_kernel<256, AK, BKM, OA, OB>), grid, block, 0, s, p, oa, ob);
        break;
      default: hipLaunchKernelGGL((gemm_bf16_kernel<128, AK, BKM, OA, OB>), grid, block, 0, s, p, oa, ob); break;
    }
  } else {
    switch (c.variant) {
      case CFM_GEMM_V_STAGED_F32_64:
        hipLaunchKernelGGL((gemm_f32_kernel<AK, BKM, OA, OB, 64>), grid, block, 0, s, p, oa, ob);
        break;
      default: hipLaunchKernelGGL((gemm_f32_kernel<AK, BKM, OA, OB>), grid, block, 0, s, p, oa, ob); break;
    }
  }
}

// rule + launch for the callers outside cfm_gemm (the conv2 gather loaders)
template <bool AK, bool BKM, class OA, class OB>
int launch_typed(GemmP p, OA oa, OB ob, int batch, hipStream_t s) {
  p.vec_c = vec_epilogue_ok(p);
  cfm_gemm_choice c;
  const int rc = staged_choice(std::is_same<decltype(oa.load(0, 0, 0, 0)), uint4>::value, p, batch, cfm::g_gemm_mode, &c);
  if (rc != CFM_OK) return rc;
  launch_staged<AK, BKM>(c, p, oa, ob, s);
  return CFM_OK;
}

}  // namespace
