// gemm_params.h -- what every GEMM kernel family shares: the kernel parameter block (GemmP), the operand loaders
// of the register-staged kernels (StridedOp, the conv2 im2col gathers), the operand descriptors of the LDS-DMA
// kernels (PipeOp, GatherA), the bf16 LDS geometry, the XCD-aware tile order and the MFMA fragment read.
// Everything lives in an unnamed namespace: the kernels' device symbols carry these type names, and each kernel
// family is instantiated by exactly one translation unit ("GEMM source map").
//
// Tile: 128x128 output per 256-thread workgroup (4 waves as 2x2, 64x64 per wave =
// 2x2 MFMA 32x32 tiles).  bf16 operands: v_mfma_f32_32x32x16_bf16, BK = 32.  fp32 operands:
// v_mfma_f32_32x32x2_f32 (exact f32 products, used for the fp32 parity mode), BK = 16.
// Operand layouts (per operand, compile-time): K-major (k contiguous, e.g. X and W in the
// forward pass) is staged row-wise and read with ds_read_b128; MN-major (m/n contiguous, e.g.
// the token dimension in weight-gradient GEMMs) is staged as [k][m] and read with the gfx950
// ds_read_b64_tr_b16 transposed LDS read, so no operand is ever transposed in HBM.
// Operands are "loader" functors: a plain strided matrix, or an on-the-fly im2col gather for
// the 3x3/stride-2 convolution (forward, weight-grad and data-grad).
// Global->LDS staging goes through registers with one-tile-ahead prefetch and a double-buffered
// LDS ring (one barrier per K tile).
#pragma once
#include "cfm_common.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace {

constexpr int BM = 128, BN = 128, NT = 256;

struct GemmP {
  int M, N, K;
  void* C; long ldc, sc; int dtc;
  float alpha;
  const float* bias;
  int act, act_grad;
  void* pre; int dtpre;
  float drop_p; uint64_t seed, doff;
  const uint64_t* salt;   // bound dropout step counter (cfm_rng_bind) or nullptr
  float out_scale;
  const void* res; long ldr; int dtr;
  int split_k, k_per_split;
  int vec_c;   // 8-wide epilogue legal: C/pre/residual/bias 16-B aligned rows
  float* slab; // split-K slabs [batch*split][M][N] (nullptr: atomics into C)
  // output row remap for the conv2 data-grad parity classes: row m = (b, i, j) of the class
  // -> dh1 row (b, 2i+pf, 2j+pt)
  int cmap, cm_F1c, cm_T1c, cm_pf, cm_pt, cm_F1, cm_T1;
  int dbg;     // timing experiments only (1: CFM_GEMM_MODE_SKIP_STORES, 2: GENERIC_DROPOUT, 4: SKIP_MAINLOOP)
  unsigned long long* probe;   // optional timing slot (cfm_gemm_desc.probe)
  float* acs_slab;             // A column-sum partials [split][M] (cfm_gemm_desc.a_colsum) or nullptr
  const bf16* rd_with;         // per-64-column-group row dots with C (cfm_gemm_desc.rowdot_*) or nullptr
  float* rd_out;
  int rd_T;
  const float* alpha_a;        // fp8 operands: per-tensor dequantisation scales (device) or nullptr
  const float* alpha_b;
  uint32_t dkey0, dthr;        // dropout constants hoisted out of the epilogue (gemm_drop_prep)
  float dkeep;
  int efast;                   // staged-epilogue fast path (epi_fast_kind; 0: the generic epilogue_store8 rows)
  const uint8_t* mxa;          // MX fp8 operands (cfm_gemm_desc.mx_a / mx_b): e8m0 block scales [rows][mxk]
  const uint8_t* mxb;
  int mxk;                     // blocks of 32 fp8 per row (K / 32)
  uint8_t* mxo8;               // EF_BF16_SILU_MX: the MX e4m3 copy of the bf16 C (cfm_gemm_desc.mx_out)
  uint8_t* mxos;               //   and its e8m0 block scales [M][N/32]
};

// salt the dropout seed and hoist the per-launch constants (hash key of the low 2^33 index range,
// threshold, keep scale -- the latter an IEEE division) out of the per-8-element epilogue
__device__ __forceinline__ void gemm_drop_prep(GemmP& p) {
  if (p.drop_p > 0.f) {
    p.seed = salted_seed(p.seed, p.salt);
    p.dkey0 = drop_key(p.seed, 0);
    p.dthr = drop_thr(p.drop_p);
    p.dkeep = drop_keep_scale(p.dthr);
  }
}

__device__ __forceinline__ long out_row(const GemmP& p, int m) {
  if (!p.cmap) return m;
  const int j = m % p.cm_T1c, r = m / p.cm_T1c, i = r % p.cm_F1c, b = r / p.cm_F1c;
  return ((long)b * p.cm_F1 + 2 * i + p.cm_pf) * p.cm_T1 + 2 * j + p.cm_pt;
}

template <typename T> struct VecOf;
template <> struct VecOf<bf16> { typedef uint4 type; static constexpr int W = 8; };
template <> struct VecOf<float> { typedef float4 type; static constexpr int W = 4; };

// element-wise fallback: W consecutive elements p[0..W), zero past `n_ok`
template <typename T>
__device__ __forceinline__ typename VecOf<T>::type ld_partial(const T* p, int n_ok) {
  typedef typename VecOf<T>::type V;
  constexpr int W = VecOf<T>::W;
  if constexpr (W == 8) {
    unsigned short t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = e < n_ok ? reinterpret_cast<const unsigned short*>(p)[e] : 0;
    V r;
    r.x = t[0] | (t[1] << 16); r.y = t[2] | (t[3] << 16); r.z = t[4] | (t[5] << 16); r.w = t[6] | (t[7] << 16);
    return r;
  } else {
    float t[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = e < n_ok ? p[e] : 0.f;
    return make_float4(t[0], t[1], t[2], t[3]);
  }
}
template <typename T> __device__ __forceinline__ typename VecOf<T>::type vzero() {
  typename VecOf<T>::type r;
  if constexpr (VecOf<T>::W == 8) r = make_uint4(0, 0, 0, 0); else r = make_float4(0.f, 0.f, 0.f, 0.f);
  return r;
}

// Plain strided operand: element (outer, inner) at base[outer*ld + inner] (+ batch stride)
template <typename T> struct StridedOp {
  const T* base; long ld; long bstride; bool vec;
  __device__ __forceinline__ void batch(int z) { base += (long)z * bstride; }
  __device__ __forceinline__ typename VecOf<T>::type load(int outer, int inner, int outer_lim, int inner_lim) const {
    constexpr int W = VecOf<T>::W;
    if (outer >= outer_lim || inner >= inner_lim) return vzero<T>();
    const T* p = base + (long)outer * ld + inner;
    if (vec && inner + W <= inner_lim) return *reinterpret_cast<const typename VecOf<T>::type*>(p);
    return ld_partial<T>(p, inner_lim - inner);
  }
};

// conv2 geometry: h1 NHWC (B, F1, T1, C1); output rows m = (b, t2, f2); taps (kh, kw) 3x3 stride 2
struct Conv2Geo { int B, F1, T1, C1, F2, T2, C2; };

// forward A (K-major): A(m, k=(kh,kw,c1)) = h1[b, 2f2+kh, 2t2+kw, c1]
template <typename T> struct Conv2FwdA {
  const T* h1; Conv2Geo g;
  __device__ __forceinline__ void batch(int) {}
  __device__ __forceinline__ typename VecOf<T>::type load(int m, int k, int m_lim, int k_lim) const {
    if (m >= m_lim || k >= k_lim) return vzero<T>();
    const int f2 = m % g.F2, r = m / g.F2, t2 = r % g.T2, b = r / g.T2;
    const int tap = k / g.C1, c1 = k % g.C1, kh = tap / 3, kw = tap % 3;
    const T* p = h1 + (((long)b * g.F1 + 2 * f2 + kh) * g.T1 + 2 * t2 + kw) * g.C1 + c1;
    return *reinterpret_cast<const typename VecOf<T>::type*>(p);
  }
};
// weight-grad B (MN-major): B(n=(kh,kw,c1), k=m) = h1[b(m), 2f2+kh, 2t2+kw, c1]
template <typename T> struct Conv2WgradB {
  const T* h1; Conv2Geo g;
  __device__ __forceinline__ void batch(int) {}
  __device__ __forceinline__ typename VecOf<T>::type load(int m, int n, int m_lim, int n_lim) const {
    if (m >= m_lim || n >= n_lim) return vzero<T>();
    const int f2 = m % g.F2, r = m / g.F2, t2 = r % g.T2, b = r / g.T2;
    const int tap = n / g.C1, c1 = n % g.C1, kh = tap / 3, kw = tap % 3;
    const T* p = h1 + (((long)b * g.F1 + 2 * f2 + kh) * g.T1 + 2 * t2 + kw) * g.C1 + c1;
    return *reinterpret_cast<const typename VecOf<T>::type*>(p);
  }
};
// data-grad, one stride-2 parity class (pf, pt) of input pixels at a time: pixel (f1, t1) with
// f1 = 2i + pf, t1 = 2j + pt only receives the taps kh = pf (+2), kw = pt (+2), i.e. 4 / 2 / 2 / 1
// taps for the four classes instead of 9 zero-padded ones (4x fewer MACs than a plain im2col).
struct Conv2Class {
  int pf, pt, F1c, T1c, ntaps;
  int kh[4], kw[4];
};
// A (K-major): rows (b, i, j) of the class, k = (tap, c2) -> dh2[b, t2 = (t1-kw)/2, f2 = (f1-kh)/2, c2]
template <typename T> struct Conv2DgradA {
  const T* dh2; Conv2Geo g; Conv2Class c;
  __device__ __forceinline__ void batch(int) {}
  __device__ __forceinline__ typename VecOf<T>::type load(int pr, int k, int p_lim, int k_lim) const {
    if (pr >= p_lim || k >= k_lim) return vzero<T>();
    const int j = pr % c.T1c, r = pr / c.T1c, i = r % c.F1c, b = r / c.F1c;
    const int ti = k / g.C2, c2 = k % g.C2;
    const int f2 = (2 * i + c.pf - c.kh[ti]) >> 1, t2 = (2 * j + c.pt - c.kw[ti]) >> 1;
    if (f2 < 0 || t2 < 0 || f2 >= g.F2 || t2 >= g.T2) return vzero<T>();
    const T* p = dh2 + (((long)b * g.T2 + t2) * g.F2 + f2) * g.C2 + c2;
    return *reinterpret_cast<const typename VecOf<T>::type*>(p);
  }
};
// B (MN-major): B(n = c1, k = (tap, c2)) = w2r[c2][kh][kw][c1]
template <typename T> struct Conv2DgradB {
  const T* w2r; Conv2Geo g; Conv2Class c;
  __device__ __forceinline__ void batch(int) {}
  __device__ __forceinline__ typename VecOf<T>::type load(int k, int n, int k_lim, int n_lim) const {
    if (k >= k_lim || n >= n_lim) return vzero<T>();
    const int ti = k / g.C2, c2 = k % g.C2;
    const T* p = w2r + ((long)c2 * 9 + c.kh[ti] * 3 + c.kw[ti]) * g.C1 + n;
    return *reinterpret_cast<const typename VecOf<T>::type*>(p);
  }
};

// bf16 LDS geometry (elements)
constexpr int BK16 = 64;
constexpr int KM_STRIDE = BK16 + 8;        // K-major tile [128][72]: 144-B rows, conflict-free b128
constexpr int MN_STRIDE = 128 + 32;        // MN-major tile [64][160]: 320-B rows, conflict-free tr16
constexpr int TILE16 = (128 * KM_STRIDE > BK16 * MN_STRIDE) ? 128 * KM_STRIDE : BK16 * MN_STRIDE;  // 20 KiB
constexpr int KV16 = BK16 / 8;             // vectors per K-major row (8)

// XCD-aware tile order: blocks b and b+8 share an XCD under round-robin dispatch, so hand each
// XCD a contiguous run of (row-major) tiles: neighbouring tiles then share their A panel in that
// XCD's L2 (bijective for any tile count; speed only, never correctness).
__device__ __forceinline__ void xcd_tile(int& tm, int& tn) {
  const int gx = gridDim.x, nwg = gx * gridDim.y;
  const int L = blockIdx.y * gx + blockIdx.x;
  int id = L;
  if (nwg > 8) {
    const int xcd = L & 7, q = nwg >> 3, r = nwg & 7;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
  }
  tm = id / gx;
  tn = id % gx;
}

// The same over the whole 3-D grid (z = batch x split-K slice, slowest): each XCD gets a contiguous
// run of (slice, tile) pairs, i.e. whole K slices -- the 4-8 tiles that re-read one slice's
// operand panels then do so from that XCD's L2 instead of every XCD fetching every panel.
__device__ __forceinline__ void xcd_tile3(int& tm, int& tn, int& zz) {
  const int gx = gridDim.x, gxy = gx * gridDim.y, nwg = gxy * gridDim.z;
  const int L = (blockIdx.z * gridDim.y + blockIdx.y) * gx + blockIdx.x;
  int id = L;
  if (nwg > 8) {
    const int xcd = L & 7, q = nwg >> 3, r = nwg & 7;
    id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
  }
  zz = id / gxy;
  const int t = id % gxy;
  tm = t / gx;
  tn = t % gx;
}

// fp32 LDS geometry: both operands stored [BK][128+4] (k-rows)
constexpr int BK32 = 16;

// Read one 32x32x16 operand fragment (8 bf16, natural k order) from a staged tile.
// MNS: row stride of the MN-major image (rows + 32 elements: 64 mod 256 bytes -> conflict-free tr16)
template <bool KMAJOR, int MNS = MN_STRIDE>
__device__ __forceinline__ bf16x8 frag16(const bf16* tile, int row0, int kk, int lane) {
  if constexpr (KMAJOR) {
    const bf16* p = tile + (row0 + (lane & 31)) * KM_STRIDE + kk + 8 * (lane >> 5);
    return *reinterpret_cast<const bf16x8*>(p);
  } else {
    const int h = lane >> 5, g1 = (lane >> 4) & 1, q = (lane & 15) >> 2, p4 = lane & 3;
    const bf16* base = tile + (kk + 8 * h + q) * MNS + row0 + 16 * g1 + 4 * p4;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(base + 4 * MNS));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  }
}


struct PipeOp {
  const bf16* base;
  long ld, bstride;
  int lim;          // valid rows (K-major) / columns (MN-major) of the M or N dimension
  unsigned bytes;   // extent of one batch for the range check
};

// Gathered K-major A operand (implicit-GEMM convolutions): GEMM row m decomposes as
// j = m % Jn, i = (m / Jn) % In, b = m / (Jn * In); its source row (of Cr channels) for tap ti is
// b * sB + i * sI + j * sJ + dR[ti], valid iff 0 <= i - di[ti] < Ilim and 0 <= j - dj[ti] < Jlim
// (invalid rows read zero through an out-of-range buffer offset).  k = (ti, c) with Ck channels per
// tap, so each BKt-deep K tile lies inside one tap (Ck % BKt == 0).
//   conv2 forward:        rows (b, t2, f2) of h1 taps: i = t2, j = f2, row = (b F1 + 2 f2 + kh) T1 + 2 t2 + kw
//   conv2 data-gradient:  rows (b, i, j) of a parity class, source dh2 (b, t2 = j - dj, f2 = i - di)
struct GatherA {
  int Jn, In;
  long sB;
  int sI, sJ, Cr, Ck, Ilim, Jlim;
  int di[9], dj[9], dR[9];
  const void* group_tab;   // grouped launch (GROUP kernels): device WgTask table, one task per GEMM
  int group_n;
  const unsigned* group_sched;   // planned grouped launch: one word per workgroup (cfm_wgrad_group_plan) or nullptr
};

GemmP plain_params(int M, int N, int K, void* C, long ldc, int dtc) {
  GemmP p{};
  p.M = M; p.N = N; p.K = K;
  p.C = C; p.ldc = ldc; p.sc = 0; p.dtc = dtc;
  p.alpha = 1.f; p.out_scale = 1.f;
  p.split_k = 1; p.k_per_split = K;
  return p;
}

int vec_epilogue_ok(const GemmP& p) {
  auto al = [](const void* q) { return q == nullptr || (uintptr_t)q % 16 == 0; };
  return (p.ldc % 8 == 0) && (p.sc % 8 == 0) && al(p.C) && al(p.pre) && al(p.bias) &&
         (p.res == nullptr || (al(p.res) && p.ldr % 8 == 0));
}

int split_k_for(const GemmP& p, int bk) {
  return ((p.K + p.split_k - 1) / p.split_k + bk - 1) / bk * bk;
}

// elements one batch of a strided operand spans: (rows - 1) * ld + row length.  Rows may overlap (ld < row
// length: the folded front-end's windowed view of the packed mels, frontfold.hip); reads past the extent
// return zero through the buffer range check
long pipe_extent(int kmajor, long mn, long K, long ld) {
  return kmajor ? (mn - 1) * ld + K : (K - 1) * ld + mn;
}

// the LDS-DMA view of a plain strided bf16 operand of cfm_gemm (mn: its M or N)
inline PipeOp pipe_op(const void* base, int kmajor, long mn, long K, long ld, long bstride) {
  return PipeOp{(const bf16*)base, ld, bstride, (int)mn, (unsigned)(pipe_extent(kmajor, mn, K, ld) * 2)};
}

// a strided operand's rows can be read as whole 16-B vectors (bf16: 8 elements, fp32: 4)
inline bool strided_vec_ok(const void* base, long ld, long bstride, bool bf) {
  const int vlen = bf ? 8 : 4;
  return ((uintptr_t)base % 16 == 0) && (ld % vlen == 0) && (bstride % vlen == 0);
}

}  // namespace
