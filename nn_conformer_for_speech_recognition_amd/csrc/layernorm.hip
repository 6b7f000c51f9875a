// layernorm.hip — nn.LayerNorm(D) forward/backward over token rows (one wave per row).
//
// Used by every LayerNorm of the torchaudio ConformerLayer (ffn*.sequential.0,
// self_attn_layer_norm, conv_module.layer_norm, final_layer_norm).  The residual stream is
// fp32; the normalised output feeds the next GEMM in the compute dtype (bf16 or fp32).
// Backward fuses the residual-gradient add (dx = LN'(dy) + dres) and produces dgamma/dbeta
// through per-workgroup partial rows reduced by cfm::colreduce (deterministic, no atomics).
// Fast kernels (D = 64*V: one wave per row; other D % 8 == 0: a lane group per row): each lane owns contiguous
// features, so every load/store is a 16-B vector; other shapes/dtypes take the generic strided kernels.  Which one
// serves a call is ln_plan's answer (ln_plan.h); the entry points at the end of this file only act on it.
#include <type_traits>

#include "ln_plan.h"

namespace {
constexpr int MAXJ = LN_DMAX / 64;   // registers per lane that hold a row of the generic kernels

// ---------------------------------------------------------------- vector helpers (V per lane)
template <int V> __device__ __forceinline__ void ldv(const float* p, float (&o)[V]) {
  if constexpr (V % 4 == 0) {
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
      const float4 a = reinterpret_cast<const float4*>(p)[i];
      o[4 * i] = a.x; o[4 * i + 1] = a.y; o[4 * i + 2] = a.z; o[4 * i + 3] = a.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = p[i];
  }
}
template <int V> __device__ __forceinline__ void ldv(const bf16* p, float (&o)[V]) {
  if constexpr (V % 8 == 0) {
#pragma unroll
    for (int i = 0; i < V / 8; ++i) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, reinterpret_cast<const uint4*>(p)[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[8 * i + e] = (float)b[e];
    }
  } else if constexpr (V == 4) {
    const bf16x4 b = __builtin_bit_cast(bf16x4, *reinterpret_cast<const uint2*>(p));
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)b[e];
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = (float)p[i];
  }
}
template <int V> __device__ __forceinline__ void stv(float* p, const float (&v)[V]) {
  if constexpr (V % 4 == 0) {
#pragma unroll
    for (int i = 0; i < V / 4; ++i)
      reinterpret_cast<float4*>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = v[i];
  }
}
template <int V> __device__ __forceinline__ void stv(bf16* p, const float (&v)[V]) {
  if constexpr (V % 8 == 0) {
#pragma unroll
    for (int i = 0; i < V / 8; ++i) {
      bf16x8 b;
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = (bf16)v[8 * i + e];
      reinterpret_cast<uint4*>(p)[i] = __builtin_bit_cast(uint4, b);
    }
  } else if constexpr (V == 4) {
    bf16x4 b;
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = (bf16)v[e];
    *reinterpret_cast<uint2*>(p) = __builtin_bit_cast(uint2, b);
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = (bf16)v[i];
  }
}

// ---------------------------------------------------------------- optional operands of the fast kernels
// MX: a second output of the bf16 y -- its MX e4m3 copy (cfm_quant_mx's bytes and block scales of the bf16 values,
// for the fp8 forward GEMM that consumes it): the 32 / V lanes of a 32-feature block exchange their maxima by xor
// shuffles, so the copy costs its 1.03 bytes per element of stores instead of a separate 3-byte pass.
struct LnMx {
  uint8_t* y8;    // M x D e4m3
  uint8_t* s8;    // M x D/32 e8m0
};
__device__ __forceinline__ int ln_mx_k(float a) {   // = fp8.hip mx_k
  if (!(a > 0.f) || !(a < INFINITY)) return 0;
  int e;
  const float m = 2.f * frexpf(a, &e);
  const int k = (m <= 1.75f ? 8 : 7) - (e - 1);
  return k < 126 ? (k > -126 ? k : -126) : 126;
}
template <int V>
__device__ __forceinline__ void ln_store_mx(const LnMx& mx, long row, int D, int lane, const float (&v)[V]) {
  constexpr int LPB = 32 / V;       // lanes per 32-feature block
  float q[V], m = 0.f;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    q[i] = (float)(bf16)v[i];       // the bf16 value the GEMM would otherwise read
    m = fmaxf(m, fabsf(q[i]));
  }
#pragma unroll
  for (int o = 1; o < LPB; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const int k = ln_mx_k(m);
  const float sc = ldexpf(1.f, k);
  uint8_t* yp = mx.y8 + row * D + lane * V;
#pragma unroll
  for (int i = 0; i < V; i += 4) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q[i] * sc, q[i + 1] * sc, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q[i + 2] * sc, q[i + 3] * sc, w, true);
    *reinterpret_cast<int*>(yp + i) = w;
  }
  if (lane % LPB == 0) mx.s8[row * (D / 32) + lane / LPB] = (uint8_t)(127 - k);
}

// RS: the residual add of the module before this LayerNorm moved in here (cfm_layernorm_fwd_res): the row is
// x + delta (delta: that module's bf16 output -- bias, dropout and out_scale applied by its GEMM's epilogue), stored
// to xo (the fp32 residual stream the backward reads) and normalised.  The GEMM then writes 2 B per element instead of
// reading and writing the 4-B stream in an epilogue nothing overlaps; the bytes move into this streaming pass.
struct LnRes {
  const bf16* d;   // M x D delta
  float* xo;       // M x D: x + delta
};

// optional fused second output of the vectorised backward: g2 = bf16(dx * scale * dropout(p, seed))
struct LnDrop {
  void* g2;
  float scale, p;
  uint64_t seed;
  const uint64_t* salt;
};

// ---------------------------------------------------------------- row geometry
// How the 64 lanes of a wave share rows; the fast kernels are written once over a Geom.
//   F, RPW, LDSW   features per lane (contiguous: 16-B vectors), rows per wave and trip, columns of an LDS partial row
//   D(), inv_d()   the row width and 1 / D
//   col(), act()   the lane's first column; whether the lane holds columns of the row at all
//   sub()          the lane's row slot inside its wave (0 .. RPW - 1)
//   leader()       the lane that writes its row's statistics
//   heads()        the lanes whose column partials go to LDS, after fold() summed the wave's row slots into them
//   sum(v)         v summed over the lanes of the row
// RowWave<V>: one wave per row, D = 64 V at compile time, every lane active.  kEarlyExit: a forward wave whose rows
// all lie past M returns at once (its shuffles span one row, nobody waits for it).
template <int V> struct RowWave {
  static constexpr int F = V, RPW = 1, LDSW = 64 * V;
  static constexpr bool kWave = true, kEarlyExit = true, kReloadY = false;
  int lane;
  __device__ __forceinline__ RowWave(int lane_, int) : lane(lane_) {}
  __device__ __forceinline__ int D() const { return 64 * V; }
  __device__ __forceinline__ float inv_d() const { return 1.f / (64 * V); }
  __device__ __forceinline__ int col() const { return lane * V; }
  __device__ __forceinline__ bool act() const { return true; }
  __device__ __forceinline__ int sub() const { return 0; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ bool heads() const { return true; }
  __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
  __device__ __forceinline__ void fold(float (&)[F]) const {}
};
// RowGroup<G>: widths that are not 64 * V (Conformer-S: D = 144) on 16-B vectors: a group of G lanes owns one row, 8
// contiguous features per lane (lanes 8 j >= D idle), 64 / G rows per wave, the row sums over the group by xor
// shuffles inside it.  (The strided generic kernels below moved 4-B elements with per-element dtype branches: 20 us
// per D-144 backward where the bytes take ~5.)  The shuffles span the wave, so every group runs the same trips and
// rows past M are masked, never skipped.
// kReloadY: the pair forward's second LayerNorm takes y as the single forward does: 16-B loads (of this lane's own
// stores just above, from the cache -- still no pass over memory) through a pointer the compiler cannot trace back to
// them.  Fed from the registers it contracts (v - sum / D) and the squares differently per element than the single
// forward, and rstd2 comes out an ulp off the two-call path.
template <int G_> struct RowGroup {
  static constexpr int G = G_, F = 8, RPW = 64 / G_, LDSW = 8 * G_;
  static constexpr bool kWave = false, kEarlyExit = false, kReloadY = true;
  int lane, d, c;
  bool a;
  float invd;
  __device__ __forceinline__ RowGroup(int lane_, int D_)
      : lane(lane_), d(D_), c(8 * (lane_ % G_)), a(8 * (lane_ % G_) < D_), invd(1.f / (float)D_) {}
  __device__ __forceinline__ int D() const { return d; }
  __device__ __forceinline__ float inv_d() const { return invd; }
  __device__ __forceinline__ int col() const { return c; }
  __device__ __forceinline__ bool act() const { return a; }
  __device__ __forceinline__ int sub() const { return lane / G; }
  __device__ __forceinline__ bool leader() const { return lane % G == 0; }
  __device__ __forceinline__ bool heads() const { return lane < G; }
  __device__ __forceinline__ float sum(float v) const {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
  // the groups of a wave hold the same columns: xor over the group index bits
  __device__ __forceinline__ void fold(float (&p)[F]) const {
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
#pragma unroll
      for (int i = 0; i < F; ++i) p[i] += __shfl_xor(p[i], o, 64);
    }
  }
};

template <int N> __device__ __forceinline__ void ln_zero(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0.f;
}

// ---------------------------------------------------------------- shared row code
// What the kernels below share beyond the geometry.  How far this goes is set by the bit-identity the tests hold the
// kernels to (the pair against two calls, every kernel against its recorded outputs): the compiler decides per
// instruction mix which multiplies it packs in pairs and which it contracts into fmas, and moving a row's arithmetic
// behind a function boundary moves those decisions.  Measured on this file: the forward's statistics written as a
// function over the row (by reference or per element by value) contract the lane-group kernels' squares and shift
// rstd by an ulp; the pair backward on ln_bwd_stage / ln_write_partials fuses one more multiply-add per stage.  So
// ln_fwd and ln_fwd_pair spell the same row statements out (two copies, one per kernel, for both geometries), the
// pair backward kernels spell out their two stages and their write-out, and the helpers here serve the rest.

// the LN_FWD_ROWS rows of a lane from row0 on, zero where the lane or the row is outside
template <typename Geom, typename T>
__device__ __forceinline__ void ln_load_rows(const Geom& geo, const T* p, long row0, long M,
                                             float (&v)[LN_FWD_ROWS][Geom::F]) {
#pragma unroll
  for (int r = 0; r < LN_FWD_ROWS; ++r) {
    if (geo.act() && row0 + r < M) ldv<Geom::F>(p + (row0 + r) * geo.D() + geo.col(), v[r]);
    else ln_zero(v[r]);
  }
}
// One LayerNorm backward stage over a lane's features of one row.  d: the gradient of the stage's output, h: its
// normalised input, gam: its weight.  Adds the row to the column partials (pg += d h, pb += d), leaves g = d gam and
// the row means s1 = mean(g), s2 = mean(g h); the stage's input gradient is then ln_bwd_term per element.
template <typename Geom>
__device__ __forceinline__ void ln_bwd_stage(const Geom& geo, const float (&d)[Geom::F], const float (&h)[Geom::F],
                                             const float (&gam)[Geom::F], float (&g)[Geom::F], float (&pg)[Geom::F],
                                             float (&pb)[Geom::F], float& s1, float& s2) {
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int i = 0; i < Geom::F; ++i) {
    g[i] = d[i] * gam[i];
    pg[i] += d[i] * h[i];
    pb[i] += d[i];
    a += g[i];
    b += g[i] * h[i];
  }
  s1 = geo.sum(a) * geo.inv_d();
  s2 = geo.sum(b) * geo.inv_d();
}
__device__ __forceinline__ float ln_bwd_term(float rstd, float g, float s1, float h, float s2) {
  return rstd * (g - s1 - h * s2);
}

// g2 of a lane's 8 features at element idx: the next module's input gradient bf16(dx * scale * dropout mask), as
// cfm_scale_dropout makes it from dx.  Only the 8-feature geometries have it (ln_plan: g2_fused).
template <typename Geom>
__device__ __forceinline__ void ln_store_g2(const LnDrop& dr, long idx, const float (&o)[Geom::F]) {
  if constexpr (Geom::F == 8) {
    if (dr.g2) {
      float sc[8];
      if (dr.p > 0.f) dropout_scale8(dr.p, dr.seed, (uint64_t)idx, sc);
#pragma unroll
      for (int i = 0; i < 8; ++i) sc[i] = dr.p > 0.f ? dr.scale * sc[i] : dr.scale;
      float q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = o[i] * sc[i];
      st8_dyn(dr.g2, CFM_BF16, idx, q);
    }
  }
}

// A workgroup's column partials [pg | pb] (already folded) summed over its four waves through LDS into row `blk` of
// ws (2 D floats).
template <typename Geom>
__device__ __forceinline__ void ln_write_partials(const Geom& geo, float (&red)[4][2 * Geom::LDSW],
                                                  const float (&pg)[Geom::F], const float (&pb)[Geom::F], float* ws,
                                                  long blk) {
  const int D = geo.D(), c = geo.col(), wv = threadIdx.x >> 6;
  if (geo.heads()) {
#pragma unroll
    for (int i = 0; i < Geom::F; ++i) {
      red[wv][c + i] = pg[i];
      red[wv][Geom::LDSW + c + i] = pb[i];
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < 2 * D; q += 256) {
    const int k = q < D ? q : Geom::LDSW + (q - D);
    ws[blk * 2 * D + q] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
  }
}

// ---------------------------------------------------------------- forward
// LN_FWD_ROWS rows per wave (RowWave) or lane group (RowGroup).  MX (RowWave, V >= 4, bf16 y): also y's MX copy.
// RS: x + delta (cfm_layernorm_fwd_res).
template <typename Geom, typename TY, bool MX = false, typename TX = float, bool RS = false>
__global__ __launch_bounds__(256) void ln_fwd(const TX* __restrict__ x, const float* __restrict__ gamma,
                                              const float* __restrict__ beta, TY* __restrict__ y,
                                              float* __restrict__ mean_out, float* __restrict__ rstd_out, long M,
                                              int D_, float eps, LnMx mx, LnRes rs) {
  constexpr int F = Geom::F, R = LN_FWD_ROWS;
  const Geom geo(threadIdx.x & 63, D_);
  const int D = geo.D(), c = geo.col();
  const long row0 = (((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * Geom::RPW + geo.sub()) * R;
  if constexpr (Geom::kEarlyExit) {
    if (row0 >= M) return;
  }
  float v[R][F], g[F], b[F];
  [[maybe_unused]] float dl[RS ? R : 1][RS ? F : 1];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (geo.act() && row0 + r < M) {
      ldv<F>(x + (row0 + r) * D + c, v[r]);
      if constexpr (RS) ldv<F>(rs.d + (row0 + r) * D + c, dl[r]);
    } else {
#pragma unroll
      for (int i = 0; i < F; ++i) v[r][i] = 0.f;
      if constexpr (RS) {
#pragma unroll
        for (int i = 0; i < F; ++i) dl[r][i] = 0.f;
      }
    }
  }
  if constexpr (RS) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int i = 0; i < F; ++i) v[r][i] += dl[r][i];
      if (geo.act() && row0 + r < M) stv<F>(rs.xo + (row0 + r) * D + c, v[r]);
    }
  }
  if (geo.act()) {
    ldv<F>(gamma + c, g);
    ldv<F>(beta + c, b);
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < F; ++i) s += v[r][i];
    const float mean = geo.sum(s) * geo.inv_d();
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < F; ++i) {
      v[r][i] = geo.act() ? v[r][i] - mean : 0.f;
      q += v[r][i] * v[r][i];
    }
    const float rstd = rsqrtf(geo.sum(q) * geo.inv_d() + eps);
    if (row0 + r < M) {    // (RowWave: wave-uniform)
      if (geo.act()) {
#pragma unroll
        for (int i = 0; i < F; ++i) v[r][i] = v[r][i] * rstd * g[i] + b[i];
        stv<F>(y + (row0 + r) * D + c, v[r]);
      }
      if (geo.leader()) {
        mean_out[row0 + r] = mean;
        rstd_out[row0 + r] = rstd;
      }
      if constexpr (MX) ln_store_mx<F>(mx, row0 + r, D, geo.lane, v[r]);
    }
  }
}

// ---------------------------------------------------------------- LayerNorm pairs (layer boundary)
// final_layer_norm of encoder layer i followed directly by the ffn1 LayerNorm of layer i + 1: y = LN(x; g1, b1) is the
// fp32 stream between the layers, z = LN(y; g2, b2) the next layer's first GEMM operand.  One kernel per direction
// instead of two: the forward keeps y in registers (no fp32 write-then-read), the backward recomputes y from x and
// never materialises the gradient of y.  Each pass is ln_fwd's row arithmetic statement for statement, which is what
// makes y, z and the statistics equal the two-call path's bit for bit (a row past M stays all zero through both).
template <typename Geom, typename TZ>
__global__ __launch_bounds__(256) void ln_fwd_pair(const float* __restrict__ x, const float* __restrict__ gamma1,
                                                   const float* __restrict__ beta1, const float* __restrict__ gamma2,
                                                   const float* __restrict__ beta2, float* __restrict__ y,
                                                   TZ* __restrict__ z, float* __restrict__ mean1,
                                                   float* __restrict__ rstd1, float* __restrict__ mean2,
                                                   float* __restrict__ rstd2, long M, int D_, float eps) {
  constexpr int F = Geom::F, R = LN_FWD_ROWS;
  const Geom geo(threadIdx.x & 63, D_);
  const int D = geo.D(), c = geo.col();
  const long row0 = (((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * Geom::RPW + geo.sub()) * R;
  if constexpr (Geom::kEarlyExit) {
    if (row0 >= M) return;
  }
  float v[R][F], g[F], b[F];
  ln_load_rows(geo, x, row0, M, v);
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if constexpr (Geom::kReloadY) {
      if (pass) {
        const float* yr = y;
        asm volatile("" : "+s"(yr) : : "memory");
        ln_load_rows(geo, yr, row0, M, v);
      }
    }
    if (geo.act()) {
      ldv<F>((pass ? gamma2 : gamma1) + c, g);
      ldv<F>((pass ? beta2 : beta1) + c, b);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < F; ++i) s += v[r][i];
      const float mean = geo.sum(s) * geo.inv_d();
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < F; ++i) {
        v[r][i] = geo.act() ? v[r][i] - mean : 0.f;
        q += v[r][i] * v[r][i];
      }
      const float rstd = rsqrtf(geo.sum(q) * geo.inv_d() + eps);
      if (row0 + r < M) {
        if (geo.act()) {
#pragma unroll
          for (int i = 0; i < F; ++i) v[r][i] = v[r][i] * rstd * g[i] + b[i];
          if (pass == 0) stv<F>(y + (row0 + r) * D + c, v[r]);
          else stv<F>(z + (row0 + r) * D + c, v[r]);
        }
        if (geo.leader()) {
          (pass ? mean2 : mean1)[row0 + r] = mean;
          (pass ? rstd2 : rstd1)[row0 + r] = rstd;
        }
      }
    }
  }
}

// ---------------------------------------------------------------- backward
// dx = dres + LN'(dy), the column partials [dgamma | dbeta] = [dy xh | dy] to row blockIdx.x of ws.  One row per wave
// and trip.
template <typename Geom, typename TDY, typename TX = float>
__global__ __launch_bounds__(256) void ln_bwd_wave(const TDY* __restrict__ dy, const TX* __restrict__ x,
                                                   const float* __restrict__ gamma, const float* __restrict__ mean_in,
                                                   const float* __restrict__ rstd_in, const float* __restrict__ dres,
                                                   float* __restrict__ dx, float* __restrict__ ws, long M, LnDrop dr) {
  static_assert(Geom::kWave, "one row per wave");
  if (dr.g2 && dr.p > 0.f) dr.seed = salted_seed(dr.seed, dr.salt);
  constexpr int F = Geom::F;
  __shared__ float red[4][2 * Geom::LDSW];
  const Geom geo(threadIdx.x & 63, 0);
  const int D = geo.D(), c = geo.col();
  const int wglob = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float gm[F], pg[F], pb[F];
  ldv<F>(gamma + c, gm);
  ln_zero(pg);
  ln_zero(pb);
  for (long row = wglob; row < M; row += nwaves) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    float d[F], xh[F], g[F], sg, sgx;
    ldv<F>(dy + row * D + c, d);
    ldv<F>(x + row * D + c, xh);
#pragma unroll
    for (int i = 0; i < F; ++i) xh[i] = (xh[i] - mean) * rstd;
    ln_bwd_stage(geo, d, xh, gm, g, pg, pb, sg, sgx);
    float o[F];
    if (dres) ldv<F>(dres + row * D + c, o);
    else ln_zero(o);
#pragma unroll
    for (int i = 0; i < F; ++i) o[i] += ln_bwd_term(rstd, g[i], sg, xh[i], sgx);
    stv<F>(dx + row * D + c, o);
    ln_store_g2<Geom>(dr, row * D + c, o);
  }
  ln_write_partials(geo, red, pg, pb, ws, blockIdx.x);
}

template <typename Geom, typename TDY, typename TX = float>
__global__ __launch_bounds__(256) void ln_bwd_group(const TDY* __restrict__ dy, const TX* __restrict__ x,
                                                    const float* __restrict__ gamma, const float* __restrict__ mean_in,
                                                    const float* __restrict__ rstd_in, const float* __restrict__ dres,
                                                    float* __restrict__ dx, float* __restrict__ ws, long M, int D,
                                                    LnDrop dr) {
  static_assert(!Geom::kWave, "a lane group per row");
  if (dr.g2 && dr.p > 0.f) dr.seed = salted_seed(dr.seed, dr.salt);
  __shared__ float red[4][2 * Geom::LDSW];
  const Geom geo(threadIdx.x & 63, D);
  const int c = geo.col();
  const bool act = geo.act();
  const long slot = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * Geom::RPW + geo.sub();
  const long nslots = (long)gridDim.x * 4 * Geom::RPW;
  float gm[8], pg[8], pb[8];
  ln_zero(gm);
  ln_zero(pg);
  ln_zero(pb);
  if (act) ldv<8>(gamma + c, gm);
  // two rows per group and iteration, all their loads issued before the first reduction (one row at a time left the
  // kernel latency-bound: 9.4 us per D-144 backward for ~28 MB)
  const long nrow_iter = (M + nslots - 1) / nslots;
  for (long it = 0; it < nrow_iter; it += 2) {
    long row[2];
    bool live[2];
    float mean[2], rstd[2], d[2][8], xh[2][8], o[2][8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      row[u] = slot + (it + u) * nslots;
      live[u] = act && row[u] < M;
      mean[u] = row[u] < M ? mean_in[row[u]] : 0.f;
      rstd[u] = row[u] < M ? rstd_in[row[u]] : 0.f;
      if (live[u]) {
        ldv<8>(dy + row[u] * D + c, d[u]);
        ldv<8>(x + row[u] * D + c, xh[u]);
        if (dres) ldv<8>(dres + row[u] * D + c, o[u]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!live[u]) d[u][i] = xh[u][i] = 0.f;
        if (!live[u] || !dres) o[u][i] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float g[8], sg, sgx;
#pragma unroll
      for (int i = 0; i < 8; ++i) xh[u][i] = live[u] ? (xh[u][i] - mean[u]) * rstd[u] : 0.f;
      ln_bwd_stage(geo, d[u], xh[u], gm, g, pg, pb, sg, sgx);
      if (live[u]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[u][i] += ln_bwd_term(rstd[u], g[i], sg, xh[u][i], sgx);
        stv<8>(dx + row[u] * D + c, o[u]);
        ln_store_g2<Geom>(dr, row[u] * D + c, o[u]);
      }
    }
  }
  geo.fold(pg);
  geo.fold(pb);
  ln_write_partials(geo, red, pg, pb, ws, blockIdx.x);
}

// Backward of the pair.  dz: gradient of z; dres: the gradient reaching y down the residual path (nullable).
//   xh = (x - m1) r1, y = xh g1 + b1, yh = (y - m2) r2, gz = dz g2
//   dy = dres + r2 (gz - mean(gz) - yh mean(gz yh)),  gy = dy g1,  dx = r1 (gy - mean(gy) - xh mean(gy xh))
// i.e. ln_bwd_stage twice per row, written out (see "shared row code").  Column partials: [dg1 | db1] = [dy xh | dy] in
// the first nb x 2D block of ws, [dg2 | db2] = [dz yh | dz] in the second (each block laid out as ln_write_partials
// does, so each is one task of the grouped column reduction; one LDS block serves both in turn).  The next row's dz and x loads are issued before this row's
// reductions: the two dependent reduction stages would otherwise leave a wave with nothing in flight for twice as
// long as ln_bwd_wave does.
template <typename Geom, typename TDZ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void ln_bwd_pair_wave(
    const TDZ* __restrict__ dz, const float* __restrict__ dres, const float* __restrict__ x,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const float* __restrict__ mean1,
    const float* __restrict__ rstd1, const float* __restrict__ gamma2, const float* __restrict__ mean2,
    const float* __restrict__ rstd2, float* __restrict__ dx, float* __restrict__ ws, long M, LnDrop dr) {
  static_assert(Geom::kWave, "one row per wave");
  if (dr.g2 && dr.p > 0.f) dr.seed = salted_seed(dr.seed, dr.salt);
  constexpr int F = Geom::F;
  __shared__ float red[4][2 * Geom::LDSW];
  const Geom geo(threadIdx.x & 63, 0);
  const int D = geo.D(), c = geo.col();
  const int wv = threadIdx.x >> 6;
  const int wglob = blockIdx.x * 4 + wv;
  const int nwaves = gridDim.x * 4;
  float ga[F], ba[F], gb[F], pg1[F], pb1[F], pg2[F], pb2[F];
  ldv<F>(gamma1 + c, ga);
  ldv<F>(beta1 + c, ba);
  ldv<F>(gamma2 + c, gb);
#pragma unroll
  for (int i = 0; i < F; ++i) pg1[i] = pb1[i] = pg2[i] = pb2[i] = 0.f;
  float d[F], xh[F], st[4];
  auto fetch = [&](long row, float (&fd)[F], float (&fx)[F], float (&fs)[4]) {
    fs[0] = mean1[row]; fs[1] = rstd1[row]; fs[2] = mean2[row]; fs[3] = rstd2[row];
    ldv<F>(dz + row * D + c, fd);
    ldv<F>(x + row * D + c, fx);
  };
  long row = wglob;
  if (row < M) fetch(row, d, xh, st);
  while (row < M) {
    const long nrow = row + nwaves;
    float o[F], nd[F], nx[F], nst[4];
    if (dres) ldv<F>(dres + row * D + c, o);   // (needed after the first reduction stage)
    else {
#pragma unroll
      for (int i = 0; i < F; ++i) o[i] = 0.f;
    }
    if (nrow < M) fetch(nrow, nd, nx, nst);
    const float m1 = st[0], r1 = st[1], m2 = st[2], r2 = st[3];
    float yh[F], gz[F];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < F; ++i) {
      xh[i] = (xh[i] - m1) * r1;
      yh[i] = (xh[i] * ga[i] + ba[i] - m2) * r2;
      gz[i] = d[i] * gb[i];
      pg2[i] += d[i] * yh[i];
      pb2[i] += d[i];
      s1 += gz[i];
      s2 += gz[i] * yh[i];
    }
    s1 = geo.sum(s1) * geo.inv_d();
    s2 = geo.sum(s2) * geo.inv_d();
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int i = 0; i < F; ++i) {
      o[i] += r2 * (gz[i] - s1 - yh[i] * s2);    // dy
      gz[i] = o[i] * ga[i];                      // gy
      pg1[i] += o[i] * xh[i];
      pb1[i] += o[i];
      t1 += gz[i];
      t2 += gz[i] * xh[i];
    }
    t1 = geo.sum(t1) * geo.inv_d();
    t2 = geo.sum(t2) * geo.inv_d();
#pragma unroll
    for (int i = 0; i < F; ++i) o[i] = r1 * (gz[i] - t1 - xh[i] * t2);
    stv<F>(dx + row * D + c, o);
    ln_store_g2<Geom>(dr, row * D + c, o);
    if (nrow < M) {
#pragma unroll
      for (int i = 0; i < F; ++i) {
        d[i] = nd[i];
        xh[i] = nx[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) st[i] = nst[i];
    }
    row = nrow;
  }
  // one LDS block serves both partial pairs in turn
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    if (blk) __syncthreads();
#pragma unroll
    for (int i = 0; i < F; ++i) {
      red[wv][c + i] = blk ? pg2[i] : pg1[i];
      red[wv][D + c + i] = blk ? pb2[i] : pb1[i];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * D; q += 256)
      ws[((long)blk * gridDim.x + blockIdx.x) * 2 * D + q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
  }
}

template <typename Geom, typename TDZ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void ln_bwd_pair_group(
    const TDZ* __restrict__ dz, const float* __restrict__ dres, const float* __restrict__ x,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const float* __restrict__ mean1,
    const float* __restrict__ rstd1, const float* __restrict__ gamma2, const float* __restrict__ mean2,
    const float* __restrict__ rstd2, float* __restrict__ dx, float* __restrict__ ws, long M, int D, LnDrop dr) {
  static_assert(!Geom::kWave, "a lane group per row");
  if (dr.g2 && dr.p > 0.f) dr.seed = salted_seed(dr.seed, dr.salt);
  __shared__ float red[4][2 * Geom::LDSW];
  const Geom geo(threadIdx.x & 63, D);
  const int c = geo.col();
  const bool act = geo.act();
  const int wv = threadIdx.x >> 6;
  const long slot = ((long)blockIdx.x * 4 + wv) * Geom::RPW + geo.sub();
  const long nslots = (long)gridDim.x * 4 * Geom::RPW;
  float ga[8], ba[8], gb[8], pg1[8], pb1[8], pg2[8], pb2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ga[i] = ba[i] = gb[i] = pg1[i] = pb1[i] = pg2[i] = pb2[i] = 0.f;
  if (act) {
    ldv<8>(gamma1 + c, ga);
    ldv<8>(beta1 + c, ba);
    ldv<8>(gamma2 + c, gb);
  }
  // U rows per group and iteration: with the four partial rows and three parameter rows a lane holds here, two rows
  // in flight (ln_bwd_group's form) do not fit the registers that three waves per SIMD leave
  constexpr int U = 1;
  const long nrow_iter = (M + nslots - 1) / nslots;
  for (long it = 0; it < nrow_iter; it += U) {
    long row[U];
    bool live[U];
    float m1[U], r1[U], m2[U], r2[U], d[U][8], xh[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row[u] = slot + (it + u) * nslots;
      live[u] = act && row[u] < M;
      m1[u] = row[u] < M ? mean1[row[u]] : 0.f;
      r1[u] = row[u] < M ? rstd1[row[u]] : 0.f;
      m2[u] = row[u] < M ? mean2[row[u]] : 0.f;
      r2[u] = row[u] < M ? rstd2[row[u]] : 0.f;
      if (live[u]) {
        ldv<8>(dz + row[u] * D + c, d[u]);
        ldv<8>(x + row[u] * D + c, xh[u]);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!live[u]) d[u][i] = xh[u][i] = 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float o[8], yh[8], gz[8], s1 = 0.f, s2 = 0.f;
      if (live[u] && dres) ldv<8>(dres + row[u] * D + c, o);   // (needed after the first reduction stage)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (!live[u] || !dres) o[i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xh[u][i] = live[u] ? (xh[u][i] - m1[u]) * r1[u] : 0.f;
        yh[i] = live[u] ? (xh[u][i] * ga[i] + ba[i] - m2[u]) * r2[u] : 0.f;
        gz[i] = d[u][i] * gb[i];
        pg2[i] += d[u][i] * yh[i];
        pb2[i] += d[u][i];
        s1 += gz[i];
        s2 += gz[i] * yh[i];
      }
      s1 = geo.sum(s1) * geo.inv_d();
      s2 = geo.sum(s2) * geo.inv_d();
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[i] = live[u] ? o[i] + r2[u] * (gz[i] - s1 - yh[i] * s2) : 0.f;    // dy
        gz[i] = o[i] * ga[i];                                                  // gy
        pg1[i] += o[i] * xh[u][i];
        pb1[i] += o[i];
        t1 += gz[i];
        t2 += gz[i] * xh[u][i];
      }
      t1 = geo.sum(t1) * geo.inv_d();
      t2 = geo.sum(t2) * geo.inv_d();
      if (live[u]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = r1[u] * (gz[i] - t1 - xh[u][i] * t2);
        stv<8>(dx + row[u] * D + c, o);
        if (dr.g2) {   // ln_store_g2, written out: through the function this kernel at G = 64 ran 8 % longer
          float sc[8];
          if (dr.p > 0.f) dropout_scale8(dr.p, dr.seed, (uint64_t)(row[u] * D + c), sc);
#pragma unroll
          for (int i = 0; i < 8; ++i) sc[i] = dr.p > 0.f ? dr.scale * sc[i] : dr.scale;
          float q[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) q[i] = o[i] * sc[i];
          st8_dyn(dr.g2, CFM_BF16, row[u] * D + c, q);
        }
      }
    }
  }
  geo.fold(pg1);
  geo.fold(pb1);
  geo.fold(pg2);
  geo.fold(pb2);
  // one LDS block serves both partial pairs in turn
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    if (blk) __syncthreads();
    if (geo.heads()) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        red[wv][c + i] = blk ? pg2[i] : pg1[i];
        red[wv][Geom::LDSW + c + i] = blk ? pb2[i] : pb1[i];
      }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 2 * D; q += 256) {
      const int k = q < D ? q : Geom::LDSW + (q - D);
      ws[((long)blk * gridDim.x + blockIdx.x) * 2 * D + q] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
    }
  }
}

// ---------------------------------------------------------------- generic kernels (any D <= 1024)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const void* __restrict__ x, int dtx,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, void* __restrict__ y,
                                                     int dty, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, long M, int D, float eps,
                                                     const void* __restrict__ delta = nullptr, int dtd = 0,
                                                     float* __restrict__ xo = nullptr) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float v[MAXJ];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int c = lane + 64 * j;
    v[j] = c < D ? ld_dyn(x, dtx, row * D + c) : 0.f;
    if (delta && c < D) {   // (cfm_layernorm_fwd_res: x + delta, stored to xo)
      v[j] += ld_dyn(delta, dtd, row * D + c);
      xo[row * D + c] = v[j];
    }
    s += v[j];
  }
  const float mean = wave_sum(s) / D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int c = lane + 64 * j;
    const float d = c < D ? v[j] - mean : 0.f;
    q += d * d;
  }
  const float rstd = rsqrtf(wave_sum(q) / D + eps);
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int c = lane + 64 * j;
    if (c < D) st_dyn(y, dty, row * D + c, (v[j] - mean) * rstd * gamma[c] + beta[c]);
  }
  if (lane == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }
}

__global__ __launch_bounds__(256) void ln_bwd_kernel(const void* __restrict__ dy, int dtdy,
                                                     const void* __restrict__ x, int dtx,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ mean_in,
                                                     const float* __restrict__ rstd_in,
                                                     const void* __restrict__ dres, int dtres,
                                                     void* __restrict__ dx, int dtdx, float* __restrict__ ws,
                                                     long M, int D) {
  const int lane = threadIdx.x & 63;
  const int wglob = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * 4;
  float pg[MAXJ], pb[MAXJ];
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) pg[j] = pb[j] = 0.f;
  for (long row = wglob; row < M; row += nwaves) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    float xh[MAXJ], g[MAXJ];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int c = lane + 64 * j;
      if (c < D) {
        const float d = ld_dyn(dy, dtdy, row * D + c);
        xh[j] = (ld_dyn(x, dtx, row * D + c) - mean) * rstd;
        g[j] = d * gamma[c];
        pg[j] += d * xh[j];
        pb[j] += d;
      } else {
        xh[j] = g[j] = 0.f;
      }
      sg += g[j];
      sgx += g[j] * xh[j];
    }
    sg = wave_sum(sg) / D;
    sgx = wave_sum(sgx) / D;
#pragma unroll
    for (int j = 0; j < MAXJ; ++j) {
      const int c = lane + 64 * j;
      if (c < D) {
        float v = rstd * (g[j] - sg - xh[j] * sgx);
        if (dres) v += ld_dyn(dres, dtres, row * D + c);
        st_dyn(dx, dtdx, row * D + c, v);
      }
    }
  }
  __shared__ float red[4][2 * 64 * MAXJ];
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MAXJ; ++j) {
    const int c = lane + 64 * j;
    if (c < D) {
      red[wv][c] = pg[j];
      red[wv][D + c] = pb[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256)
    ws[(long)blockIdx.x * 2 * D + c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// ---------------------------------------------------------------- host: one dispatcher
template <typename T> struct LnTag { typedef T type; };

// Turns a cfm_ln_choice and the runtime dtypes into compile-time tags, once: f(LnTag<Geom>, LnTag<TX>, LnTag<TY>)
// with Geom = RowWave<V> / RowGroup<G>, TX the type of x and TY that of the other streamed operand (y, z, dy or dz).
// f launches and returns true, or returns false where its kernel set (the ln_*_exists predicates below) has no such
// kernel -- ln_plan never chooses one, so false is a bug and the entry points report it.  GENERIC is not f's business.
template <typename Fn> bool ln_dispatch(const cfm_ln_choice& c, int dtx, int dty, Fn&& f) {
  auto types = [&](auto geo) {
    auto ty = [&](auto tx) { return dty == CFM_BF16 ? f(geo, tx, LnTag<bf16>{}) : f(geo, tx, LnTag<float>{}); };
    return dtx == CFM_BF16 ? ty(LnTag<bf16>{}) : ty(LnTag<float>{});
  };
  if (c.family == CFM_LN_WAVE) {
    switch (c.width) {
      case 2: return types(LnTag<RowWave<2>>{});
      case 4: return types(LnTag<RowWave<4>>{});
      case 8: return types(LnTag<RowWave<8>>{});
      case 16: return types(LnTag<RowWave<16>>{});
    }
  } else if (c.family == CFM_LN_GROUP) {
    switch (c.width) {
      case 16: return types(LnTag<RowGroup<16>>{});
      case 32: return types(LnTag<RowGroup<32>>{});
      case 64: return types(LnTag<RowGroup<64>>{});
    }
  }
  return false;
}
// the kernels that exist: the MX copy on RowWave V >= 4 with a bf16 y; x + delta on the fp32 stream; pairs on V 4 / 8
// and the lane groups, fp32 x
template <typename Geom, typename TY, bool MX, typename TX, bool RS>
constexpr bool ln_fwd_exists = (!MX || (Geom::kWave && Geom::F >= 4 && std::is_same<TY, bf16>::value)) &&
                               (!RS || std::is_same<TX, float>::value);
template <typename Geom, typename TX>
constexpr bool ln_pair_exists = (!Geom::kWave || Geom::F == 4 || Geom::F == 8) && std::is_same<TX, float>::value;

#define LN_TAGS(geo, tx, ty)                 \
  typedef typename decltype(geo)::type Geom; \
  typedef typename decltype(tx)::type TX;    \
  typedef typename decltype(ty)::type TY

// The forward of cfm_layernorm_fwd / _fwd_mx_ex / _fwd_res: fills the rest of q, plans, launches.  delta / xout (x +
// delta) and y8 / s8 (the MX copy) are nullable.
int ln_forward(const char* who, cfm_ln_query& q, const void* x, int dtx, const void* delta, int dtd, float* xout,
               const float* gamma, const float* beta, void* y, int dty, void* y8, uint8_t* s8, float* mean, float* rstd,
               long M, int D, float eps, void* stream) {
  q.M = M; q.D = D; q.dt_x = dtx; q.dt_y = dty; q.dt_delta = dtd; q.want_mx = y8 != nullptr;
  q.x_mod16 = ln_mod16(x); q.y_mod16 = ln_mod16(y); q.gamma_mod16 = ln_mod16(gamma); q.beta_mod16 = ln_mod16(beta);
  q.delta_mod16 = ln_mod16(delta); q.xout_mod16 = ln_mod16(xout); q.y8_mod16 = ln_mod16(y8);
  cfm_ln_choice c;
  const int rc = ln_plan(q, c, who);
  if (rc != CFM_OK || M == 0) return rc;
  hipStream_t s = cfm::as_stream(stream);
  if (c.family == CFM_LN_GENERIC) {
    hipLaunchKernelGGL(ln_fwd_kernel, dim3(c.blocks), dim3(256), 0, s, x, dtx, gamma, beta, y, dty, mean, rstd, M, D,
                       eps, delta, dtd, xout);
    return cfm::check_launch(who);
  }
  const LnMx mx{(uint8_t*)y8, s8};
  const LnRes rs{(const bf16*)delta, xout};
  auto launch = [&](auto mxt, auto rst) {
    constexpr bool MX = decltype(mxt)::value, RS = decltype(rst)::value;
    return ln_dispatch(c, dtx, dty, [&](auto geo, auto tx, auto ty) {
      LN_TAGS(geo, tx, ty);
      if constexpr (ln_fwd_exists<Geom, TY, MX, TX, RS>) {
        hipLaunchKernelGGL((ln_fwd<Geom, TY, MX, TX, RS>), dim3(c.blocks), dim3(256), 0, s, (const TX*)x, gamma, beta,
                           (TY*)y, mean, rstd, M, D, eps, mx, rs);
        return true;
      } else {
        return false;
      }
    });
  };
  const std::true_type yes;
  const std::false_type no;
  const bool ok = y8 ? (delta ? launch(yes, yes) : launch(yes, no)) : (delta ? launch(no, yes) : launch(no, no));
  if (!ok) return cfm::fail(CFM_ERR_UNSUPPORTED, std::string(who) + ": no kernel for the plan's choice");
  return cfm::check_launch(who);
}

// the column reductions behind a backward kernel: out (+)= the nb partial rows of ws
void ln_reduce_cols(float* ws, int nb, int D, float* dgamma, float* dbeta, hipStream_t s) {
  if (dgamma && dbeta && dbeta == dgamma + D) {
    cfm::colreduce(ws, nb, 2L * D, dgamma, 0, s);               // one pass for [dgamma | dbeta]
  } else {
    if (dgamma) cfm::colreduce(ws, nb, D, dgamma, 0, s, 2L * D);
    if (dbeta) cfm::colreduce(ws + D, nb, D, dbeta, 0, s, 2L * D);
  }
}
}  // namespace

CFM_EXPORT int cfm_layernorm_plan(const cfm_ln_query* q, cfm_ln_choice* out) {
  CFM_REQUIRE(q && out, CFM_ERR_ARG, "null pointer");
  return ln_plan(*q, *out, "cfm_layernorm_plan");
}

CFM_EXPORT int cfm_layernorm_fwd(const void* x, int dtx, const float* gamma, const float* beta, void* y, int dty,
                                 float* mean, float* rstd, long M, int D, float eps, void* stream) {
  CFM_REQUIRE(x && gamma && beta && y && mean && rstd, CFM_ERR_ARG, "null pointer");
  cfm_ln_query q{CFM_LN_FWD};
  return ln_forward("cfm_layernorm_fwd", q, x, dtx, nullptr, 0, nullptr, gamma, beta, y, dty, nullptr, nullptr, mean,
                    rstd, M, D, eps, stream);
}

CFM_EXPORT int cfm_layernorm_fwd_mx_ex(const void* x, int dtx, const float* gamma, const float* beta, void* y, void* y8,
                                       uint8_t* s8, float* mean, float* rstd, long M, int D, float eps, void* stream) {
  CFM_REQUIRE(x && gamma && beta && y && y8 && s8 && mean && rstd, CFM_ERR_ARG, "null pointer");
  cfm_ln_query q{CFM_LN_FWD};
  return ln_forward("cfm_layernorm_fwd_mx", q, x, dtx, nullptr, 0, nullptr, gamma, beta, y, CFM_BF16, y8, s8, mean,
                    rstd, M, D, eps, stream);
}

CFM_EXPORT int cfm_layernorm_fwd_res(const float* x, const void* delta, int dtd, float* xout, const float* gamma,
                                     const float* beta, void* y, int dty, void* y8, uint8_t* s8, float* mean,
                                     float* rstd, long M, int D, float eps, void* stream) {
  CFM_REQUIRE(x && delta && xout && gamma && beta && y && mean && rstd, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE((const void*)x != (const void*)xout && delta != (const void*)xout, CFM_ERR_ARG,
              "xout must not alias x or delta");
  CFM_REQUIRE(!y8 || s8, CFM_ERR_SHAPE, "MX copy: y8 and s8");
  cfm_ln_query q{CFM_LN_FWD_RES};
  return ln_forward("cfm_layernorm_fwd_res", q, x, CFM_F32, delta, dtd, xout, gamma, beta, y, dty, y8, s8, mean, rstd,
                    M, D, eps, stream);
}

CFM_EXPORT int cfm_layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* y, void* y8,
                                    uint8_t* s8, float* mean, float* rstd, long M, int D, float eps, void* stream) {
  return cfm_layernorm_fwd_mx_ex(x, CFM_F32, gamma, beta, y, y8, s8, mean, rstd, M, D, eps, stream);
}

// the workspace of a backward over M rows of width D; 0 where the entry point refuses the shape
CFM_EXPORT size_t cfm_layernorm_ws_bytes(long M, int D) {
  cfm_ln_query q{CFM_LN_BWD, D, M};
  cfm_ln_choice c;
  return ln_plan(q, c, "cfm_layernorm_ws_bytes") == CFM_OK ? c.ws_bytes : 0;
}

CFM_EXPORT int cfm_scale_dropout(const void* x, int dtx, void* y, int dty, long n, float scale, float p,
                                 uint64_t seed, uint64_t off, void* stream);

CFM_EXPORT int cfm_layernorm_bwd_drop(const void* dy, int dtdy, const void* x, int dtx, const float* gamma,
                                      const float* mean, const float* rstd, const void* dres, int dtres, void* dx,
                                      int dtdx, float* dgamma, float* dbeta, float* ws, long M, int D, void* g2,
                                      float g2_scale, float g2_p, uint64_t g2_seed, void* stream) {
  CFM_REQUIRE(dy && x && gamma && mean && rstd && dx && ws, CFM_ERR_ARG, "null pointer");
  cfm_ln_query q{CFM_LN_BWD, D, M};
  q.dt_x = dtx; q.dt_dy = dtdy; q.dt_dx = dtdx; q.dt_dres = dres ? dtres : (int)CFM_F32; q.want_g2 = g2 != nullptr;
  q.dy_mod16 = ln_mod16(dy); q.x_mod16 = ln_mod16(x); q.gamma_mod16 = ln_mod16(gamma); q.dres_mod16 = ln_mod16(dres);
  q.dx_mod16 = ln_mod16(dx); q.g2_mod16 = ln_mod16(g2);
  cfm_ln_choice c;
  const int rc = ln_plan(q, c, "cfm_layernorm_bwd");
  if (rc != CFM_OK) return rc;
  hipStream_t s = cfm::as_stream(stream);
  const LnDrop dr{c.g2_fused ? g2 : nullptr, g2_scale, g2_p, g2_seed, cfm::g_rng_salt};
  if (c.family == CFM_LN_GENERIC) {
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(c.blocks), dim3(256), 0, s, dy, dtdy, x, dtx, gamma, mean, rstd, dres, dtres,
                       dx, dtdx, ws, M, D);
  } else {
    ln_dispatch(c, dtx, dtdy, [&](auto geo, auto tx, auto ty) {
      LN_TAGS(geo, tx, ty);
      if constexpr (Geom::kWave)
        hipLaunchKernelGGL((ln_bwd_wave<Geom, TY, TX>), dim3(c.blocks), dim3(256), 0, s, (const TY*)dy, (const TX*)x,
                           gamma, mean, rstd, (const float*)dres, (float*)dx, ws, M, dr);
      else
        hipLaunchKernelGGL((ln_bwd_group<Geom, TY, TX>), dim3(c.blocks), dim3(256), 0, s, (const TY*)dy, (const TX*)x,
                           gamma, mean, rstd, (const float*)dres, (float*)dx, ws, M, D, dr);
      return true;
    });
  }
  if (g2 && !c.g2_fused) {
    const int rc2 = cfm_scale_dropout(dx, dtdx, g2, CFM_BF16, M * D, g2_scale, g2_p, g2_seed, 0, stream);
    if (rc2 != CFM_OK) return rc2;
  }
  ln_reduce_cols(ws, c.blocks, D, dgamma, dbeta, s);
  return cfm::check_launch("cfm_layernorm_bwd");
}

CFM_EXPORT int cfm_layernorm_bwd(const void* dy, int dtdy, const void* x, int dtx, const float* gamma,
                                 const float* mean, const float* rstd, const void* dres, int dtres, void* dx,
                                 int dtdx, float* dgamma, float* dbeta, float* ws, long M, int D,
                                 void* stream) {
  return cfm_layernorm_bwd_drop(dy, dtdy, x, dtx, gamma, mean, rstd, dres, dtres, dx, dtdx, dgamma, dbeta, ws, M, D,
                                nullptr, 0.f, 0.f, 0, stream);
}

CFM_EXPORT int cfm_layernorm_pair_ok(int D, int dtype_z) {
  cfm_ln_query q{CFM_LN_FWD_PAIR, D, 0};
  q.dt_y = dtype_z;
  cfm_ln_choice c;
  return ln_plan(q, c, "cfm_layernorm_pair_ok") == CFM_OK;
}

CFM_EXPORT size_t cfm_layernorm_fwd_pair_ws_bytes(long, int) { return 0; }

CFM_EXPORT int cfm_layernorm_fwd_pair(const float* x, const float* gamma1, const float* beta1, const float* gamma2,
                                      const float* beta2, float* y, void* z, int dtz, float* mean1, float* rstd1,
                                      float* mean2, float* rstd2, long M, int D, float eps, void* stream) {
  CFM_REQUIRE(x && gamma1 && beta1 && gamma2 && beta2 && y && z && mean1 && rstd1 && mean2 && rstd2, CFM_ERR_ARG,
              "null pointer");
  cfm_ln_query q{CFM_LN_FWD_PAIR, D, M};
  q.dt_y = dtz;
  q.x_mod16 = ln_mod16(x); q.y_mod16 = ln_mod16(y); q.z_mod16 = ln_mod16(z); q.gamma_mod16 = ln_mod16(gamma1);
  q.beta_mod16 = ln_mod16(beta1); q.gamma2_mod16 = ln_mod16(gamma2); q.beta2_mod16 = ln_mod16(beta2);
  cfm_ln_choice c;
  const int rc = ln_plan(q, c, "cfm_layernorm_fwd_pair");
  if (rc != CFM_OK || M == 0) return rc;
  hipStream_t s = cfm::as_stream(stream);
  ln_dispatch(c, CFM_F32, dtz, [&](auto geo, auto tx, auto ty) {
    LN_TAGS(geo, tx, ty);
    if constexpr (ln_pair_exists<Geom, TX>) {
      hipLaunchKernelGGL((ln_fwd_pair<Geom, TY>), dim3(c.blocks), dim3(256), 0, s, x, gamma1, beta1, gamma2, beta2, y,
                         (TY*)z, mean1, rstd1, mean2, rstd2, M, D, eps);
      return true;
    } else {
      return false;
    }
  });
  return cfm::check_launch("cfm_layernorm_fwd_pair");
}

// 0 where no fused pair kernel exists (cfm_layernorm_pair_ok)
CFM_EXPORT size_t cfm_layernorm_bwd_pair_ws_bytes(long M, int D) {
  cfm_ln_query q{CFM_LN_BWD_PAIR, D, M};
  cfm_ln_choice c;
  return ln_plan(q, c, "cfm_layernorm_bwd_pair_ws_bytes") == CFM_OK ? c.ws_bytes : 0;
}

CFM_EXPORT int cfm_layernorm_bwd_pair(const void* dz, int dtdz, const float* dres, const float* x,
                                      const float* gamma1, const float* beta1, const float* mean1, const float* rstd1,
                                      const float* gamma2, const float* mean2, const float* rstd2, float* dx,
                                      float* dgb1, float* dgb2, float* ws, long M, int D, void* g2, float g2_scale,
                                      float g2_p, uint64_t g2_seed, void* stream) {
  CFM_REQUIRE(dz && x && gamma1 && beta1 && mean1 && rstd1 && gamma2 && mean2 && rstd2 && dx && ws, CFM_ERR_ARG,
              "null pointer");
  cfm_ln_query q{CFM_LN_BWD_PAIR, D, M};
  q.dt_dy = dtdz; q.want_g2 = g2 != nullptr;
  q.dy_mod16 = ln_mod16(dz); q.dres_mod16 = ln_mod16(dres); q.x_mod16 = ln_mod16(x); q.dx_mod16 = ln_mod16(dx);
  q.gamma_mod16 = ln_mod16(gamma1); q.beta_mod16 = ln_mod16(beta1); q.gamma2_mod16 = ln_mod16(gamma2);
  q.g2_mod16 = ln_mod16(g2);
  cfm_ln_choice c;
  const int rc = ln_plan(q, c, "cfm_layernorm_bwd_pair");
  if (rc != CFM_OK) return rc;
  hipStream_t s = cfm::as_stream(stream);
  const int nb = c.blocks;
  const LnDrop dr{c.g2_fused ? g2 : nullptr, g2_scale, g2_p, g2_seed, cfm::g_rng_salt};
  ln_dispatch(c, CFM_F32, dtdz, [&](auto geo, auto tx, auto ty) {
    LN_TAGS(geo, tx, ty);
    if constexpr (!ln_pair_exists<Geom, TX>) {
      return false;
    } else {
      if constexpr (Geom::kWave)
        hipLaunchKernelGGL((ln_bwd_pair_wave<Geom, TY>), dim3(nb), dim3(256), 0, s, (const TY*)dz, dres, x, gamma1,
                           beta1, mean1, rstd1, gamma2, mean2, rstd2, dx, ws, M, dr);
      else
        hipLaunchKernelGGL((ln_bwd_pair_group<Geom, TY>), dim3(nb), dim3(256), 0, s, (const TY*)dz, dres, x, gamma1,
                           beta1, mean1, rstd1, gamma2, mean2, rstd2, dx, ws, M, D, dr);
      return true;
    }
  });
  if (g2 && !c.g2_fused) {
    const int rc2 = cfm_scale_dropout(dx, CFM_F32, g2, CFM_BF16, M * D, g2_scale, g2_p, g2_seed, 0, stream);
    if (rc2 != CFM_OK) return rc2;
  }
  float* part2 = ws + (long)nb * 2 * D;
  if (dgb1 && dgb2) cfm::colreduce_pair(ws, part2, nb, 2L * D, dgb1, dgb2, s);
  else if (dgb1) cfm::colreduce(ws, nb, 2L * D, dgb1, 0, s);
  else if (dgb2) cfm::colreduce(part2, nb, 2L * D, dgb2, 0, s);
  return cfm::check_launch("cfm_layernorm_bwd_pair");
}
