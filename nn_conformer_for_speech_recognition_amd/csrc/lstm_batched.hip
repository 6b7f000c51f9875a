// Batched LSTM recurrence: B independent sequences of up to T steps side by side (nn.LSTM on a 3-D input with
// packed-sequence semantics), next to the single-sequence recurrence of lstm.hip, which stays as it is.
//   forward   gates_t = gx_t + h_pred W_hh^T,  c_t = f c_pred + i g,  h_t = o tanh(c_t)      (gate order i, f, g, o)
//   backward  dh_t = dy_t + dg_succ W_hh,  dc_t = dh_t o (1 - tanh^2 c_t) + dc_succ f_succ,   dg_t as lstm_bwd_rec
// Sequence b has len_b = clamp(lengths[b], 0, T) valid steps.  The forward direction runs t = 0 .. len_b-1, the
// reverse direction t = len_b-1 .. 0, both from a zero state; step s of a pass handles t = s (forward) or
// t = len_b-1-s (reverse) of every sequence with s < len_b, and the padding position t = s of every other one.
//
// ONE PLAIN LAUNCH PER TIME STEP, issued by the C entry point in a stream-ordered loop: step s reads row (b, t -+ 1)
// of y / c (forward) or dg (backward) that the previous launch stored.  No cooperative launch, no flag, no wait on
// another workgroup anywhere, so nothing can time out and the T launches capture into a HIP graph.
//
// Tiling.  A step is the product (B x K) . (K x N) per direction: K = H, N = 4H forward; K = 4H, N = H backward
// (against the transposed weights, so both read weight rows along K).  One workgroup of 4 waves owns an 8-unit x
// 8-sequence tile; the launch has (H / 8) x ndir x ceil(B / 8) of them (512 at H 512, B 32: two per CU).  A step
// is bound by memory LATENCY, not by arithmetic (2048 FMAs per lane in all), so the tile's K is dealt out in
// 16-B chunks first over the 4 waves and then over the lanes of a wave: at H 512 a lane has 4 chunks, whose loads
// are all in flight before its first FMA.  Every lane keeps a 4 x 8 register tile (4 weight rows x 8 sequences),
// so one weight float4 is reused by 8 sequences and one state float4 by 4 rows: 12 loads per 128 FMAs, all 16-B,
// each a whole 128-B (forward) or 512-B (backward) run per weight row / sequence across the lanes.  Neither
// operand is reused by another lane, so staging them in LDS would only add a hop.  The K-partials are combined by
// a halving butterfly inside the wave (28 or 31 shuffles) that leaves every lane one (unit, sequence) pair, then
// across the 4 waves through 4 KB of LDS in the fixed order (w0 + w1) + (w2 + w3) by wave 0, which does the
// pointwise part.  Lane pairing, chunk order and wave order are the same for every slot, so the operation order
// of a sequence does not depend on its place in the batch, and two runs are bit-identical (no atomics).
// Padding: every use of a length is a select -- state and gradient rows of a finished or not-yet-started sequence
// are never loaded (zeros take their place), y = 0 / hprev = 0 / dg = 0 are stored at padding positions, and gx,
// dy, gates and c are never read there.
#include "cfm_common.h"

namespace {

constexpr int kUnits = 8;      // hidden units per workgroup
constexpr int kSeq = 8;        // sequences per workgroup
constexpr int kWaves = 4;      // waves per workgroup: they split K
constexpr int kMaxH = 1024;

// the sigm / tanh_f forms of lstm.hip
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float r = (1.f - e) / (1.f + e);
  return copysignf(r, x);
}

__device__ __forceinline__ int seq_len(const int32_t* lengths, int b, int B, int T) {
  if (b >= B) return 0;
  return lengths ? min(max(lengths[b], 0), T) : T;
}

// acc[s * 4 + g] += sum over this lane's chunks of K of w[g][k] * a[s][k]: K is cut into runs of KL float4; wave
// `wave` takes the runs wave, wave + 4, ... and lane kl the float4 kl of each.  Sequence s takes part when bit s
// of `live` is set (wave-uniform); else its row is not read.
template <int KL>
__device__ __forceinline__ void tile_dot(const float* const (&wr)[4], const float* const (&ar)[kSeq], unsigned live,
                                         int K, int wave, int kl, float (&acc)[4 * kSeq]) {
#pragma unroll 2
  for (int k = 4 * (wave * KL + kl); k < K; k += 4 * KL * kWaves) {
    float4 w[4], a[kSeq];
#pragma unroll
    for (int g = 0; g < 4; ++g) w[g] = *reinterpret_cast<const float4*>(wr[g] + k);
#pragma unroll
    for (int s = 0; s < kSeq; ++s)
      a[s] = (live >> s) & 1u ? *reinterpret_cast<const float4*>(ar[s] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int s = 0; s < kSeq; ++s)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v = acc[s * 4 + g];
        v = fmaf(w[g].x, a[s].x, v);
        v = fmaf(w[g].y, a[s].y, v);
        v = fmaf(w[g].z, a[s].z, v);
        v = fmaf(w[g].w, a[s].w, v);
        acc[s * 4 + g] = v;
      }
  }
}

// One exchange of the butterfly: lanes kl and kl ^ OFF split the first 2 * HALF slots between them (the lane with
// bit OFF set keeps the upper half) and add what the partner gives.  All slot indices are compile-time constants.
template <int OFF, int HALF>
__device__ __forceinline__ void reduce_step(float (&acc)[4 * kSeq], int kl) {
  const bool up = (kl & OFF) != 0;
#pragma unroll
  for (int j = 0; j < HALF; ++j) {
    const float give = up ? acc[j] : acc[j + HALF];
    const float keep = up ? acc[j + HALF] : acc[j];
    acc[j] = keep + __shfl_xor(give, OFF, 64);
  }
}

// Sum the 32 slots over the KL lanes of a group, halving the slots a lane keeps at every exchange: afterwards
// lane kl holds slots (kl * 32 / KL) .. in acc[0 .. 32 / KL).  KL 8: the four gates of sequence kl; KL 32: slot kl.
template <int KL>
__device__ __forceinline__ void tile_reduce(float (&acc)[4 * kSeq], int kl) {
  if constexpr (KL == 8) {
    reduce_step<4, 16>(acc, kl);
    reduce_step<2, 8>(acc, kl);
    reduce_step<1, 4>(acc, kl);
  } else {
    static_assert(KL == 32, "KL 8 or 32");
    reduce_step<16, 16>(acc, kl);
    reduce_step<8, 8>(acc, kl);
    reduce_step<4, 4>(acc, kl);
    reduce_step<2, 2>(acc, kl);
    reduce_step<1, 1>(acc, kl);
  }
}

// Sum the first N slots of every lane over the 4 waves, in the order (w0 + w1) + (w2 + w3); the result is valid
// in wave 0 only.  red: kWaves * 64 * N floats of LDS.
template <int N>
__device__ __forceinline__ void wave_reduce(float (&acc)[4 * kSeq], float* red, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < N; ++j) red[(wave * N + j) * 64 + lane] = acc[j];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j)
      acc[j] = (acc[j] + red[(N + j) * 64 + lane]) + (red[(2 * N + j) * 64 + lane] + red[(3 * N + j) * 64 + lane]);
  }
}

// One forward step.  grid (H / 8, ndir, ceil(B / 8)); block 256.
__global__ __launch_bounds__(64 * kWaves) void lstm_batched_fwd_step(
    const float* __restrict__ gx, const float* __restrict__ whh, const int32_t* __restrict__ lengths, float* y,
    float* __restrict__ gates, float* c, float* __restrict__ hprev, int B, int T, long sb, long st, int H, int ndir,
    int step) {
  __shared__ float red[kWaves * 64 * 4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dir = blockIdx.y;
  const int b0 = blockIdx.z * kSeq;
  const int kl = lane & 7;
  const int u = blockIdx.x * kUnits + (lane >> 3);
  const long ldy = (long)ndir * H, ldg = 4 * ldy;

  float acc[4 * kSeq];
#pragma unroll
  for (int j = 0; j < 4 * kSeq; ++j) acc[j] = 0.f;
  if (step > 0) {
    unsigned live = 0;
    const float* ar[kSeq];
#pragma unroll
    for (int s = 0; s < kSeq; ++s) {
      const int len = seq_len(lengths, b0 + s, B, T);
      const bool on = step < len;
      // predecessor: t - 1 = step - 1 forward, t + 1 = len - step reverse
      const long tp = on ? (dir ? len - step : step - 1) : 0;
      const long b = on ? b0 + s : 0;
      ar[s] = y + (b * sb + tp * st) * ldy + (long)dir * H;
      live |= (on ? 1u : 0u) << s;
    }
    if (live) {
      const float* wr[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) wr[g] = whh + ((long)dir * 4 * H + (long)g * H + u) * H;
      tile_dot<8>(wr, ar, live, H, wave, kl, acc);
    }
  }
  tile_reduce<8>(acc, kl);   // acc[0..3]: this wave's part of i, f, g, o of (unit u, sequence b0 + kl), without gx
  wave_reduce<4>(acc, red, wave, lane);
  if (wave != 0) return;

  const int b = b0 + kl;
  if (b >= B) return;
  const int len = seq_len(lengths, b, B, T);
  const long col = (long)dir * H + u;
  if (step < len) {
    const long t = dir ? len - 1 - step : step;
    const long row = b * sb + t * st;
    const float* gp = gx + row * ldg + (long)dir * 4 * H + u;
    const float ig = sigm(acc[0] + gp[0]), fg = sigm(acc[1] + gp[H]);
    const float gg = tanh_f(acc[2] + gp[2 * H]), og = sigm(acc[3] + gp[3 * H]);
    float cp = 0.f, hp = 0.f;
    if (step > 0) {
      const long prow = b * sb + (dir ? t + 1 : t - 1) * st;
      cp = c[prow * ldy + col];
      hp = y[prow * ldy + col];
    }
    const float cn = fg * cp + ig * gg;
    float* go = gates + row * ldg + (long)dir * 4 * H + u;
    go[0] = ig;
    go[H] = fg;
    go[2 * H] = gg;
    go[3 * H] = og;
    c[row * ldy + col] = cn;
    y[row * ldy + col] = og * tanh_f(cn);
    if (hprev) hprev[row * ldy + col] = hp;
  } else {
    const long row = b * sb + (long)step * st;   // padding position t = step
    y[row * ldy + col] = 0.f;
    if (hprev) hprev[row * ldy + col] = 0.f;
  }
}

// One backward step (steps run T-1 .. 0).  Same grid; whh_t (ndir, H, 4H) is W_hh transposed per direction;
// dcarry (B, ndir*H): dc_succ * f_succ of every (sequence, unit), read and rewritten by the one lane that owns it.
__global__ __launch_bounds__(64 * kWaves) void lstm_batched_bwd_step(
    const float* __restrict__ dy, const float* __restrict__ whh_t, const float* __restrict__ gates,
    const float* __restrict__ cst, const int32_t* __restrict__ lengths, float* dg, float* dcarry, int B, int T,
    long sb, long st, int H, int ndir, int step) {
  __shared__ float red[kWaves * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int dir = blockIdx.y;
  const int b0 = blockIdx.z * kSeq;
  const int kl = lane & 31;
  const int u4 = blockIdx.x * kUnits + (lane >> 5) * 4;   // this half-wave's 4 units
  const int H4 = 4 * H;
  const long ldy = (long)ndir * H, ldg = 4 * ldy;

  float acc[4 * kSeq];
#pragma unroll
  for (int j = 0; j < 4 * kSeq; ++j) acc[j] = 0.f;
  {
    unsigned live = 0;
    const float* ar[kSeq];
#pragma unroll
    for (int s = 0; s < kSeq; ++s) {
      const int len = seq_len(lengths, b0 + s, B, T);
      const bool on = step + 1 < len;
      // successor: t + 1 = step + 1 forward, t - 1 = len - 2 - step reverse
      const long tn = on ? (dir ? len - 2 - step : step + 1) : 0;
      const long b = on ? b0 + s : 0;
      ar[s] = dg + (b * sb + tn * st) * ldg + (long)dir * H4;
      live |= (on ? 1u : 0u) << s;
    }
    if (live) {
      const float* wr[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) wr[g] = whh_t + ((long)dir * H + u4 + g) * H4;
      tile_dot<32>(wr, ar, live, H4, wave, kl, acc);
    }
  }
  tile_reduce<32>(acc, kl);   // acc[0]: this wave's part of dg_succ W_hh of (unit u4 + (kl & 3), sequence b0 + (kl >> 2))
  wave_reduce<1>(acc, red, wave, lane);
  if (wave != 0) return;

  const int b = b0 + (kl >> 2), u = u4 + (kl & 3);
  if (b >= B) return;
  const int len = seq_len(lengths, b, B, T);
  const long col = (long)dir * H + u;
  if (step < len) {
    const long t = dir ? len - 1 - step : step;
    const long row = b * sb + t * st;
    const float* gp = gates + row * ldg + (long)dir * H4 + u;
    const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
    const float ct = cst[row * ldy + col];
    const float cp = step > 0 ? cst[(b * sb + (dir ? t + 1 : t - 1) * st) * ldy + col] : 0.f;
    float* dcp = dcarry + (long)b * ldy + col;
    const float carry = step + 1 < len ? *dcp : 0.f;
    const float dh = dy[row * ldy + col] + acc[0];
    const float tc = tanh_f(ct);
    const float dc = dh * og * (1.f - tc * tc) + carry;
    float* o = dg + row * ldg + (long)dir * H4 + u;
    o[0] = dc * gg * ig * (1.f - ig);
    o[H] = dc * cp * fg * (1.f - fg);
    o[2 * H] = dc * ig * (1.f - gg * gg);
    o[3 * H] = dh * tc * og * (1.f - og);
    *dcp = dc * fg;
  } else {
    float* o = dg + (b * sb + (long)step * st) * ldg + (long)dir * H4 + u;   // padding position t = step
    o[0] = 0.f;
    o[H] = 0.f;
    o[2 * H] = 0.f;
    o[3 * H] = 0.f;
  }
}

int check_shape(const char* fn, int B, int T, long sb, long st, int H, int ndir) {
  if (!(B >= 1 && T >= 1 && (ndir == 1 || ndir == 2)))
    return cfm::fail(CFM_ERR_ARG, std::string(fn) + ": B >= 1, T >= 1, ndir 1 or 2");
  if (!(H >= kUnits && H % kUnits == 0 && H <= kMaxH))
    return cfm::fail(CFM_ERR_SHAPE, std::string(fn) + ": hidden size: multiple of 8, <= 1024");
  // the rows b*stride_b + t*stride_t must be exactly the B*T rows of the arrays
  if (!(sb >= 1 && st >= 1 && (B - 1) * sb + (T - 1) * st == (long)B * T - 1))
    return cfm::fail(CFM_ERR_SHAPE, std::string(fn) + ": strides must address the B*T rows (batch- or time-major)");
  return CFM_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

void step_grid(int B, int H, int ndir, dim3* grid, dim3* block) {
  *grid = dim3(H / kUnits, ndir, cdiv(B, kSeq));
  *block = dim3(64 * kWaves);
}

}  // namespace

// the backward's cell-gradient carry, (B, ndir*H) fp32; the forward needs no workspace
CFM_EXPORT size_t cfm_lstm_batched_ws_bytes(int B, int T, int H, int ndir) {
  (void)T;
  if (B < 1 || H < 1 || ndir < 1) return 0;
  return (size_t)B * ndir * H * sizeof(float);
}

CFM_EXPORT int cfm_lstm_batched_fwd(const float* gx, const float* whh, const int32_t* lengths, float* y, float* gates,
                                    float* c, float* hprev, int B, int T, long stride_b, long stride_t, int H,
                                    int ndir, void* ws, void* stream) {
  (void)ws;
  CFM_REQUIRE(gx && whh && y && gates && c, CFM_ERR_ARG, "null pointer");
  if (int rc = check_shape(__func__, B, T, stride_b, stride_t, H, ndir)) return rc;
  CFM_REQUIRE(aligned16(whh) && aligned16(y), CFM_ERR_ALIGN, "whh and y 16-B aligned");
  hipStream_t s = cfm::as_stream(stream);
  dim3 grid, block;
  step_grid(B, H, ndir, &grid, &block);
  for (int step = 0; step < T; ++step)
    hipLaunchKernelGGL(lstm_batched_fwd_step, grid, block, 0, s, gx, whh, lengths, y, gates, c, hprev, B, T, stride_b,
                       stride_t, H, ndir, step);
  return cfm::check_launch("cfm_lstm_batched_fwd");
}

CFM_EXPORT int cfm_lstm_batched_bwd(const float* dy, const float* whh_t, const float* gates, const float* c,
                                    const int32_t* lengths, float* dg, int B, int T, long stride_b, long stride_t,
                                    int H, int ndir, void* ws, void* stream) {
  CFM_REQUIRE(dy && whh_t && gates && c && dg && ws, CFM_ERR_ARG, "null pointer");
  if (int rc = check_shape(__func__, B, T, stride_b, stride_t, H, ndir)) return rc;
  CFM_REQUIRE(aligned16(whh_t) && aligned16(dg), CFM_ERR_ALIGN, "whh_t and dg 16-B aligned");
  CFM_REQUIRE(((uintptr_t)ws & 3) == 0, CFM_ERR_ALIGN, "ws 4-B aligned");
  hipStream_t s = cfm::as_stream(stream);
  dim3 grid, block;
  step_grid(B, H, ndir, &grid, &block);
  for (int step = T - 1; step >= 0; --step)
    hipLaunchKernelGGL(lstm_batched_bwd_step, grid, block, 0, s, dy, whh_t, gates, c, lengths, dg, (float*)ws, B, T,
                       stride_b, stride_t, H, ndir, step);
  return cfm::check_launch("cfm_lstm_batched_bwd");
}
