// rnnt_greedy.hip — time-synchronous greedy search of a transducer head (transducer.TransducerHead), one launch.
//
// B utterances, T frames, V classes, prediction LSTM of H units, joint width J.  Inputs, fp32 contiguous:
//   ep (B, T, J) = enc_proj(enc) with bias;  gtab (V, 4H) = embedding.weight W_ih^T + b_ih + b_hh (the cell's input
//   half is a table row: the prediction network's input is a token id);  w_hh (4H, H);  w_pp (J, H), b_pp (J);
//   w_out (V, J), b_out (V);  lengths (B) int32 or null (T).
// Per utterance, T_b = ctc_common.h's clamp of lengths[b] to [0, T]:
//   (h, c) = cell(0, 0, gtab[blank]);  pp = w_pp h + b_pp
//   for t < T_b, at most max_symbols times:
//     logits = w_out tanh(ep[b,t] + pp) + b_out;  tok = argmax (ties: the lowest index, torch's rule)
//     score += log_softmax(logits)[tok]      ((x - m) - log sum exp(x - m) in fp32, the sum over decisions in double)
//     tok == blank: next frame.  else: emit tok at frame t; with W tokens emitted the utterance stops there;
//     (h, c) = cell(h, c, gtab[tok]) (gates = gtab[tok] + w_hh h, order i, f, g, o, lstm.hip's sigm / tanh_f); pp again
// A frame closed by the max_symbols cap adds no blank term.  Outputs: tokens, frames (B, W) int32 padded with -1,
// counts (B) int32, scores (B) fp32; every element is written.
//
// Kernel: rnnt_greedy<V4>, ONE WORKGROUP of 512 threads PER UTTERANCE (the search is a serial chain of decisions
// within an utterance, utterances are independent; B workgroups occupy B compute units, so the kernel is bound by the
// LATENCY of the chain matvec -> argmax -> (cell -> matvec), not by occupancy).  Every matvec is WAVE-PER-ROW over the
// row-major weights: wave w takes the rows w, w + 8, ..; RB = 8 rows are loaded per pass before any is reduced (64 KB
// in flight per compute unit at K = 256), each lane multiplies its K / 64 columns against the vector it holds in REGISTERS
// (h from LDS; z = tanh(ep + pp) is formed in registers by every wave, so z needs no LDS and no barrier), then one
// xor butterfly per row; the row's bias (b_out, b_pp, or the row of gtab[tok]) is loaded beside the weights by lane
// rb and added after the butterfly.  The logits are not stored: a wave parks its rows' logits in one lane each and
// folds them, 64 at a time, into per-lane running (max, sum exp, argmax); lanes, then waves (through LDS) are merged
// in a fixed order, so any V works.  h, c, the gates, pp and two rows of ep (the next frame's is fetched a frame ahead)
// live in LDS (36 KB).
// Bound: per blank decision one L2-hit sweep of w_out (V J 4 bytes) and one barrier; per emitted token also w_hh and
// w_pp ((4H + J) H 4 bytes: 1.25 MB at H = J = 256, about 7 us at the 64 B / clk one compute unit reads from L2) and
// three barriers.  Measured (profiles/rnnt_greedy/times.txt): 7 us per blank decision at V = 64 and 28 us
// at V = 1024 -- the instructions around the sweep (a butterfly per row, the tanh of all 16 register slots, the exp of
// the merges), not the sweep, set the time; 8x to 66x the torch loop all the same.
//
// Properties:
//   * No hang is possible.  No communication between workgroups, no atomics, no spin, no cooperative launch.  Every
//     barrier sits in workgroup-uniform control flow: the branches around barriers test T_b, the loop counters, the
//     token count n and the chosen token, and the chosen token is computed by EVERY thread from the same per-wave
//     partials, which are published to LDS and read after a barrier, before anyone branches on it.  Trip counts are
//     bounded by T_b * max_symbols, known from the clamped inputs.
//   * No out-of-bounds access from bad lengths (clamped); the argmax result is in [0, V) by construction (a row
//     index, 0 if nothing compares greater, e.g. all NaN), the emitted count never exceeds W.
//   * No host synchronisation; graph-capturable on one stream.  Two runs are bit-identical.
//   * A logit's operation order depends on neither its row index v nor the utterance's place in the batch: the same
//     lane takes the same columns in the same order for every row (explicit fmaf), then the same butterfly, then
//     + bias.  Two identical rows of w_out with identical biases give bit-equal logits.
//   * Limits: H <= 1024 with H % 8 == 0, J <= 1024, V >= 2 (any, by looping); outside them the entry point returns
//     CFM_ERR_UNSUPPORTED without launching.  V4 (float4 loads) needs J % 4 == 0 and 16-byte aligned ep / w_hh / w_pp /
//     w_out; otherwise every load is a scalar one (a choice per launch, never per row).
#include "ctc_common.h"

using namespace ctc;

namespace {

constexpr int GR_THREADS = 512;    // 8 waves, two per SIMD: up to 256 VGPRs each, so 8 rows in flight spill nothing
constexpr int GR_WAVES = GR_THREADS / 64;
constexpr int GR_MAX = 1024;   // H and J: a lane holds 16 columns of the vector
constexpr int EPT = GR_MAX / GR_THREADS;   // columns of an ep row per thread
constexpr int RB = 8;          // rows in flight per wave

// the sigm / tanh_f forms of lstm.hip
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  const float e = __expf(-2.f * fabsf(x));
  const float r = (1.f - e) / (1.f + e);
  return copysignf(r, x);
}

struct GreedyP {
  const float *ep, *gtab, *w_hh, *w_pp, *b_pp, *w_out, *b_out;
  const int32_t* lengths;
  int32_t *tokens, *frames, *counts;
  float* scores;
  int B, T, V, H, J, blank, max_symbols, W;
};

// The lane's columns of a K-vector: V4: x[4i + c] = src[lane * 4 + 256 i + c], else x[i] = src[lane + 64 i]; zero past K.
template <bool V4>
__device__ __forceinline__ void load_x(float (&x)[16], const float* src, int K, int lane) {
  if (V4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = lane * 4 + 256 * i;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < K) v = *reinterpret_cast<const float4*>(src + k);
      x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = lane + 64 * i;
      x[i] = k < K ? src[k] : 0.f;
    }
  }
}

// y[r] = W[r, :] . x + bias[r] for the wave's rows r = wave + GR_WAVES * j, j = 0, 1, ..; emit(j, r, y) is called by
// the whole wave (y is the same in every lane) for each row r < rows, j ascending.  Loads are unconditional at
// clamped addresses (no branch between the loads of a pass); what lies past the row count or past K is masked out.
template <bool V4, typename Emit>
__device__ __forceinline__ void matvec(const float* __restrict__ W, const float* __restrict__ bias, int rows, int K,
                                       const float (&x)[16], int wave, int lane, Emit emit) {
  const int ni = V4 ? (K + 255) >> 8 : (K + 63) >> 6;
  for (int j0 = 0; wave + GR_WAVES * j0 < rows; j0 += RB) {
    const int rl = wave + GR_WAVES * (j0 + lane);
    const float bv = (lane < RB && rl < rows) ? bias[rl] : 0.f;
    const float* wr[RB];
    float acc[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      wr[rb] = W + (long)min(wave + GR_WAVES * (j0 + rb), rows - 1) * K;
      acc[rb] = 0.f;
    }
    if (V4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < ni) {   // uniform
          const int k = lane * 4 + 256 * i;
          const bool ok = k < K;
          const int kc = min(k, K - 4);
          float4 w[RB];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) w[rb] = *reinterpret_cast<const float4*>(wr[rb] + kc);
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) {
            float a = acc[rb];
            a = fmaf(w[rb].x, x[4 * i], a);
            a = fmaf(w[rb].y, x[4 * i + 1], a);
            a = fmaf(w[rb].z, x[4 * i + 2], a);
            a = fmaf(w[rb].w, x[4 * i + 3], a);
            acc[rb] = ok ? a : acc[rb];
          }
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i < ni) {   // uniform
          const int k = lane + 64 * i;
          const bool ok = k < K;
          const int kc = min(k, K - 1);
          float w[RB];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) w[rb] = wr[rb][kc];
#pragma unroll
          for (int rb = 0; rb < RB; ++rb) acc[rb] = ok ? fmaf(w[rb], x[i], acc[rb]) : acc[rb];
        }
      }
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb] = wave_sum(acc[rb]);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int r = wave + GR_WAVES * (j0 + rb);
      if (r < rows) emit(j0 + rb, r, acc[rb] + __shfl(bv, rb, 64));   // uniform
    }
  }
}

// a lane's running (max, sum exp(x - max), best value, its row) over the logits it has been handed
struct Run {
  float m, s, best;
  int idx;
};
__device__ __forceinline__ void run_add(Run& q, float x, int r) {
  if (x > q.best) {   // rows reach a lane in ascending order: strict > keeps the lowest index of a tie
    q.best = x;
    q.idx = r;
  }
  if (x > q.m) {
    q.s = (q.m == NEG_INF ? 0.f : q.s * expf(q.m - x)) + 1.f;
    q.m = x;
  } else {
    q.s += expf(x - q.m);
  }
}
// b into a: the sums rescaled to the larger max; the larger value wins, a tie goes to the lower row
__device__ __forceinline__ void run_merge(Run& a, const Run& b) {
  const float m = fmaxf(a.m, b.m);
  const float sa = a.m == NEG_INF ? 0.f : a.s * expf(a.m - m);
  const float sb = b.m == NEG_INF ? 0.f : b.s * expf(b.m - m);
  a.m = m;
  a.s = sa + sb;
  if (b.best > a.best || (b.best == a.best && b.idx < a.idx)) {
    a.best = b.best;
    a.idx = b.idx;
  }
}

template <bool V4>
__global__ __launch_bounds__(GR_THREADS) void rnnt_greedy(GreedyP p) {
  __shared__ __attribute__((aligned(16))) float sh_h[GR_MAX], sh_c[GR_MAX], sh_pp[GR_MAX], sh_g[4 * GR_MAX];
  // ep[b, t], double-buffered by the frame's parity: frame t + 1's row is loaded into a register when frame t begins
  // and parked here before the barrier of frame t's first decision
  __shared__ __attribute__((aligned(16))) float sh_ep[2][GR_MAX];
  // the waves' partial (max, sum, best, row) of a decision, double-buffered by the decision's parity: a wave may
  // write decision d + 1 while another still reads decision d (one barrier per decision)
  __shared__ float pm[2][GR_WAVES], ps[2][GR_WAVES], pb[2][GR_WAVES];
  __shared__ int pi[2][GR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: row addresses are formed on the scalar unit
  const int b = blockIdx.x, H = p.H, J = p.J;
  const int Tb = clamp_len(p.lengths, b, p.T);
  int32_t* tokens = p.tokens + (long)b * p.W;
  int32_t* frames = p.frames + (long)b * p.W;
  int n = 0;            // tokens emitted (the same in every thread)
  double score = 0.0;   // thread 0's

  // (h, c) <- cell(h, c, gtab[tok]); pp <- w_pp h + b_pp.  Three barriers, uniform.
  auto cell = [&](int tok) {
    float x[16];
    load_x<V4>(x, sh_h, H, lane);
    matvec<V4>(p.w_hh, p.gtab + (long)tok * 4 * H, 4 * H, H, x, wave, lane,
               [&](int, int r, float y) { if (lane == 0) sh_g[r] = y; });
    lds_barrier();   // the gates are complete; every wave holds its copy of the old h
    for (int u = tid; u < H; u += GR_THREADS) {
      const float ig = sigm(sh_g[u]), fg = sigm(sh_g[H + u]);
      const float gg = tanh_f(sh_g[2 * H + u]), og = sigm(sh_g[3 * H + u]);
      const float c = fg * sh_c[u] + ig * gg;
      sh_c[u] = c;
      sh_h[u] = og * tanh_f(c);
    }
    lds_barrier();   // the new h
    load_x<V4>(x, sh_h, H, lane);
    matvec<V4>(p.w_pp, p.b_pp, J, H, x, wave, lane, [&](int, int r, float y) { if (lane == 0) sh_pp[r] = y; });
    lds_barrier();   // the new pp
  };

  if (Tb > 0) {   // uniform
    for (int u = tid; u < H; u += GR_THREADS) {
      sh_h[u] = 0.f;
      sh_c[u] = 0.f;
    }
    const float* epb = p.ep + (long)b * p.T * J;
    for (int k = tid; k < J; k += GR_THREADS) sh_ep[0][k] = epb[k];
    lds_barrier();
    cell(p.blank);
    int d = 0;           // decisions taken
    bool full = false;   // W tokens emitted
    for (int t = 0; t < Tb && !full; ++t) {
      float epn[EPT];   // the next frame's row, ahead of its use
#pragma unroll
      for (int q = 0; q < EPT; ++q) {
        const int k = tid + q * GR_THREADS;
        epn[q] = k < J ? epb[(long)min(t + 1, Tb - 1) * J + k] : 0.f;
      }
      for (int sym = 0; sym < p.max_symbols; ++sym) {
        float z[16];
        {
          float e[16], q[16];
          load_x<V4>(e, sh_ep[t & 1], J, lane);
          load_x<V4>(q, sh_pp, J, lane);
#pragma unroll
          for (int i = 0; i < 16; ++i) z[i] = tanhf(e[i] + q[i]);   // (columns past J: tanh(0) = 0)
        }
        Run run = {NEG_INF, 0.f, NEG_INF, 0x7fffffff};
        float park = 0.f;
        auto fold = [&](int j) {   // the 64 parked logits of rows j - (j & 63) .. : one per lane
          const int r = wave + GR_WAVES * ((j & ~63) + lane);
          if (lane <= (j & 63) && r < p.V) run_add(run, park, r);
        };
        int last = -1;
        matvec<V4>(p.w_out, p.b_out, p.V, J, z, wave, lane, [&](int j, int, float y) {
          park = lane == (j & 63) ? y : park;
          last = j;
          if ((j & 63) == 63) fold(j);
        });
        if (last >= 0 && (last & 63) != 63) fold(last);
        // lanes -> wave (a fixed butterfly), wave -> LDS
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          Run other;
          other.m = __shfl_xor(run.m, o, 64);
          other.s = __shfl_xor(run.s, o, 64);
          other.best = __shfl_xor(run.best, o, 64);
          other.idx = __shfl_xor(run.idx, o, 64);
          run_merge(run, other);
        }
        const int buf = d & 1;
        if (lane == 0) {
          pm[buf][wave] = run.m;
          ps[buf][wave] = run.s;
          pb[buf][wave] = run.best;
          pi[buf][wave] = run.idx;
        }
        if (sym == 0) {   // last read in frame t - 1, barriers ago
#pragma unroll
          for (int q = 0; q < EPT; ++q) {
            const int k = tid + q * GR_THREADS;
            if (k < J) sh_ep[(t + 1) & 1][k] = epn[q];
          }
        }
        lds_barrier();   // the decision's partials (and the next frame's ep) are published
        Run all = {pm[buf][0], ps[buf][0], pb[buf][0], pi[buf][0]};
        for (int w = 1; w < GR_WAVES; ++w) {
          const Run other = {pm[buf][w], ps[buf][w], pb[buf][w], pi[buf][w]};
          run_merge(all, other);
        }
        // every thread now holds the same token, from the same LDS words in the same order
        const int tok = all.idx == 0x7fffffff ? 0 : min(all.idx, p.V - 1);
        ++d;
        if (tid == 0) score += (double)((all.best - all.m) - logf(all.s));
        if (tok == p.blank) break;
        if (tid == 0) {
          tokens[n] = tok;
          frames[n] = t;
        }
        ++n;
        if (n >= p.W) {
          full = true;
          break;
        }
        cell(tok);
      }
    }
  }
  for (int k = n + tid; k < p.W; k += GR_THREADS) {
    tokens[k] = -1;
    frames[k] = -1;
  }
  if (tid == 0) {
    p.counts[b] = n;
    p.scores[b] = (float)score;
  }
}

}  // namespace

CFM_EXPORT int cfm_rnnt_greedy(const float* ep, const float* gtab, const float* w_hh, const float* w_pp,
                               const float* b_pp, const float* w_out, const float* b_out, const int32_t* lengths,
                               int B, int T, int V, int H, int J, int blank, int max_symbols, int W, int32_t* tokens,
                               int32_t* frames, int32_t* counts, float* scores, void* stream) {
  CFM_REQUIRE(B > 0 && T > 0 && V > 0 && H > 0 && J > 0 && W > 0, CFM_ERR_SHAPE, "bad shape");
  CFM_REQUIRE(ep && gtab && w_hh && w_pp && b_pp && w_out && b_out && tokens && frames && counts && scores,
              CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(blank >= 0 && blank < V, CFM_ERR_ARG, "blank out of range");
  CFM_REQUIRE(max_symbols >= 1, CFM_ERR_ARG, "max_symbols must be >= 1");
  CFM_REQUIRE(V >= 2, CFM_ERR_UNSUPPORTED, "V must be >= 2");
  CFM_REQUIRE(H <= GR_MAX && H % 8 == 0, CFM_ERR_UNSUPPORTED, "H must be a multiple of 8, at most 1024");
  CFM_REQUIRE(J <= GR_MAX, CFM_ERR_UNSUPPORTED, "J must be at most 1024");
  CFM_REQUIRE((long)B * T * J <= 0x7fffffffL * 4 && (long)V * 4 * H <= 0x7fffffffL && (long)B * W <= 0x7fffffffL,
              CFM_ERR_UNSUPPORTED, "problem too large");
  GreedyP p = {ep, gtab, w_hh, w_pp, b_pp, w_out, b_out, lengths, tokens, frames, counts, scores,
               B, T, V, H, J, blank, max_symbols, W};
  const bool v4 = J % 4 == 0 && ((uintptr_t)ep | (uintptr_t)w_hh | (uintptr_t)w_pp | (uintptr_t)w_out) % 16 == 0;
  hipStream_t s = cfm::as_stream(stream);
  if (v4) hipLaunchKernelGGL(rnnt_greedy<true>, dim3(B), dim3(GR_THREADS), 0, s, p);
  else hipLaunchKernelGGL(rnnt_greedy<false>, dim3(B), dim3(GR_THREADS), 0, s, p);
  return cfm::check_launch("cfm_rnnt_greedy");
}
