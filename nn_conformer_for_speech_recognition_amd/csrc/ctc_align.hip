// ctc_align.hip — CTC forced alignment on the device: the best single alignment (Viterbi path) of a given
// transcript, the fourth CTC operation beside the loss, the greedy decode and the beam search.  The surface is
// modelled on torchaudio.functional.forced_align, batched, with per-token spans.
//
// Kernels (B utterances, T frames, V classes, L_b target labels, S_b = 2 L_b + 1 states: blank, l1, blank, ...):
//   align_prep       one wave per frame row: m = max, sum = sum exp(x - m) of the logits row; lpe[b,t,s] = (logit of
//                    the s-th extended label - m) - log(sum): the log-softmax ctc_prep of ctc.hip produces, in the
//                    form whose roundings scale with the result (the row sweep is ctc_common.h's prep_row; the
//                    last expression is this kernel's)                                        HBM: one row read
//   align_viterbi    one workgroup per utterance, one state per thread, the time loop sequential: the max-plus
//                    recursion v[t,s] = lpe[t,s] + max(v[t-1,s], v[t-1,s-1], v[t-1,s-2] if allowed) with the chosen
//                    move (0 stay, 1 from s-1, 2 from s-2) stored per (t, s) as one byte.  <true>: S <= 64, one wave,
//                    the neighbours by DPP wave shifts, no LDS and no barrier.  <false>: block = S rounded up to 64,
//                    the previous frame's row double-buffered in LDS, one workgroup barrier per frame.  No loop waits
//                    on a value another wave writes: every trip count is a function of T_b and S alone.
//   align_backtrace  one wave per utterance (a launch of its own, so the moves are visible without in-kernel fences):
//                    follows the moves from the end state back to frame 0 in chunks of 32 frames -- the state drops by
//                    at most 2 per frame, so the 64 states at and below the chunk's entry state cover every move the
//                    chunk can need: each lane loads its state's 32 moves (independent loads) and the wave-uniform walk
//                    reads them with v_readlane instead of one dependent global load per frame.  Lane f of the chunk
//                    then writes frame t's label and score and, where a span starts or ends there, the span's edge;
//                    the per-token sums follow in frame order, one thread per token (no atomics: deterministic).
// Tie rule (part of the contract): equal predecessors prefer stay, then s-1, then s-2; at the end the final blank
// S_b-1 wins a tie against S_b-2.
#include "ctc_common.h"

using namespace ctc;

namespace {

constexpr int VT_NT = CTC_MAX_STATES;   // largest block of the recursion
constexpr int BT_F = 32;      // frames per chunk of the backtrace: the state drops by <= 2 (BT_F - 1) = 62 < 64

struct AlignP : CtcView {
  float* lpe;                         // (B, T, S)
  int32_t* end_state;                 // (B) state of the last frame; -1: no alignment (infeasible)
  uint8_t* moves;                     // (B, T, S) 0 stay / 1 from s-1 / 2 from s-2
};

// ---------------------------------------------------------------------------------- emissions
__global__ __launch_bounds__(256) void align_prep(AlignP p) {
  // (x - m) - log(sum), not x - (m + log(sum)): both terms are <= 0 and no larger than the result, so every rounding is
  // relative to the log-probability itself; through lse = m + log(sum) it would be relative to |lse|, which for raw
  // logits with an offset is far above a confident frame's log-probability (and above a short path's whole score)
  prep_row(p, p.lpe, nullptr, [](float x, float m, float ls) { return (x - m) - ls; });
}

// ---------------------------------------------------------------------------------- Viterbi recursion
// blockIdx.x = utterance.  ONE: 64 threads, else blockDim.x = S rounded up to 64 (<= 1024).
template <bool ONE>
__global__ __launch_bounds__(ONE ? 64 : VT_NT) void align_viterbi(AlignP p, float* __restrict__ score) {
  // previous frame's row, double-buffered, two -inf pads in front so that s - 1 and s - 2 need no bounds test
  __shared__ float rowbuf[ONE ? 1 : 2][ONE ? 1 : VT_NT + 2];
  const int b = blockIdx.x, s = threadIdx.x, lane = s & 63;
  const int Tb = in_len_of(p, b), L = tgt_len_of(p, b), Sb = 2 * L + 1;
  const int32_t* tg = tgt_of(p, b);
  const bool valid = s < Sb;
  const int sc = min(s, Sb - 1);
  const bool odd = valid && (s & 1) && s >= 3;
  const bool skip = odd && ext_label(p, tg, s) != ext_label(p, tg, s - 2);   // s - 2 -> s allowed (s == 1: no s - 2)
  // a label equal to its predecessor needs a blank frame between the two: T_b >= L_b + repeats or no alignment
  int reps;
  if (ONE) reps = __popcll(__ballot(odd && !skip));
  else reps = __syncthreads_count(odd && !skip);
  if (Tb < L + reps || Tb <= 0) {   // uniform over the workgroup (T_b == 0: feasible only with no labels, score 0)
    if (s == 0) {
      const bool empty_ok = Tb <= 0 && L == 0;
      score[b] = empty_ok ? 0.f : NEG_INF;
      p.end_state[b] = empty_ok ? 0 : -1;
    }
    return;
  }
  const float* lp = p.lpe + (long)b * p.T * p.S;
  uint8_t* mv_out = p.moves + (long)b * p.T * p.S;
  if (!ONE) {
    if (s < 2) rowbuf[0][s] = rowbuf[1][s] = NEG_INF;
  }
  // lpe of this state, PF frames per block prefetched one block ahead (unconditional clamped loads)
  float cur[PF], nxt[PF];
  auto frame = [](int i) { return i; };
  float prev = NEG_INF;
  fetch_lpe(cur, lp, p.S, sc, 0, Tb, frame);
  for (int i0 = 0; i0 < Tb; i0 += PF) {
    fetch_lpe(nxt, lp, p.S, sc, min(i0 + PF, Tb - 1), Tb, frame);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int i = i0 + q;
      const bool live = i < Tb;   // uniform; steps past the utterance in the last block change nothing
      float n1, n2;
      if (ONE) {
        // lane l <- lane l - 1 (wave_shr; the shifted-in lanes are set to -inf)
        n1 = wave_shr1(prev);
        n2 = wave_shr1(n1);
        n1 = lane < 1 ? NEG_INF : n1;
        n2 = lane < 2 ? NEG_INF : n2;
      } else {
        const float* r = rowbuf[i & 1];   // written in frame i - 1 (frame 0 does not use it)
        n1 = r[s + 1];
        n2 = r[s];
      }
      // stay, then s - 1, then s - 2: a later candidate must be strictly better
      float best = prev;
      int mv = 0;
      if (n1 > best) { best = n1; mv = 1; }
      if (skip && n2 > best) { best = n2; mv = 2; }
      float v = best + cur[q];
      if (i == 0) { v = s <= 1 ? cur[q] : NEG_INF; mv = 0; }
      if (!valid) v = NEG_INF;
      if (live && valid) mv_out[(long)i * p.S + s] = (uint8_t)mv;
      prev = live ? v : prev;
      if (!ONE) {
        if (live) rowbuf[(i + 1) & 1][s + 2] = v;
        lds_barrier();   // frame i's row is complete; its readers are done with the other buffer
      }
    }
#pragma unroll
    for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
  }
  float fa, fb;   // the final blank S_b - 1 and the last label S_b - 2
  if (ONE) {
    fa = __shfl(prev, Sb - 1, 64);
    fb = __shfl(prev, max(Sb - 2, 0), 64);
  } else {
    const float* r = rowbuf[Tb & 1];   // frame T_b - 1's row (the last barrier of the loop made it visible)
    fa = r[Sb - 1 + 2];
    fb = r[max(Sb - 2, 0) + 2];
  }
  if (s == 0) {
    const bool last_label = Sb >= 2 && fb > fa;   // a tie goes to the final blank
    const float best = last_label ? fb : fa;
    const bool ok = best > NEG_INF;               // false for -inf and NaN (non-finite logits): no alignment
    score[b] = ok ? best : NEG_INF;
    p.end_state[b] = ok ? (last_label ? Sb - 2 : Sb - 1) : -1;
  }
}

// ---------------------------------------------------------------------------------- backtrace, outputs, spans
__global__ __launch_bounds__(64) void align_backtrace(AlignP p, int32_t* __restrict__ alignments,
                                                      float* __restrict__ scores, int32_t* __restrict__ starts,
                                                      int32_t* __restrict__ ends, float* __restrict__ token_scores) {
  extern __shared__ int32_t span[];   // [2][Smax]: starts, ends (only with span outputs)
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = in_len_of(p, b), L = tgt_len_of(p, b), Sb = 2 * L + 1;
  const int32_t* tg = tgt_of(p, b);
  const int e = p.end_state[b];
  const bool ok = e >= 0 && Tb > 0;
  const int Tv = ok ? Tb : 0;   // frames that carry an alignment
  int32_t* al = alignments + (long)b * p.T;
  float* sco = scores + (long)b * p.T;
  for (int t = Tv + lane; t < p.T; t += 64) { al[t] = -1; sco[t] = 0.f; }
  const bool spans = starts != nullptr;
  if (spans) {
    for (int u = lane; u < p.Smax; u += 64) { span[u] = -1; span[p.Smax + u] = -1; }
    __syncthreads();
  }
  const float* lp = p.lpe + (long)b * p.T * p.S;
  const uint8_t* mvs = p.moves + (long)b * p.T * p.S;
  int s = __builtin_amdgcn_readfirstlane(min(max(e, 0), Sb - 1));   // state of frame t_hi (wave-uniform)
  int s_next = -1;                                                   // state of frame t_hi + 1 (-1: none)
  for (int t_hi = Tv - 1; t_hi >= 0; t_hi -= BT_F) {
    // lane l holds state base + l of the chunk's frames t_hi, t_hi - 1, ...: s >= s_hi - 62 = base + 1 throughout
    const int base = s - 63;
    const int sl = min(max(base + lane, 0), Sb - 1);
    int m[BT_F];
#pragma unroll
    for (int f = 0; f < BT_F; ++f) m[f] = t_hi - f >= 0 ? (int)mvs[(long)(t_hi - f) * p.S + sl] : 0;
    int my_s = 0;
    bool my_start = false, my_end = false;
#pragma unroll
    for (int f = 0; f < BT_F; ++f) {
      const int t = t_hi - f;
      const bool live = t >= 0;   // uniform; steps before frame 0 in the last chunk change nothing
      int mv = __builtin_amdgcn_readlane(m[f], __builtin_amdgcn_readfirstlane(min(max(s - base, 0), 63)));
      if (mv > 2 || t <= 0) mv = 0;   // anything but 0 / 1 / 2 counts as stay
      const bool is_label = s & 1;
      if (lane == f) {
        my_s = s;
        my_start = is_label && (t == 0 || mv != 0);
        my_end = is_label && s_next != s;
      }
      s_next = live ? s : s_next;
      s = __builtin_amdgcn_readfirstlane(max(s - mv, 0));
    }
    const int t = t_hi - lane;
    if (lane < BT_F && t >= 0) {
      al[t] = ext_label(p, tg, my_s);
      sco[t] = lp[(long)t * p.S + my_s];
      if (spans && my_start) span[my_s >> 1] = t;
      if (spans && my_end) span[p.Smax + (my_s >> 1)] = t + 1;
    }
  }
  if (!spans) return;
  __syncthreads();
  for (int u = lane; u < p.Smax; u += 64) {
    int t0 = span[u], t1 = span[p.Smax + u];
    if (u >= L || !ok || t0 < 0 || t1 < 0) t0 = t1 = -1;   // a label the path never visits (a corrupted move table)
    t0 = min(t0, Tv);
    t1 = min(t1, Tv);
    float acc = 0.f;
    for (int t = t0; t < t1 && t0 >= 0; ++t) acc += lp[(long)t * p.S + 2 * u + 1];   // frame order, one thread
    const long o = (long)b * p.Smax + u;
    starts[o] = t0;
    ends[o] = t1;
    token_scores[o] = acc;
  }
}

struct AlignWs { size_t lpe, end_state, moves, total; };
AlignWs align_ws(int B, int T, int Smax) {
  const size_t bts = (size_t)B * T * (2 * (size_t)Smax + 1);
  AlignWs w;
  w.lpe = 0;
  w.end_state = sizeof(float) * bts;
  w.moves = w.end_state + sizeof(int32_t) * (size_t)B;
  w.total = (w.moves + bts + 15) & ~(size_t)15;
  return w;
}

}  // namespace

CFM_EXPORT size_t cfm_ctc_align_ws_bytes(int B, int T, int Smax) {
  if (B <= 0 || T <= 0 || Smax < 0) return 0;
  return align_ws(B, T, Smax).total;
}

CFM_EXPORT int cfm_ctc_forced_align(const float* logits, long sb, long st, const int32_t* targets, int ldt,
                                    const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int B, int T,
                                    int V, int Smax, int blank, int32_t* alignments, float* scores, float* score,
                                    int32_t* starts, int32_t* ends, float* token_scores, void* ws, void* stream) {
  CFM_REQUIRE(logits && in_len && tgt_len && alignments && scores && score && ws, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(targets || Smax == 0, CFM_ERR_ARG, "null targets");
  CFM_REQUIRE((starts != nullptr) == (ends != nullptr) && (ends != nullptr) == (token_scores != nullptr), CFM_ERR_ARG,
              "starts, ends and token_scores: all three or none");
  AlignP p;
  static_cast<CtcView&>(p) = make_view(logits, sb, st, targets, ldt, tgt_off, in_len, tgt_len, B, T, V, Smax, blank);
  if (const int rc = check_ctc_problem(__func__, p)) return rc;
  const int S = p.S;
  hipStream_t s = cfm::as_stream(stream);
  const AlignWs w = align_ws(B, T, Smax);
  char* base = static_cast<char*>(ws);
  p.lpe = reinterpret_cast<float*>(base + w.lpe);
  p.end_state = reinterpret_cast<int32_t*>(base + w.end_state);
  p.moves = reinterpret_cast<uint8_t*>(base + w.moves);
  hipLaunchKernelGGL(align_prep, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), 0, s, p);
  if (S <= 64) hipLaunchKernelGGL(align_viterbi<true>, dim3(B), dim3(64), 0, s, p, score);
  else hipLaunchKernelGGL(align_viterbi<false>, dim3(B), dim3((S + 63) & ~63), 0, s, p, score);
  const size_t sh = starts ? 2 * (size_t)Smax * sizeof(int32_t) : 0;
  hipLaunchKernelGGL(align_backtrace, dim3(B), dim3(64), sh, s, p, alignments, scores, starts, ends, token_scores);
  return cfm::check_launch("cfm_ctc_forced_align");
}
