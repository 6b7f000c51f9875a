// ctc_common.h — what the CTC-side kernels share (ctc.hip, ctc_align.hip, ctc_beam.hip, ctc_nbest.hip, edit_distance.hip): the
// problem view with its clamped accessors, the emission prep's row sweep, the lpe prefetch of the recursions, and
// the host-side argument check.  A new CTC-side kernel includes this, derives its parameter struct from CtcView
// and adds no clamp of its own ("CTC family: the shared header").
#pragma once

#include "cfm_common.h"

#include <math.h>

namespace ctc {

constexpr float NEG_INF = -INFINITY;
constexpr int PF = 16;               // frames of lpe prefetched per chunk
constexpr int CTC_MAX_STATES = 1024; // one state per thread of the recursions' largest block: 2 * 511 + 1 states

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == NEG_INF) return NEG_INF;
  return m + logf(expf(a - m) + expf(b - m));
}

// ---------------------------------------------------------------------------------- clamps
// The one clamp of device-side lengths and labels: v into [0, hi].
__device__ __forceinline__ int clamp0(int v, int hi) { return min(max(v, 0), hi); }
// length of row b, clamped to [0, T]; null lens: every row is T long
__device__ __forceinline__ int clamp_len(const int32_t* lens, int b, int T) { return lens ? clamp0(lens[b], T) : T; }

// ---------------------------------------------------------------------------------- the problem
// One CTC problem as the loss and the aligner see it; their parameter structs derive from it and add their work
// arrays.
struct CtcView {
  const float* logits; long sb, st;   // row (b, t) at logits + b*sb + t*st (batch- or time-major)
  const int32_t* tgt; int ldt;        // targets: utterance b at tgt + (off ? off[b] : b*ldt)
  const int32_t* off;
  const int32_t* in_len; const int32_t* tgt_len;
  int B, T, V, Smax, S;               // S = 2*Smax + 1 (state stride of the work arrays)
  int blank;
};

__device__ __forceinline__ const int32_t* tgt_of(const CtcView& p, int b) {
  return p.tgt + (p.off ? (long)p.off[b] : (long)b * p.ldt);
}
// lengths are device data: clamp to the buffers' extents (in_len <= T, tgt_len <= Smax) so that a bad
// length can only give a wrong loss, never an access outside lpe / alpha / beta / sh[] (torch raises
// on such inputs; the host wrapper validates host-side lengths the same way).  The same holds for every user of
// the view: a bad device length or label can give a wrong answer, never an access outside logits / the work arrays /
// the outputs.  (in_len and tgt_len are never null: the entry points require them.)
__device__ __forceinline__ int in_len_of(const CtcView& p, int b) { return clamp0(p.in_len[b], p.T); }
__device__ __forceinline__ int tgt_len_of(const CtcView& p, int b) { return clamp0(p.tgt_len[b], p.Smax); }
// label u of an utterance, clamped to the class range (an out-of-range id would index x / corr[] out of bounds)
__device__ __forceinline__ int label_of(const CtcView& p, const int32_t* tg, int u) { return clamp0(tg[u], p.V - 1); }
// extended label of state s (blank, l1, blank, l2, ...)
__device__ __forceinline__ int ext_label(const CtcView& p, const int32_t* tg, int s) { return (s & 1) ? label_of(p, tg, s >> 1) : p.blank; }

// ---------------------------------------------------------------------------------- emission prep
// One wave per frame row (256 threads, four rows per workgroup): m = max and s = sum exp(x - m) of the logits row,
// then lpe[row, st] = emit(logit of the st-th extended label, m, log s) for the utterance's states; with lse_out the
// row's m + log s is stored too.  The two callers differ in emit alone (their roundings differ on purpose).
// beam_topk has a sweep of its own: it stages the row in LDS and sums in double.
// row_stats is the sweep alone (m and ls = log s of the row at x, the whole wave taking part), for a caller that
// writes the emissions of several label sequences from one sweep (ctc_nbest.hip).
__device__ __forceinline__ void row_stats(const CtcView& p, const float* x, int lane, float& m, float& ls) {
  m = NEG_INF;
  const bool v4 = (p.V % 4 == 0) && (p.sb % 4 == 0) && (p.st % 4 == 0) && ((uintptr_t)p.logits % 16 == 0);
  if (v4) {
    for (int v = lane * 4; v < p.V; v += 256) {
      const float4 q = *reinterpret_cast<const float4*>(x + v);
      m = fmaxf(m, fmaxf(fmaxf(q.x, q.y), fmaxf(q.z, q.w)));
    }
  } else {
    for (int v = lane; v < p.V; v += 64) m = fmaxf(m, x[v]);
  }
  m = wave_max(m);
  float s = 0.f;
  if (v4) {
    for (int v = lane * 4; v < p.V; v += 256) {
      const float4 q = *reinterpret_cast<const float4*>(x + v);
      s += expf(q.x - m) + expf(q.y - m) + expf(q.z - m) + expf(q.w - m);
    }
  } else {
    for (int v = lane; v < p.V; v += 64) s += expf(x[v] - m);
  }
  s = wave_sum(s);
  ls = logf(s);
}

template <typename Emit>
__device__ __forceinline__ void prep_row(const CtcView& p, float* lpe, float* lse_out, Emit emit) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)p.B * p.T) return;
  const int b = (int)(row / p.T), t = (int)(row % p.T);
  if (t >= in_len_of(p, b)) return;
  const float* x = p.logits + b * p.sb + t * p.st;
  float m, ls;
  row_stats(p, x, lane, m, ls);
  if (lse_out && lane == 0) lse_out[row] = m + ls;
  const int Sb = 2 * tgt_len_of(p, b) + 1;
  const int32_t* tg = tgt_of(p, b);
  float* dst = lpe + row * p.S;
  for (int st = lane; st < Sb; st += 64) dst[st] = emit(x[ext_label(p, tg, st)], m, ls);
}

// ---------------------------------------------------------------------------------- lpe prefetch
// lpe of state sc for the PF steps i0 .. i0 + PF - 1 of a recursion over n steps, step i at frame(i) (alpha and
// Viterbi: i, beta: n - 1 - i): unconditional loads, the step clamped to n - 1.  The recursions fetch one block ahead.
template <typename Frame>
__device__ __forceinline__ void fetch_lpe(float (&r)[PF], const float* lp, int S, int sc, int i0, int n, Frame frame) {
#pragma unroll
  for (int q = 0; q < PF; ++q) r[q] = lp[(long)frame(min(i0 + q, n - 1)) * S + sc];
}

// ---------------------------------------------------------------------------------- host side
inline CtcView make_view(const float* logits, long sb, long st, const int32_t* targets, int ldt, const int32_t* off,
                         const int32_t* in_len, const int32_t* tgt_len, int B, int T, int V, int Smax, int blank) {
  CtcView p;
  p.logits = logits; p.sb = sb; p.st = st; p.tgt = targets; p.ldt = ldt; p.off = off;
  p.in_len = in_len; p.tgt_len = tgt_len;
  p.B = B; p.T = T; p.V = V; p.Smax = Smax; p.S = 2 * Smax + 1; p.blank = blank;
  return p;
}

// What every entry point that takes a CtcView requires of it (fn: the entry point's name, for the message).
inline int check_ctc_problem(const char* fn, const CtcView& p) {
  CFM_REQUIRE_FN(fn, p.B > 0 && p.T > 0 && p.V > 0 && p.Smax >= 0 && (p.off || p.ldt >= p.Smax), CFM_ERR_SHAPE,
                 "bad shape");
  CFM_REQUIRE_FN(fn, p.blank >= 0 && p.blank < p.V, CFM_ERR_ARG, "blank out of range");
  CFM_REQUIRE_FN(fn, p.S <= CTC_MAX_STATES, CFM_ERR_UNSUPPORTED, "target length must be <= 511");
  return CFM_OK;
}

}  // namespace ctc
