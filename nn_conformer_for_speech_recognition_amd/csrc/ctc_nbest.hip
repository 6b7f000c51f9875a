// ctc_nbest.hip — the CTC likelihood of N hypotheses per utterance against the utterance's ONE emission matrix, and
// the gradient of a risk-weighted sum of them: the expected risk over an n-best list (MWER, Prabhavalkar et al. 2018).
//
// B utterances, T frames, V classes; J = B N problems, problem j = (b, n) = (j / N, j % N) reads the logits rows of
// utterance b and hypothesis row j (L_j labels, S_j = 2 L_j + 1 states: blank, l1, blank, ...).  A hypothesis whose
// length is negative (missing) or above max_labels takes no part: ll = -inf, post = 0, no gradient.
//
//   ll[j]    = log P_ctc(y_j | x_b) over all alignments (-inf: infeasible or not finite)
//   live     = present and ll finite;  post = softmax of ll over the live n;  rbar = mean of the risk over the live n
//   loss[b]  = sum_n post (r - rbar)  (0 with fewer than two live hypotheses)
//   c[j]     = post ((r - rbar) - loss[b]),  sum_n c = 0
//   dlogits[b, t, v] = g[b] sum_n c[j] occ_j[t, v]:  d ll_j / d x = occ_j - softmax(x) and the softmax term is
//              multiplied by sum_n c = 0, so it is never formed.  Non-zero only at the blank and at the labels of the
//              utterance's hypotheses.
//
// Kernels:
//   nbest_prep     one wave per frame row: the row's max and log-sum ONCE (ctc_common.h's row_stats), then
//                  lpe[j, t, s] = (x[label] - m) - log(sum) for every hypothesis of the utterance (the aligner's form:
//                  see align_prep)                                                              HBM: one row read
//   nbest_alpha    one workgroup per problem, one state per thread, the time loop sequential, as align_viterbi with the
//                  max replaced by a three-way log-sum-exp.  <64>: S <= 64, one wave, DPP shifts, no LDS, no barrier;
//                  <256> / <1024>: the previous row double-buffered in LDS, one barrier per frame (256: S <= 256, the
//                  common case, with twice the registers per thread).  Stores alpha[j, t, s] and ll.
//   nbest_weights  one wave per utterance: live mask, post, loss, c; every sum in n order.
//   nbest_beta     the same recursion backwards; writes the occupancy occ = exp(alpha + beta - lpe - ll) over
//                  lpe[j, t, s] (the same thread reads and writes a cell).  Problems with c == 0 are skipped.  Its
//                  prologue links the equal labels of the hypothesis into chains (first occurrence, next occurrence)
//                  for the gradient's per-class sums.
//   nbest_grad     one workgroup per (b, t) row writes the whole V-wide row: the class sums are kept in LDS; the
//                  hypotheses are added one after the other with a barrier between them, and within a hypothesis the
//                  thread of a label's FIRST occurrence adds its chain's occupancies in state order, so each class has
//                  one writer per hypothesis; the blank's states are summed per thread, then over the lanes, then over
//                  the waves in wave order.  No atomics anywhere: every sum's order is a function of the inputs alone.
// No loop waits on, or takes its trip count from, a value another wave writes in the same launch.
//
// Precision.  The recursions' STATE (alpha, beta, ll) is double, their exponentials and logarithms are fp32: a step is
// m + log(sum exp(v - m)) + lpe with m the largest of three states; the differences v - m are formed in double and
// are O(1), the fp32 functions see only them, and the sum m + log(...) + lpe is again double.  A step's error is then
// about 1e-7 whatever |alpha| is; with an fp32 state it is half an ulp of |alpha|, 1.2e-4 at the |log p| = 2.6e3 of a
// 373-frame utterance, which exp(alpha + beta - lpe - ll) turns into a relative error of the occupancy and the softmax
// over n into an error of post.  The price is a handful of double additions per frame and an 8-byte alpha.
#include "ctc_common.h"

using namespace ctc;

namespace {

constexpr int NBEST_MAX = 128;
constexpr int GR_NT = 256;              // threads of a gradient row
constexpr int GR_VC = 8192;             // classes per LDS pass of a gradient row
constexpr int CHAIN_FIRST = 1 << 16;    // chain word: next occurrence (0: none) | CHAIN_FIRST
constexpr double NEG_INF_D = -INFINITY;

// The view's B, T, in_len are the utterances'; its target rows are the J = B N hypotheses (row j at tgt + j ldt,
// tgt_len[j] labels).
struct NbestP : CtcView {
  int N;
  const float* risk;   // (J), nullable
  float* lpe;          // (J, T, S): the emissions after the forward, the occupancy after nbest_beta
  double* alpha;       // (J, T, S)
  float* ll;           // (J)
  float* post;         // (J)
  float* loss;         // (B), null without risk
  float* c;            // (J)
  double* llw;         // (J) the forward's ll, unrounded, for the weights and the backward
  int32_t* chain;      // (J, Smax)
};

// a hypothesis takes part when its length lies in [0, Smax]: negative is "missing", longer is over max_labels (its
// labels and states are still addressed through the clamped tgt_len_of)
__device__ __forceinline__ bool present(const NbestP& p, int j) {
  const int l = p.tgt_len[j];
  return l >= 0 && l <= p.Smax;
}

// log(exp(a) + exp(b) + exp(c)): double in and out, the functions in fp32 on the O(1) differences (header comment)
__device__ __forceinline__ double lse3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (m == NEG_INF_D) return NEG_INF_D;
  const float s = expf((float)(a - m)) + expf((float)(b - m)) + expf((float)(c - m));
  return m + (double)logf(s);
}

// the one-lane wave shifts of cfm_common.h on the two halves of a double (own names: an overload declared in this
// namespace would hide the int ones it is built from)
__device__ __forceinline__ double shr1_f64(double v) {
  const int hi = ::wave_shr1(__double2hiint(v)), lo = ::wave_shr1(__double2loint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shl1_f64(double v) {
  const int hi = ::wave_shl1(__double2hiint(v)), lo = ::wave_shl1(__double2loint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_bcast(double v, int lane) {
  return __hiloint2double(__shfl(__double2hiint(v), lane, 64), __shfl(__double2loint(v), lane, 64));
}

// ---------------------------------------------------------------------------------- emissions
__global__ __launch_bounds__(256) void nbest_prep(NbestP p) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)p.B * p.T) return;
  const int b = (int)(row / p.T), t = (int)(row % p.T);
  if (t >= in_len_of(p, b)) return;
  const float* x = p.logits + b * p.sb + t * p.st;
  float m, ls;
  row_stats(p, x, lane, m, ls);
  for (int n = 0; n < p.N; ++n) {
    const int j = b * p.N + n;
    if (!present(p, j)) continue;
    const int Sj = 2 * tgt_len_of(p, j) + 1;
    const int32_t* tg = tgt_of(p, j);
    float* dst = p.lpe + ((long)j * p.T + t) * p.S;
    // (x - m) - log(sum): every rounding relative to the log-probability itself (align_prep's comment)
    for (int st = lane; st < Sj; st += 64) dst[st] = (x[ext_label(p, tg, st)] - m) - ls;
  }
}

// ---------------------------------------------------------------------------------- alpha
// blockIdx.x = problem.  NT 64: one wave, else blockDim.x = S rounded up to 64 (<= NT).
template <int NT>
__global__ __launch_bounds__(NT) void nbest_alpha(NbestP p) {
  constexpr bool ONE = NT == 64;
  // previous frame's row, double-buffered, two -inf pads in front so that s - 1 and s - 2 need no bounds test
  __shared__ double rowbuf[ONE ? 1 : 2][ONE ? 1 : NT + 2];
  const int j = blockIdx.x, b = j / p.N, s = threadIdx.x, lane = s & 63;
  const int Tb = in_len_of(p, b), L = tgt_len_of(p, j), Sb = 2 * L + 1;
  const int32_t* tg = tgt_of(p, j);
  const bool valid = s < Sb;
  const int sc = min(s, Sb - 1);
  const bool odd = valid && (s & 1) && s >= 3;
  const bool skip = odd && ext_label(p, tg, s) != ext_label(p, tg, s - 2);   // s - 2 -> s allowed
  int reps;
  if (ONE) reps = __popcll(__ballot(odd && !skip));
  else reps = __syncthreads_count(odd && !skip);
  const bool here = present(p, j);
  if (!here || Tb < L + reps || Tb <= 0) {   // uniform over the workgroup
    if (s == 0) {
      const bool empty_ok = here && Tb <= 0 && L == 0;
      p.ll[j] = empty_ok ? 0.f : NEG_INF;
      p.llw[j] = empty_ok ? 0.0 : NEG_INF_D;
    }
    return;
  }
  const float* lp = p.lpe + (long)j * p.T * p.S;
  double* al = p.alpha + (long)j * p.T * p.S;
  if (!ONE) {
    if (s < 2) rowbuf[0][s] = rowbuf[1][s] = NEG_INF_D;
  }
  float cur[PF], nxt[PF];
  auto frame = [](int i) { return i; };
  double prev = NEG_INF_D;
  fetch_lpe(cur, lp, p.S, sc, 0, Tb, frame);
  for (int i0 = 0; i0 < Tb; i0 += PF) {
    fetch_lpe(nxt, lp, p.S, sc, min(i0 + PF, Tb - 1), Tb, frame);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int i = i0 + q;
      const bool live = i < Tb;   // uniform; steps past the utterance in the last block change nothing
      double n1, n2;
      if (ONE) {
        n1 = shr1_f64(prev);
        n2 = shr1_f64(n1);
        n1 = lane < 1 ? NEG_INF_D : n1;
        n2 = lane < 2 ? NEG_INF_D : n2;
      } else {
        const double* r = rowbuf[i & 1];   // written in frame i - 1 (frame 0 does not use it)
        n1 = r[s + 1];
        n2 = r[s];
      }
      double a = lse3(prev, n1, skip ? n2 : NEG_INF_D) + (double)cur[q];
      if (i == 0) a = s <= 1 ? (double)cur[q] : NEG_INF_D;
      if (!valid) a = NEG_INF_D;
      if (live && valid) al[(long)i * p.S + s] = a;
      prev = live ? a : prev;
      if (!ONE) {
        if (live) rowbuf[(i + 1) & 1][s + 2] = a;
        lds_barrier();   // frame i's row is complete; its readers are done with the other buffer
      }
    }
#pragma unroll
    for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
  }
  double fa, fb;   // the final blank S_b - 1 and the last label S_b - 2
  if (ONE) {
    fa = wave_bcast(prev, Sb - 1);
    fb = wave_bcast(prev, max(Sb - 2, 0));
  } else {
    const double* r = rowbuf[Tb & 1];   // frame T_b - 1's row (the last barrier of the loop made it visible)
    fa = r[Sb - 1 + 2];
    fb = r[max(Sb - 2, 0) + 2];
  }
  if (s == 0) {
    double v = Sb >= 2 ? lse3(fa, fb, NEG_INF_D) : fa;
    if (!(v > NEG_INF_D && v < (double)INFINITY)) v = NEG_INF_D;   // -inf, +inf, NaN (non-finite logits): not live
    p.ll[j] = (float)v;
    p.llw[j] = v;
  }
}

// ---------------------------------------------------------------------------------- weights
// blockIdx.x = utterance, one wave.  Every lane runs the same sums in n order; lane l stores n = l and l + 64.
__global__ __launch_bounds__(64) void nbest_weights(NbestP p) {
  const int b = blockIdx.x, lane = threadIdx.x, j0 = b * p.N;
  int cnt = 0;
  double mx = NEG_INF_D;
  double rs = 0.0;   // in double the sum of <= 128 equal risks is exact, so equal risks give r - rbar == 0 exactly
  for (int n = 0; n < p.N; ++n) {
    const double l = p.llw[j0 + n];   // finite or -inf (nbest_alpha); -inf for a hypothesis that is not present
    if (!(l > NEG_INF_D)) continue;
    ++cnt;
    mx = fmax(mx, l);
    if (p.risk) rs += (double)p.risk[j0 + n];
  }
  float z = 0.f;
  for (int n = 0; n < p.N; ++n) {
    const double l = p.llw[j0 + n];
    if (l > NEG_INF_D) z += expf((float)(l - mx));
  }
  const float rbar = cnt > 0 ? (float)(rs / (double)cnt) : 0.f;
  float loss = 0.f;
  if (p.risk && cnt >= 2) {
    for (int n = 0; n < p.N; ++n) {
      const double l = p.llw[j0 + n];
      if (l > NEG_INF_D) loss += (expf((float)(l - mx)) / z) * (p.risk[j0 + n] - rbar);
    }
  }
  for (int n = lane; n < p.N; n += 64) {
    const double l = p.llw[j0 + n];
    const bool live = l > NEG_INF_D;
    const float po = live ? expf((float)(l - mx)) / z : 0.f;
    p.post[j0 + n] = po;
    p.c[j0 + n] = (live && p.risk && cnt >= 2) ? po * ((p.risk[j0 + n] - rbar) - loss) : 0.f;
  }
  if (p.loss && lane == 0) p.loss[b] = loss;
}

// ---------------------------------------------------------------------------------- beta, occupancy
template <int NT>
__global__ __launch_bounds__(NT) void nbest_beta(NbestP p) {
  constexpr bool ONE = NT == 64;
  // next frame's row, double-buffered, two -inf pads behind so that s + 1 and s + 2 need no bounds test
  __shared__ double rowbuf[ONE ? 1 : 2][ONE ? 1 : NT + 2];
  const int j = blockIdx.x, b = j / p.N, s = threadIdx.x, lane = s & 63;
  if (p.c[j] == 0.f) return;   // uniform (also every problem that is not live: its c is 0)
  const int Tb = in_len_of(p, b), L = tgt_len_of(p, j), Sb = 2 * L + 1;
  if (Tb <= 0) return;         // (a live problem without frames has no labels and no gradient)
  const int32_t* tg = tgt_of(p, j);
  const bool valid = s < Sb;
  const int sc = min(s, Sb - 1);
  const bool odd = valid && (s & 1);
  const bool skip = odd && s + 2 < Sb && ext_label(p, tg, s) != ext_label(p, tg, s + 2);   // s -> s + 2 allowed
  if (odd) {
    // equal labels of the hypothesis as chains in position order, for the gradient's per-class sums
    const int u = s >> 1, lab = label_of(p, tg, u);
    bool first = true;
    for (int k = 0; k < u; ++k) first = first && label_of(p, tg, k) != lab;
    int next = 0;
    for (int k = L - 1; k > u; --k) next = label_of(p, tg, k) == lab ? k : next;
    p.chain[(long)j * p.Smax + u] = next | (first ? CHAIN_FIRST : 0);
  }
  const double ll = p.llw[j];
  float* lp = p.lpe + (long)j * p.T * p.S;
  const double* al = p.alpha + (long)j * p.T * p.S;
  const int nt = blockDim.x;
  if (!ONE) {
    if (s < 2) rowbuf[0][nt + s] = rowbuf[1][nt + s] = NEG_INF_D;
  }
  float cur[PF], nxt[PF];
  auto frame = [Tb](int i) { return Tb - 1 - i; };
  double next = NEG_INF_D;   // beta of the frame after this step's
  fetch_lpe(cur, lp, p.S, sc, 0, Tb, frame);
  for (int i0 = 0; i0 < Tb; i0 += PF) {
    // this block's alpha: loaded here, used as the block's steps reach it; the lpe cells are fetched one block ahead,
    // so a cell's emission is in a register of ITS thread before that thread overwrites it with the occupancy
    double cua[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) cua[q] = al[(long)frame(min(i0 + q, Tb - 1)) * p.S + sc];
    fetch_lpe(nxt, lp, p.S, sc, min(i0 + PF, Tb - 1), Tb, frame);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int i = i0 + q;
      const bool live = i < Tb;   // uniform
      double n1, n2;
      if (ONE) {
        // lane l <- lane l + 1 (wave_shl; the shifted-in lanes are set to -inf)
        n1 = shl1_f64(next);
        n2 = shl1_f64(n1);
        n1 = lane > 62 ? NEG_INF_D : n1;
        n2 = lane > 61 ? NEG_INF_D : n2;
      } else {
        const double* r = rowbuf[i & 1];   // written in step i - 1 (step 0 does not use it)
        n1 = r[s + 1];
        n2 = r[s + 2];
      }
      double bt = lse3(next, n1, skip ? n2 : NEG_INF_D) + (double)cur[q];
      if (i == 0) bt = s >= Sb - 2 ? (double)cur[q] : NEG_INF_D;
      if (!valid) bt = NEG_INF_D;
      if (live && valid) {
        const double a = cua[q];
        lp[(long)(Tb - 1 - i) * p.S + s] =
            (a > NEG_INF_D && bt > NEG_INF_D) ? expf((float)(((a + bt) - (double)cur[q]) - ll)) : 0.f;
      }
      next = live ? bt : next;
      if (!ONE) {
        if (live) rowbuf[(i + 1) & 1][s] = bt;
        lds_barrier();
      }
    }
#pragma unroll
    for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
  }
}

// ---------------------------------------------------------------------------------- gradient rows
__device__ __forceinline__ void store_row(float* out, const float* src, int n, bool v4, int tid) {
  if (v4) {
    for (int v = tid * 4; v < n; v += GR_NT * 4) {
      const float4 q = src ? make_float4(src[v], src[v + 1], src[v + 2], src[v + 3]) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(out + v) = q;
    }
  } else {
    for (int v = tid; v < n; v += GR_NT) out[v] = src ? src[v] : 0.f;
  }
}

// blockIdx.x = b T + t.  Dynamic LDS: min(V, GR_VC) class sums + GR_NT / 64 wave partials.
__global__ __launch_bounds__(GR_NT) void nbest_grad(NbestP p, const float* __restrict__ grad_loss, int grad_stride,
                                                    float* __restrict__ grad, long gsb, long gst) {
  extern __shared__ float acc[];
  const int b = blockIdx.x / p.T, t = blockIdx.x % p.T, tid = threadIdx.x;
  float* out = grad + b * gsb + t * gst;
  const bool v4 = (p.V % 4 == 0) && (gsb % 4 == 0) && (gst % 4 == 0) && ((uintptr_t)grad % 16 == 0);
  bool any = false;   // uniform
  if (t < in_len_of(p, b)) {
    for (int n = 0; n < p.N; ++n) any = any || p.c[b * p.N + n] != 0.f;
  }
  if (!any) {
    store_row(out, nullptr, p.V, v4, tid);
    return;
  }
  const float g = grad_loss[(long)b * grad_stride];
  const int vcap = min(p.V, GR_VC);
  float* part = acc + vcap;
  for (int v0 = 0; v0 < p.V; v0 += GR_VC) {
    const int vc = min(GR_VC, p.V - v0);
    for (int v = tid; v < vc; v += GR_NT) acc[v] = 0.f;
    __syncthreads();
    const bool has_blank = p.blank >= v0 && p.blank < v0 + vc;
    float bl = 0.f;   // this thread's share of the blank states' sum
    for (int n = 0; n < p.N; ++n) {
      const int j = b * p.N + n;
      const float cn = p.c[j];
      if (cn == 0.f) continue;   // uniform
      const float w = g * cn;
      const int L = tgt_len_of(p, j), Sj = 2 * L + 1;
      const int32_t* tg = tgt_of(p, j);
      const float* oc = p.lpe + ((long)j * p.T + t) * p.S;   // the occupancy (nbest_beta)
      const int32_t* ch = p.chain + (long)j * p.Smax;
      for (int u = tid; u < L; u += GR_NT) {
        if (!(ch[u] & CHAIN_FIRST)) continue;
        const int v = label_of(p, tg, u) - v0;
        if (v < 0 || v >= vc) continue;
        float sum = 0.f;
        int k = u;
        for (int hop = 0; hop < L; ++hop) {   // at most L links, in position order
          sum += oc[2 * k + 1];
          k = min(ch[k] & (CHAIN_FIRST - 1), L - 1);
          if (k == 0) break;
        }
        acc[v] += w * sum;   // the one writer of class v in this hypothesis
      }
      if (has_blank) {
        for (int s = 2 * tid; s < Sj; s += 2 * GR_NT) bl += w * oc[s];
      }
      __syncthreads();   // the next hypothesis may hold the class in another thread
    }
    if (has_blank) {
      bl = wave_sum(bl);
      if ((tid & 63) == 0) part[tid >> 6] = bl;
      __syncthreads();
      if (tid == 0) {
        float sum = 0.f;
        for (int w = 0; w < GR_NT / 64; ++w) sum += part[w];
        acc[p.blank - v0] += sum;
      }
      __syncthreads();
    }
    store_row(out + v0, acc, vc, v4, tid);
    __syncthreads();
  }
}

struct NbestWs { size_t alpha, llw, lpe, c, chain, total; };
NbestWs nbest_ws(int B, int T, int N, int Smax) {
  const size_t J = (size_t)B * N, jts = J * T * (2 * (size_t)Smax + 1);
  NbestWs w;
  w.alpha = 0;                                  // the doubles first: 8-byte aligned
  w.llw = w.alpha + sizeof(double) * jts;
  w.lpe = w.llw + sizeof(double) * J;
  w.c = w.lpe + sizeof(float) * jts;
  w.chain = w.c + sizeof(float) * J;
  w.total = (w.chain + sizeof(int32_t) * J * (size_t)Smax + 15) & ~(size_t)15;
  return w;
}

int nbest_params(const char* fn, NbestP& p, const float* logits, long sb, long st, const int32_t* in_len, int B, int T,
                 int V, const int32_t* hyp, int ldh, const int32_t* hyp_len, int N, int max_labels, int blank,
                 void* ws) {
  CFM_REQUIRE_FN(fn, N >= 1, CFM_ERR_ARG, "N must be >= 1");
  CFM_REQUIRE_FN(fn, N <= NBEST_MAX, CFM_ERR_UNSUPPORTED, "N must be <= 128");
  CFM_REQUIRE_FN(fn, logits && in_len && hyp_len && ws, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE_FN(fn, hyp || max_labels == 0, CFM_ERR_ARG, "null hypotheses");
  CFM_REQUIRE_FN(fn, (uintptr_t)ws % 8 == 0, CFM_ERR_ALIGN, "ws must be 8-byte aligned");
  static_cast<CtcView&>(p) = make_view(logits, sb, st, hyp, ldh, nullptr, in_len, hyp_len, B, T, V, max_labels, blank);
  if (const int rc = check_ctc_problem(fn, p)) return rc;
  CFM_REQUIRE_FN(fn, (long)B * N * T <= 0x7fffffffL && (long)B * T <= 0x7fffffffL, CFM_ERR_UNSUPPORTED,
                 "B * N * T must fit 31 bits");
  const NbestWs w = nbest_ws(B, T, N, max_labels);
  char* base = static_cast<char*>(ws);
  p.N = N;
  p.risk = nullptr; p.ll = nullptr; p.post = nullptr; p.loss = nullptr;
  p.alpha = reinterpret_cast<double*>(base + w.alpha);
  p.llw = reinterpret_cast<double*>(base + w.llw);
  p.lpe = reinterpret_cast<float*>(base + w.lpe);
  p.c = reinterpret_cast<float*>(base + w.c);
  p.chain = reinterpret_cast<int32_t*>(base + w.chain);
  return CFM_OK;
}

// the recursion's block for S states: one wave, a block of up to 256 threads, or up to 1024
#define NBEST_LAUNCH(kernel, S, J, s, p)                                                                  \
  do {                                                                                                    \
    if ((S) <= 64) hipLaunchKernelGGL(kernel<64>, dim3(J), dim3(64), 0, s, p);                            \
    else if ((S) <= 256) hipLaunchKernelGGL(kernel<256>, dim3(J), dim3(((S) + 63) & ~63), 0, s, p);       \
    else hipLaunchKernelGGL(kernel<CTC_MAX_STATES>, dim3(J), dim3(((S) + 63) & ~63), 0, s, p);            \
  } while (0)

}  // namespace

CFM_EXPORT size_t cfm_ctc_nbest_ws_bytes(int B, int T, int N, int max_labels) {
  if (B <= 0 || T <= 0 || N <= 0 || max_labels < 0) return 0;
  return nbest_ws(B, T, N, max_labels).total;
}

CFM_EXPORT int cfm_ctc_nbest_fwd(const float* logits, long sb, long st, const int32_t* in_len, int B, int T, int V,
                                 const int32_t* hyp, int ldh, const int32_t* hyp_len, int N, int max_labels, int blank,
                                 const float* risk, float* ll, float* post, float* loss, void* ws, void* stream) {
  NbestP p;
  if (const int rc = nbest_params(__func__, p, logits, sb, st, in_len, B, T, V, hyp, ldh, hyp_len, N, max_labels,
                                  blank, ws))
    return rc;
  CFM_REQUIRE(ll && post, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE((risk != nullptr) == (loss != nullptr), CFM_ERR_ARG, "risk and loss: both or neither");
  p.risk = risk; p.ll = ll; p.post = post; p.loss = loss;
  hipStream_t s = cfm::as_stream(stream);
  const int J = B * N;
  hipLaunchKernelGGL(nbest_prep, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), 0, s, p);
  NBEST_LAUNCH(nbest_alpha, p.S, J, s, p);
  hipLaunchKernelGGL(nbest_weights, dim3(B), dim3(64), 0, s, p);
  return cfm::check_launch("cfm_ctc_nbest_fwd");
}

CFM_EXPORT int cfm_ctc_nbest_bwd(const float* logits, long sb, long st, const int32_t* in_len, int B, int T, int V,
                                 const int32_t* hyp, int ldh, const int32_t* hyp_len, int N, int max_labels, int blank,
                                 void* ws, const float* grad_loss, int grad_stride, float* grad_logits, long gsb,
                                 long gst, void* stream) {
  NbestP p;
  if (const int rc = nbest_params(__func__, p, logits, sb, st, in_len, B, T, V, hyp, ldh, hyp_len, N, max_labels,
                                  blank, ws))
    return rc;
  CFM_REQUIRE(grad_loss && grad_logits, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(grad_stride == 0 || grad_stride == 1, CFM_ERR_ARG, "grad_stride must be 0 or 1");
  hipStream_t s = cfm::as_stream(stream);
  const int J = B * N;
  NBEST_LAUNCH(nbest_beta, p.S, J, s, p);
  const size_t sh = sizeof(float) * ((size_t)(V < GR_VC ? V : GR_VC) + GR_NT / 64);
  hipLaunchKernelGGL(nbest_grad, dim3((unsigned)((long)B * T)), dim3(GR_NT), sh, s, p, grad_loss, grad_stride,
                     grad_logits, gsb, gst);
  return cfm::check_launch("cfm_ctc_nbest_bwd");
}
