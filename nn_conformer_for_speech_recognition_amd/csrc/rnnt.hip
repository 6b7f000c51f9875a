// rnnt.hip — the RNN-T (transducer, Graves 2012) loss over a dense lattice of joint logits, and its gradient.
//
// B utterances, T frames, U1 = Umax + 1 label positions, V classes: logits x (B, T, U1, V) fp32, dense.  With T_b,
// U_b the clamped lengths, lp = log_softmax over V, b(t,u) = lp[t,u,blank], y(t,u) = lp[t,u,label_{u+1}] (u < U_b):
//
//   alpha(0,0) = 0;  alpha(t,u) = lse(alpha(t-1,u) + b(t-1,u), alpha(t,u-1) + y(t,u-1))
//   beta(T_b-1,U_b) = b(T_b-1,U_b);  beta(t,u) = lse(beta(t+1,u) + b(t,u), beta(t,u+1) + y(t,u))
//   ll_b = alpha(T_b-1,U_b) + b(T_b-1,U_b)  (= beta(0,0));  loss_b = -ll_b
//   gamma(t,u) = exp(alpha + beta - ll)
//   d loss_b / d x[t,u,v] = softmax(x)[t,u,v] gamma(t,u) - [v = blank] exp(alpha(t,u) + b(t,u) + beta(t+1,u) - ll)
//                           - [v = label_{u+1}, u < U_b] exp(alpha(t,u) + y(t,u) + beta(t,u+1) - ll)
//   (at the corner (T_b-1, U_b) the blank term is exp(alpha + b - ll) = gamma); every valid row sums to 0 over v,
//   because beta(t,u) is the log-sum of exactly the two subtracted exponents.
// Outside the valid cells (t < T_b, u <= U_b) the gradient is written as exact zeros and the logits are never read.
// T_b = 0, or an ll that is not finite: ll = -inf and a zero gradient for the utterance.
//
// Work arrays are DIAGONAL-MAJOR: cell (t, u) of utterance b lies at [b][d = t + u][u], D = T + U1 - 1 diagonals of
// U1 columns.  The recursions run one column per thread over the anti-diagonals; both neighbours of a cell lie on the
// diagonal before (alpha) or after (beta), so a step reads ONE contiguous line of b and of y instead of a line of
// stride U1 - 1, and alpha / beta are stored as contiguous lines too.
//
// Kernels (two launches forward -- prep, lattice -- and one backward):
//   rnnt_prep      one wave per (b, t, u) row, four rows per workgroup: the row's max and log-sum once
//                  (ctc_common.h's row_stats), then b(t,u), y(t,u) and the row's m + log s into the workspace.  The
//                  forward's only pass over the logits.                   Bound: HBM, one read of B T U1 V floats
//   rnnt_lattice   grid (B, 2): blockIdx.y 0 runs alpha, 1 runs beta, side by side in one launch.  T_b + U_b
//                  sequential steps of one dependent log-sum-exp each.  <64>: U1 <= 64, one wave, the neighbour's
//                  value through DPP shifts, no LDS, no barrier; <256> / <1024>: the previous diagonal double-buffered
//                  in LDS, one barrier per diagonal.  The b / y lines are prefetched a chunk of PF diagonals ahead.
//                  Bound: latency -- the dependent chain of T_b + U_b steps (two fp32 exp, one log, a handful of
//                  double additions, plus the barrier above one wave); 2 B workgroups occupy a fraction of the card,
//                  and its traffic (16 + 8 bytes per cell) is small beside the logits.
//   rnnt_grad      one wave per (b, t, u) row: reads the logits row, the row's log-sum, alpha(t,u), beta(t,u),
//                  beta(t+1,u), beta(t,u+1) and ll, writes the whole V-wide gradient row times grad_loss[b] (float4
//                  where V and the bases allow); zero rows outside the valid cells.
//                                                                         Bound: HBM, one read and one write of B T U1 V
// Algorithmic HBM traffic of a forward + backward: 3 B T U1 V 4 bytes.
// No atomics, no host synchronisation (graph-capturable).  No loop waits on, or takes its trip count from, a value
// another wave writes in the same launch: the trip counts come from in_len / tgt_len, which no kernel writes.
//
// Precision follows ctc_nbest.hip, "Precision": alpha, beta and ll are double; exp and log are fp32 on O(1)
// differences formed in double; emissions are (x - m) - log sum exp(x - m), as align_prep forms them.
#include "ctc_common.h"

using namespace ctc;

namespace {

constexpr int RNNT_MAX_U1 = 1024;   // one column per thread of the recursion's largest block
constexpr double NEG_INF_D = -INFINITY;

// The view's logits rows are the B * T * U1 lattice rows (sb = T U1 V, st = U1 V, so row_stats' alignment test is
// the one of a dense array); Smax = U1 - 1 makes tgt_len_of the clamp to [0, U1 - 1].
struct RnntP : CtcView {
  int U1, D;           // D = T + U1 - 1 diagonals
  float* bl;           // (B, D, U1) b(t,u), diagonal-major
  float* yl;           // (B, D, U1) y(t,u)
  float* lse;          // (B, T, U1) the row's m + log s
  double* alpha;       // (B, D, U1)
  double* beta;        // (B, D, U1)
  double* llw;         // (B) ll, unrounded
  float* ll;           // (B) the caller's
};

__device__ __forceinline__ long cell_of(const RnntP& p, int b, int t, int u) {
  return ((long)b * p.D + (t + u)) * p.U1 + u;
}

// log(exp(a) + exp(b)): double in and out, the functions in fp32 on the O(1) differences (header comment)
__device__ __forceinline__ double lse2d(double a, double b) {
  const double m = fmax(a, b);
  if (m == NEG_INF_D) return NEG_INF_D;
  const float s = expf((float)(a - m)) + expf((float)(b - m));
  return m + (double)logf(s);
}

// the one-lane wave shifts of cfm_common.h on the two halves of a double (as ctc_nbest.hip's)
__device__ __forceinline__ double shr1_f64(double v) {
  const int hi = ::wave_shr1(__double2hiint(v)), lo = ::wave_shr1(__double2loint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double shl1_f64(double v) {
  const int hi = ::wave_shl1(__double2hiint(v)), lo = ::wave_shl1(__double2loint(v));
  return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------------- emissions
__global__ __launch_bounds__(256) void rnnt_prep(RnntP p) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long tu = (long)p.T * p.U1;
  if (row >= (long)p.B * tu) return;
  const int b = (int)(row / tu), t = (int)((row % tu) / p.U1), u = (int)(row % p.U1);
  const int Ub = tgt_len_of(p, b);
  if (t >= in_len_of(p, b) || u > Ub) return;   // the logits outside the valid cells are never read
  const float* x = p.logits + row * p.V;
  float m, ls;
  row_stats(p, x, lane, m, ls);
  if (lane == 0) {
    const long c = cell_of(p, b, t, u);
    // (x - m) - log(sum): every rounding relative to the log-probability itself (align_prep's comment)
    p.bl[c] = (x[p.blank] - m) - ls;
    p.yl[c] = u < Ub ? (x[label_of(p, tgt_of(p, b), u)] - m) - ls : NEG_INF;
    p.lse[row] = m + ls;
  }
}

// ---------------------------------------------------------------------------------- alpha, beta
// grid (B, 2), blockIdx.y 0: alpha, 1: beta.  NT 64: one wave, else blockDim.x = U1 rounded up to 64 (<= NT).
// Step i works on diagonal d = i (alpha) or n - 1 - i (beta), n = T_b + U_b diagonals; thread u holds cell
// (d - u, u).  A cell outside the lattice has the value -inf, so a valid cell's missing neighbour needs no test.
//   alpha: the cell's two incoming terms were formed by their SOURCE cells on the diagonal before: up = own
//          alpha + b (from (t-1, u)), left = the neighbour u - 1's alpha + y (from (t, u-1)).
//   beta:  beta = lse(own previous (t+1, u) + b, the neighbour u + 1's previous (t, u+1) + y), b and y its own.
template <int NT>
__global__ __launch_bounds__(NT) void rnnt_lattice(RnntP p) {
  constexpr bool ONE = NT == 64;
  // the neighbouring diagonal's values, double-buffered; slot u + 1 holds column u, slots 0 and nt + 1 stay -inf
  __shared__ double rowbuf[ONE ? 1 : 2][ONE ? 1 : NT + 2];
  const int b = blockIdx.x, u = threadIdx.x, lane = u & 63;
  const bool back = blockIdx.y != 0;
  const int Tb = in_len_of(p, b), Ub = tgt_len_of(p, b);
  if (Tb <= 0) {   // uniform over the workgroup: the utterance takes no part
    if (u == 0 && !back) {
      p.ll[b] = NEG_INF;
      p.llw[b] = NEG_INF_D;
    }
    return;
  }
  const int n = Tb + Ub;                     // diagonals with a valid cell
  const int uc = min(u, p.U1 - 1);           // threads past U1 (the block is rounded up to a wave) load column U1 - 1
  const bool col = u <= Ub;
  const long base = (long)b * p.D * p.U1;
  const float* bl = p.bl + base;
  const float* yl = p.yl + base;
  double* out = (back ? p.beta : p.alpha) + base;
  if (!ONE) {
    for (int k = u; k < 2 * (NT + 2); k += blockDim.x) (&rowbuf[0][0])[k] = NEG_INF_D;
    __syncthreads();
  }
  float cb[PF], cy[PF], nb[PF], ny[PF];
  double keep = NEG_INF_D;   // alpha: own alpha + b of the step before; beta: own beta of the step before
  double pass = NEG_INF_D;   // what the neighbour reads: alpha + y (alpha), beta (beta)
  if (!back) {
    auto diag = [](int i) { return i; };
    fetch_lpe(cb, bl, p.U1, uc, 0, n, diag);
    fetch_lpe(cy, yl, p.U1, uc, 0, n, diag);
    for (int i0 = 0; i0 < n; i0 += PF) {
      fetch_lpe(nb, bl, p.U1, uc, min(i0 + PF, n - 1), n, diag);
      fetch_lpe(ny, yl, p.U1, uc, min(i0 + PF, n - 1), n, diag);
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int i = i0 + q, t = i - u;
        const bool live = i < n;                      // uniform; steps past the last diagonal change nothing
        const bool valid = col && t >= 0 && t < Tb;
        double left;
        if (ONE) {
          left = shr1_f64(pass);
          left = lane < 1 ? NEG_INF_D : left;
        } else {
          left = rowbuf[i & 1][u];                    // column u - 1, written in step i - 1
        }
        double a = lse2d(keep, left);
        if (i == 0) a = u == 0 ? 0.0 : NEG_INF_D;
        if (!valid) a = NEG_INF_D;                    // (also keeps the unwritten b / y of such a cell out)
        if (live && valid) out[(long)i * p.U1 + u] = a;
        const double k2 = valid ? a + (double)cb[q] : NEG_INF_D;
        const double p2 = valid && u < Ub ? a + (double)cy[q] : NEG_INF_D;
        keep = live ? k2 : keep;
        pass = live ? p2 : pass;
        if (!ONE) {
          if (live) rowbuf[(i + 1) & 1][u + 1] = p2;
          lds_barrier();   // step i's line is complete; its readers are done with the other buffer
        }
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) { cb[q] = nb[q]; cy[q] = ny[q]; }
    }
    if (u == Ub) {   // keep = alpha(T_b-1, U_b) + b(T_b-1, U_b), the last diagonal's one cell
      double v = keep;
      if (!(v > NEG_INF_D && v < (double)INFINITY)) v = NEG_INF_D;   // -inf, +inf, NaN: the utterance takes no part
      p.ll[b] = (float)v;
      p.llw[b] = v;
    }
  } else {
    auto diag = [n](int i) { return n - 1 - i; };
    fetch_lpe(cb, bl, p.U1, uc, 0, n, diag);
    fetch_lpe(cy, yl, p.U1, uc, 0, n, diag);
    for (int i0 = 0; i0 < n; i0 += PF) {
      fetch_lpe(nb, bl, p.U1, uc, min(i0 + PF, n - 1), n, diag);
      fetch_lpe(ny, yl, p.U1, uc, min(i0 + PF, n - 1), n, diag);
#pragma unroll
      for (int q = 0; q < PF; ++q) {
        const int i = i0 + q, d = n - 1 - i, t = d - u;
        const bool live = i < n;                      // uniform
        const bool valid = col && t >= 0 && t < Tb;
        double right;
        if (ONE) {
          right = shl1_f64(pass);
          right = lane > 62 ? NEG_INF_D : right;
        } else {
          right = rowbuf[i & 1][u + 2];               // column u + 1, written in step i - 1
        }
        const double viaY = valid && u < Ub ? right + (double)cy[q] : NEG_INF_D;
        double bt = valid ? lse2d(keep + (double)cb[q], viaY) : NEG_INF_D;
        if (valid && t == Tb - 1 && u == Ub) bt = (double)cb[q];   // the corner
        if (live && valid) out[(long)d * p.U1 + u] = bt;
        keep = live ? bt : keep;
        pass = keep;
        if (!ONE) {
          if (live) rowbuf[(i + 1) & 1][u + 1] = bt;
          lds_barrier();
        }
      }
#pragma unroll
      for (int q = 0; q < PF; ++q) { cb[q] = nb[q]; cy[q] = ny[q]; }
    }
  }
}

// ---------------------------------------------------------------------------------- gradient rows
__global__ __launch_bounds__(256) void rnnt_grad(RnntP p, const float* __restrict__ grad_loss,
                                                 float* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long tu = (long)p.T * p.U1;
  if (row >= (long)p.B * tu) return;
  const int b = (int)(row / tu), t = (int)((row % tu) / p.U1), u = (int)(row % p.U1);
  const int Tb = in_len_of(p, b), Ub = tgt_len_of(p, b);
  float* out = grad + row * p.V;
  const bool v4 = (p.V % 4 == 0) && ((uintptr_t)p.logits % 16 == 0) && ((uintptr_t)grad % 16 == 0);
  // (llw is read only where the forward wrote it: T_b > 0)
  const double ll = Tb > 0 ? p.llw[b] : NEG_INF_D;
  if (t >= Tb || u > Ub || !(ll > NEG_INF_D)) {   // uniform over the wave
    if (v4) {
      for (int v = lane * 4; v < p.V; v += 256) *reinterpret_cast<float4*>(out + v) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int v = lane; v < p.V; v += 64) out[v] = 0.f;
    }
    return;
  }
  const float* x = p.logits + row * p.V;
  const long c = cell_of(p, b, t, u);
  const double a = p.alpha[c], bt = p.beta[c];
  const float g = grad_loss[b], lz = p.lse[row];
  const float gam = expf((float)((a + bt) - ll));
  float wb, wy = 0.f;   // the blank's and the label's path weights
  if (t + 1 < Tb) wb = expf((float)(((a + (double)p.bl[c]) + p.beta[cell_of(p, b, t + 1, u)]) - ll));
  else wb = u == Ub ? expf((float)((a + (double)p.bl[c]) - ll)) : 0.f;
  int lab = -1;
  if (u < Ub) {
    lab = label_of(p, tgt_of(p, b), u);
    wy = expf((float)(((a + (double)p.yl[c]) + p.beta[cell_of(p, b, t, u + 1)]) - ll));
  }
  auto one = [&](float xv, int v) {
    float r = expf(xv - lz) * gam;
    if (v == p.blank) r -= wb;
    if (v == lab) r -= wy;
    return g * r;
  };
  if (v4) {
    for (int v = lane * 4; v < p.V; v += 256) {
      const float4 q = *reinterpret_cast<const float4*>(x + v);
      *reinterpret_cast<float4*>(out + v) = make_float4(one(q.x, v), one(q.y, v + 1), one(q.z, v + 2), one(q.w, v + 3));
    }
  } else {
    for (int v = lane; v < p.V; v += 64) out[v] = one(x[v], v);
  }
}

struct RnntWs { size_t alpha, beta, llw, bl, yl, lse, total; };
RnntWs rnnt_ws(int B, int T, int U1) {
  const size_t cells = (size_t)B * ((size_t)T + U1 - 1) * U1, rows = (size_t)B * T * U1;
  RnntWs w;
  w.alpha = 0;                                   // the doubles first: 8-byte aligned
  w.beta = w.alpha + sizeof(double) * cells;
  w.llw = w.beta + sizeof(double) * cells;
  w.bl = w.llw + sizeof(double) * (size_t)B;
  w.yl = w.bl + sizeof(float) * cells;
  w.lse = w.yl + sizeof(float) * cells;
  w.total = (w.lse + sizeof(float) * rows + 15) & ~(size_t)15;
  return w;
}

int rnnt_params(const char* fn, RnntP& p, const float* logits, const int32_t* targets, int ldt, const int32_t* in_len,
                const int32_t* tgt_len, int B, int T, int U1, int V, int blank, const void* ws) {
  CFM_REQUIRE_FN(fn, B > 0 && T > 0 && U1 > 0 && V > 0 && ldt >= U1 - 1, CFM_ERR_SHAPE, "bad shape");
  CFM_REQUIRE_FN(fn, logits && in_len && tgt_len && ws && (targets || U1 == 1), CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE_FN(fn, blank >= 0 && blank < V, CFM_ERR_ARG, "blank out of range");
  CFM_REQUIRE_FN(fn, U1 <= RNNT_MAX_U1, CFM_ERR_UNSUPPORTED, "at most 1023 labels (U1 <= 1024)");
  CFM_REQUIRE_FN(fn, V >= 2, CFM_ERR_UNSUPPORTED, "V must be >= 2");
  CFM_REQUIRE_FN(fn, (long)B * T * U1 <= 0x7fffffffL, CFM_ERR_UNSUPPORTED, "B * T * U1 must fit 31 bits");
  CFM_REQUIRE_FN(fn, (uintptr_t)ws % 8 == 0, CFM_ERR_ALIGN, "ws must be 8-byte aligned");
  static_cast<CtcView&>(p) = make_view(logits, (long)T * U1 * V, (long)U1 * V, targets, ldt, nullptr, in_len, tgt_len,
                                       B, T, V, U1 - 1, blank);
  const RnntWs w = rnnt_ws(B, T, U1);
  char* base = static_cast<char*>(const_cast<void*>(ws));
  p.U1 = U1;
  p.D = T + U1 - 1;
  p.alpha = reinterpret_cast<double*>(base + w.alpha);
  p.beta = reinterpret_cast<double*>(base + w.beta);
  p.llw = reinterpret_cast<double*>(base + w.llw);
  p.bl = reinterpret_cast<float*>(base + w.bl);
  p.yl = reinterpret_cast<float*>(base + w.yl);
  p.lse = reinterpret_cast<float*>(base + w.lse);
  p.ll = nullptr;
  return CFM_OK;
}

}  // namespace

CFM_EXPORT size_t cfm_rnnt_ws_bytes(int B, int T, int U1) {
  if (B <= 0 || T <= 0 || U1 <= 0) return 0;
  return rnnt_ws(B, T, U1).total;
}

CFM_EXPORT int cfm_rnnt_loss_fwd(const float* logits, const int32_t* targets, int ldt, const int32_t* in_len,
                                 const int32_t* tgt_len, int B, int T, int U1, int V, int blank, float* ll, void* ws,
                                 void* stream) {
  RnntP p;
  if (const int rc = rnnt_params(__func__, p, logits, targets, ldt, in_len, tgt_len, B, T, U1, V, blank, ws)) return rc;
  CFM_REQUIRE(ll, CFM_ERR_ARG, "null pointer");
  p.ll = ll;
  hipStream_t s = cfm::as_stream(stream);
  const unsigned rows4 = (unsigned)(((long)B * T * U1 + 3) / 4);
  hipLaunchKernelGGL(rnnt_prep, dim3(rows4), dim3(256), 0, s, p);
  const dim3 grid(B, 2), block((U1 + 63) & ~63);
  if (U1 <= 64) hipLaunchKernelGGL(rnnt_lattice<64>, grid, block, 0, s, p);
  else if (U1 <= 256) hipLaunchKernelGGL(rnnt_lattice<256>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(rnnt_lattice<RNNT_MAX_U1>, grid, block, 0, s, p);
  return cfm::check_launch("cfm_rnnt_loss_fwd");
}

CFM_EXPORT int cfm_rnnt_loss_bwd(const float* logits, const int32_t* targets, int ldt, const int32_t* in_len,
                                 const int32_t* tgt_len, int B, int T, int U1, int V, int blank, const void* ws,
                                 const float* grad_loss, float* dlogits, void* stream) {
  RnntP p;
  if (const int rc = rnnt_params(__func__, p, logits, targets, ldt, in_len, tgt_len, B, T, U1, V, blank, ws)) return rc;
  CFM_REQUIRE(grad_loss && dlogits, CFM_ERR_ARG, "null pointer");
  hipStream_t s = cfm::as_stream(stream);
  const unsigned rows4 = (unsigned)(((long)B * T * U1 + 3) / 4);
  hipLaunchKernelGGL(rnnt_grad, dim3(rows4), dim3(256), 0, s, p, grad_loss, dlogits);
  return cfm::check_launch("cfm_rnnt_loss_bwd");
}
