// optim.hip — multi-tensor fused Adafactor step (the reference's optimizer, runner.py:36:
// transformers.Adafactor(lr, beta1=0.9, scale_parameter=False, relative_step=False); defaults
// eps=(1e-30, 1e-3), clip_threshold=1, decay_rate=-0.8, weight_decay=0).
//
// Every parameter is viewed as nb x R x C (leading dims folded into nb).  Factored second moment
// for ndim >= 2 (row/col EMAs of g^2+eps1), full EMA otherwise; update u = g * rsqrt(row_r /
// mean(row)) * rsqrt(col_c) (or g * rsqrt(v)), clipped by max(1, RMS(u)/clip), scaled by lr,
// first moment m = b1*m + (1-b1)*u, p -= m.  All parameters are handled by five launches over a
// device-side parameter table (no per-tensor launches): one pass over g for the row statistics
// and column partial sums of wide matrices (64 <= C <= 2560), row stats of narrow ones, column
// finish (partials in fixed order), row-stat means, u^2 block partials, apply (each block sums its
// tensor's partials in block order: deterministic, no atomics).  float4 paths where aligned.  Work items are "tasks" whose shape
// adapts to the tensor: a wide row (C >= 64) is one wave, narrow rows (e.g. the 3x3 taps of the
// conv2 weight, nb = 65536) are packed 64 per wave (one per lane).  HBM-bound.
//
// The hyper-parameters add the rest of transformers.Adafactor to the same launches: scale_parameter (the step
// size times max(eps2, RMS(p)); the u^2 pass also sums p^2 per block), weight_decay, and a device-side step
// (ada_scalars: step count, beta2t and relative step size in device memory, so a captured launch sequence
// replays as successive steps).  All of it is compile-time variants: the kernels a step without them launches
// (<float>, <false>) have the instruction stream they had before the variants existed.
#include <vector>

#include "ada_plan.h"

namespace {

constexpr int EB = 256;          // threads per block

// unsigned 32-bit division by an invariant divisor d >= 1 (Granlund-Montgomery): with l = ceil(log2 d) and
// m = floor(2^32 (2^l - d) / d) + 1, n / d = (t + ((n - t) >> 1)) >> (l - 1) for t = mulhi(m, n) (d >= 2);
// d == 1: m = 0, sh = 0 and the formula is replaced by n.  Exact for every 32-bit n.
struct UDiv { uint32_t m, sh, one; };
static inline UDiv udiv_make(uint32_t d) {
  if (d <= 1) return UDiv{0u, 0u, 1u};
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
  return UDiv{(uint32_t)m, l - 1, 0u};
}
__device__ __forceinline__ uint32_t udiv(uint32_t n, const UDiv& v) {
  if (v.one) return n;
  const uint32_t t = __umulhi(v.m, n);
  return (t + ((n - t) >> 1)) >> v.sh;
}

// a table entry: the parameter (col == nullptr: unfactored, row = v), the plan's totals in front of it (tasks /
// elements / workspace floats), and its element index -> (matrix, row, column) divisions
struct AdaP : cfm_adafactor_param {
  long row_toff, col_off, blk_off, rm_off, rm_toff, cp_toff, part_off;
  UDiv div_rc, div_c;
};

__device__ __forceinline__ long off_of(const AdaP& q, AdaPhase which) {
  return which == ADA_ROWS ? q.row_toff : which == ADA_COLS ? q.col_off : which == ADA_BLOCKS ? q.blk_off
         : which == ADA_ROWMEAN ? q.rm_toff : q.cp_toff;
}
__device__ __forceinline__ int find_param(const AdaP* t, int n, long idx, AdaPhase which) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off_of(t[mid], which) <= idx) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// beta2t reaches a kernel as the host's float (B2 = float: the kernels a host-scalar step launches), or is read
// from the device step scalars that ada_scalars writes (B2 = const float*: the capturable step)
constexpr int SC_B2T = 0, SC_REL = 1;   // scalar block: beta2t, relative step size
__device__ __forceinline__ float b2t_of(float v) { return v; }
__device__ __forceinline__ float b2t_of(const float* sc) { return sc[SC_B2T]; }

__device__ __forceinline__ void row_update(const AdaP& q, long lr, float s, float b2t) {
  q.row[lr] = b2t * q.row[lr] + (1.f - b2t) * (s / q.C);
}

// Wide factored tensors (64 <= C <= 2560), one pass over g: task (b, rb) covers rows
// rb*RB .. rb*RB+RB-1 of matrix b.  Row statistics are finished here (wave reduction per row);
// column sums of the block go to part[b][rb][c] (finished by ada_cols, fixed order).
template <class B2>
__global__ __launch_bounds__(EB) void ada_colpart(const AdaP* __restrict__ t, int n, long ntasks, B2 b2,
                                                  float eps1, float* __restrict__ part) {
  const float b2t = b2t_of(b2);
  __shared__ float red[4][64 * KMAX];
  const long task = blockIdx.x;
  if (task >= ntasks) return;
  const AdaP& q = t[find_param(t, n, task, ADA_COLPART)];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nrb = (q.R + RB - 1) / RB;
  const long lt = task - q.cp_toff;
  const int b = (int)(lt / nrb), rb = (int)(lt % nrb);
  const int r0 = rb * RB, r1 = min(q.R, r0 + RB);
  const int nk = (q.C + 63) / 64;
  float cacc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) cacc[k] = 0.f;
  // the wave's RB/4 rows: their sums stay in registers (lane j keeps row j's) and the row EMAs are updated
  // once after the loop -- a read-modify-write per row inside it serialised every row on a memory round trip
  float rsum = 0.f;
  if (q.C % 4 == 0 && ((uintptr_t)q.g & 15) == 0) {
    // float4 columns: lane owns columns 4 lane + 256 k4 .. +3 (k4 < nk4); cacc[4 k4 + e] = column 4 lane + 256 k4 + e
    const int nk4 = (q.C + 255) / 256;
    // the wave's next row is loaded while this one is summed (one row per round trip otherwise)
    float4 cur[KMAX / 4], nxt[KMAX / 4];
    auto load_row = [&](int r, float4 (&dst)[KMAX / 4]) {
      const float* g = q.g + ((long)b * q.R + r) * q.C;
#pragma unroll
      for (int k4 = 0; k4 < KMAX / 4; ++k4) {
        const int c = 4 * lane + 256 * k4;
        if (k4 < nk4 && c < q.C) dst[k4] = *reinterpret_cast<const float4*>(g + c);
      }
    };
    if (r0 + wv < r1) load_row(r0 + wv, cur);
    for (int j = 0; j < RB / 4; ++j) {
      const int r = r0 + wv + 4 * j;
      if (r >= r1) break;
      if (j + 1 < RB / 4 && r + 4 < r1) load_row(r + 4, nxt);
      float s = 0.f;
#pragma unroll
      for (int k4 = 0; k4 < KMAX / 4; ++k4) {
        const int c = 4 * lane + 256 * k4;
        if (k4 < nk4 && c < q.C) {
          const float4 v = cur[k4];
          const float e0 = v.x * v.x + eps1, e1 = v.y * v.y + eps1, e2 = v.z * v.z + eps1, e3 = v.w * v.w + eps1;
          s += (e0 + e1) + (e2 + e3);
          cacc[4 * k4] += e0; cacc[4 * k4 + 1] += e1; cacc[4 * k4 + 2] += e2; cacc[4 * k4 + 3] += e3;
        }
      }
      s = wave_sum(s);
      rsum = lane == j ? s : rsum;
#pragma unroll
      for (int k4 = 0; k4 < KMAX / 4; ++k4) cur[k4] = nxt[k4];
    }
#pragma unroll
    for (int k4 = 0; k4 < KMAX / 4; ++k4)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k4 < nk4 && 4 * lane + 256 * k4 + e < q.C) red[wv][4 * lane + 256 * k4 + e] = cacc[4 * k4 + e];
  } else {
    for (int j = 0; j < RB / 4; ++j) {   // (the early exit keeps this loop rolled)
      const int r = r0 + wv + 4 * j;
      if (r >= r1) break;
      const float* g = q.g + ((long)b * q.R + r) * q.C;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int c = lane + 64 * k;
        if (k < nk && c < q.C) {
          const float v = g[c];
          const float e = v * v + eps1;
          s += e;
          cacc[k] += e;
        }
      }
      s = wave_sum(s);
      rsum = lane == j ? s : rsum;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < nk) red[wv][lane + 64 * k] = cacc[k];
  }
  {
    const int r = r0 + wv + 4 * lane;
    if (lane < RB / 4 && r < r1) row_update(q, (long)b * q.R + r, rsum, b2t);
  }
  __syncthreads();
  float* dst = part + q.part_off + ((long)b * nrb + rb) * q.C;
  for (int c = threadIdx.x; c < q.C; c += EB) dst[c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// row tasks of NARROW factored tensors: ROWS_PER_TASK = 256 rows per wave (lane = 4 rows; a task per 64 rows left
// each wave's parameter search -- ~9 dependent table loads -- in front of one 4-byte row: ~18.6 M such rows at L15,
// the degenerate (O, I, 1) pointwise-conv weights, ran 95 us)
template <class B2>
__global__ void ada_rows(const AdaP* __restrict__ t, int n, long ntasks, B2 b2, float eps1) {
  const float b2t = b2t_of(b2);
  const int lane = threadIdx.x & 63;
  // wave-uniform task made provably uniform: the parameter search and the table fields become scalar loads
  const long task = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;
  const AdaP& q = t[find_param(t, n, task, ADA_ROWS)];
  const long lt = task - q.row_toff;
  if (is_wide(q.C)) {      // (wide rows are done by ada_colpart; kept for a wide tensor with no tasks)
    const float* g = q.g + lt * q.C;
    float s = 0.f;
    for (int c = lane; c < q.C; c += 64) s += g[c] * g[c] + eps1;
    s = wave_sum(s);
    if (lane == 0) row_update(q, lt, s, b2t);
    return;
  }
  const long nrows = (long)q.nb * q.R, base = lt * ROWS_PER_TASK;
  if (q.C == 1 && ((uintptr_t)q.g & 15) == 0 && ((uintptr_t)q.row & 15) == 0 && base + ROWS_PER_TASK <= nrows) {
    // one element per row: lane owns rows base + 4 lane .. +3 (16-B loads of g and of the row state)
    const long lr = base + 4 * lane;
    const float4 g = *reinterpret_cast<const float4*>(q.g + lr);
    float4 v = *reinterpret_cast<const float4*>(q.row + lr);
    v.x = b2t * v.x + (1.f - b2t) * ((g.x * g.x + eps1) / q.C);
    v.y = b2t * v.y + (1.f - b2t) * ((g.y * g.y + eps1) / q.C);
    v.z = b2t * v.z + (1.f - b2t) * ((g.z * g.z + eps1) / q.C);
    v.w = b2t * v.w + (1.f - b2t) * ((g.w * g.w + eps1) / q.C);
    *reinterpret_cast<float4*>(q.row + lr) = v;
    return;
  }
#pragma unroll
  for (int k = 0; k < ROWS_PER_TASK / 64; ++k) {
    const long lr = base + lane + 64 * k;
    if (lr < nrows) {
      const float* g = q.g + lr * q.C;
      float s = 0.f;
#pragma unroll 8     // independent loads in flight (a serial chain of load latencies otherwise)
      for (int c = 0; c < q.C; ++c) s += g[c] * g[c] + eps1;
      row_update(q, lr, s, b2t);
    }
  }
}

// one thread per factored column: col = b2t*col + (1-b2t)*mean_r(g^2 + eps1)
// wide: sum of the ada_colpart partials in row-block order; narrow: direct sum over the R rows
template <class B2>
__global__ void ada_cols(const AdaP* __restrict__ t, int n, long ncols, B2 b2, float eps1,
                         const float* __restrict__ part) {
  const float b2t = b2t_of(b2);
  const long cidx = (long)blockIdx.x * EB + threadIdx.x;
  if (cidx >= ncols) return;
  // the block's first column's parameter by a uniform (scalar) search, then a short per-lane forward scan
  int pi = find_param(t, n, (long)blockIdx.x * EB, ADA_COLS);
  while (pi + 1 < n && t[pi + 1].col_off <= cidx) ++pi;
  const AdaP& q = t[pi];
  const long lc = cidx - q.col_off;     // = b*C + j
  const int b = (int)(lc / q.C), j = (int)(lc % q.C);
  float s = 0.f;
  if (is_wide(q.C)) {
    const int nrb = (q.R + RB - 1) / RB;
    const float* pp = part + q.part_off + (long)b * nrb * q.C + j;
#pragma unroll 8     // (fixed order kept: the unrolled adds still run k = 0, 1, 2, ...)
    for (int k = 0; k < nrb; ++k) s += pp[(long)k * q.C];
  } else if (q.C == 1 && q.R % 4 == 0 && ((uintptr_t)q.g & 15) == 0) {
    // C == 1 (the pointwise-conv weights (O, I, 1): R = I rows of one element): the column is contiguous, so
    // 16-B loads, a quarter of the latency rounds; the adds keep the r = 0, 1, 2, ... order (bit-identical)
    const float4* g4 = reinterpret_cast<const float4*>(q.g + (long)b * q.R);
#pragma unroll 8
    for (int r4 = 0; r4 < q.R / 4; ++r4) {
      const float4 v = g4[r4];
      s += v.x * v.x + eps1;
      s += v.y * v.y + eps1;
      s += v.z * v.z + eps1;
      s += v.w * v.w + eps1;
    }
  } else {
    const float* g = q.g + (long)b * q.R * q.C + j;
#pragma unroll 8
    for (int r = 0; r < q.R; ++r) {
      const float v = g[(long)r * q.C];
      s += v * v + eps1;
    }
  }
  q.col[lc] = b2t * q.col[lc] + (1.f - b2t) * (s / q.R);
}

// mean over R of the row state per (param, b): wide R -> one wave per b; narrow -> 64 b per wave
__global__ void ada_rowmean(const AdaP* __restrict__ t, int n, long ntasks, float* __restrict__ rowmean) {
  const int lane = threadIdx.x & 63;
  const long task = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (task >= ntasks) return;
  const AdaP& q = t[find_param(t, n, task, ADA_ROWMEAN)];
  if (!q.factored) return;
  const long lt = task - q.rm_toff;
  if (q.R >= 64) {
    float s = 0.f;
#pragma unroll 8
    for (int r = lane; r < q.R; r += 64) s += q.row[lt * q.R + r];
    s = wave_sum(s);
    if (lane == 0) rowmean[q.rm_off + lt] = s / q.R;
  } else {
    const long b = lt * 64 + lane;
    if (b < q.nb) {
      float s = 0.f;
#pragma unroll 8
      for (int r = 0; r < q.R; ++r) s += q.row[b * q.R + r];
      rowmean[q.rm_off + b] = s / q.R;
    }
  }
}

// The update direction of 4 consecutive elements i..i+3 (same row: C % 4 == 0, i % 4 == 0) or of
// one element (n4 == 1).  32-bit index arithmetic (numel < 2^31, checked on the host).
template <int W>
__device__ __forceinline__ void ada_u(const AdaP& q, const float* rowmean, unsigned i, float b2t, float eps1,
                                      bool update_v, float (&u)[W]) {
  float g[W];
  if constexpr (W == 4) {
    const float4 v = *reinterpret_cast<const float4*>(q.g + i);
    g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
  } else {
    g[0] = q.g[i];
  }
  if (!q.factored) {
#pragma unroll
    for (int e = 0; e < W; ++e) {
      float v = q.row[i + e];
      if (update_v) {
        v = b2t * v + (1.f - b2t) * (g[e] * g[e] + eps1);
        q.row[i + e] = v;
      }
      u[e] = g[e] * rsqrtf(v);
    }
    return;
  }
  // (the two divisions by the tensor's R*C and C as multiply-high sequences: as plain 32-bit divisions they were
  // ~40 VALU per element group in two HBM-bound passes)
  const unsigned rc = (unsigned)q.R * (unsigned)q.C;
  const unsigned b = udiv(i, q.div_rc), w = i - b * rc;
  const unsigned r = udiv(w, q.div_c), c = w - r * (unsigned)q.C;
  const float rf = rsqrtf(q.row[(long)b * q.R + r] / rowmean[q.rm_off + b]);
  const float* cp = q.col + (long)b * q.C + c;
#pragma unroll
  for (int e = 0; e < W; ++e) u[e] = g[e] * rf * rsqrtf(cp[e]);
}

__device__ __forceinline__ bool vec4_ok(const AdaP& q) {
  return (q.numel % 4 == 0) && (!q.factored || q.C % 4 == 0) && ((uintptr_t)q.g % 16 == 0) &&
         ((uintptr_t)q.p % 16 == 0) && (!q.m || (uintptr_t)q.m % 16 == 0) &&
         (q.factored || (uintptr_t)q.row % 16 == 0);
}

// What scale_parameter / weight_decay / the device step add to the two elementwise kernels, as a trailing kernel
// argument that is empty without them (<false>: the kernels of a step without them; no extra load or store).
template <bool PRMS> struct SumsqEx {};
template <> struct SumsqEx<true> { float* partial_p; };   // per-block sums of p^2
template <bool EX> struct ApplyEx {};
// rel = sc ? sc[SC_REL] : lr;  lr_p = rel * (partial_p ? max(eps2, RMS(p)) : 1), RMS(p) -> rms_out[param];
// p += -wd * lr_p * p before p -= update  (transformers.Adafactor._get_lr and its weight decay)
template <> struct ApplyEx<true> {
  const float* partial_p; const float* sc; float* rms_out;
  float eps2, wd;
};

// per-block sum of u^2 -> partial[blk] (summed in block order by ada_apply: deterministic)
// PRMS (scale_parameter): the same pass reads p and writes the block's sum of p^2 -> partial_p[blk]; that is p
// before this step's update, which ada_apply makes in the next launch.
template <bool PRMS, class B2>
__global__ __launch_bounds__(EB) void ada_sumsq(const AdaP* __restrict__ t, int n, const float* __restrict__ rowmean,
                                                B2 b2, float eps1, float* __restrict__ partial, SumsqEx<PRMS> ex) {
  const float b2t = b2t_of(b2);
  __shared__ float red[EB / 64];
  __shared__ float redp[PRMS ? EB / 64 : 1];
  const int pi = find_param(t, n, blockIdx.x, ADA_BLOCKS);
  const AdaP& q = t[pi];
  const long start = (long)(blockIdx.x - q.blk_off) * CHUNK;
  const long end = min(q.numel, start + CHUNK);
  float s = 0.f, sp = 0.f;
  if (vec4_ok(q)) {
    // CHUNK / (4 EB) = 4 float4 steps per thread, unrolled: their loads are in flight together
#pragma unroll
    for (int j = 0; j < CHUNK / (4 * EB); ++j) {
      const long i = start + 4 * threadIdx.x + (long)j * 4 * EB;
      if (i < end) {
        float u[4];
        ada_u<4>(q, rowmean, (unsigned)i, b2t, eps1, true, u);
        s += u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3];
        if constexpr (PRMS) {
          const float4 p = *reinterpret_cast<const float4*>(q.p + i);
          sp += p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w;
        }
      }
    }
  } else {
    for (long i = start + threadIdx.x; i < end; i += EB) {
      float u[1];
      ada_u<1>(q, rowmean, (unsigned)i, b2t, eps1, true, u);
      s += u[0] * u[0];
      if constexpr (PRMS) sp += q.p[i] * q.p[i];
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  if constexpr (PRMS) {
    sp = wave_sum(sp);
    if ((threadIdx.x & 63) == 0) redp[threadIdx.x >> 6] = sp;
  }
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
  if constexpr (PRMS) {
    if (threadIdx.x == 0) ex.partial_p[blockIdx.x] = redp[0] + redp[1] + redp[2] + redp[3];
  }
}

template <bool EX>
__global__ __launch_bounds__(EB) void ada_apply(const AdaP* __restrict__ t, int n, const float* __restrict__ rowmean,
                                                float b2t, float eps1, const float* __restrict__ partial, float lr,
                                                float beta1, float clip, ApplyEx<EX> ex) {
  __shared__ float red[EB / 64];
  __shared__ float redp[EX ? EB / 64 : 1];
  const int pi = find_param(t, n, blockIdx.x, ADA_BLOCKS);
  const AdaP& q = t[pi];
  // RMS(u) of the whole tensor: its blocks' partials in block order
  const int nblk = (int)((q.numel + CHUNK - 1) / CHUNK);
  float ps = 0.f;
  for (int k = threadIdx.x; k < nblk; k += EB) ps += partial[q.blk_off + k];
  ps = wave_sum(ps);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ps;
  if constexpr (EX) {
    if (ex.partial_p) {   // RMS(p): the same fixed order
      float pp = 0.f;
      for (int k = threadIdx.x; k < nblk; k += EB) pp += ex.partial_p[q.blk_off + k];
      pp = wave_sum(pp);
      if ((threadIdx.x & 63) == 0) redp[threadIdx.x >> 6] = pp;
    }
  }
  __syncthreads();
  const float sumsq = red[0] + red[1] + red[2] + red[3];
  const long start = (long)(blockIdx.x - q.blk_off) * CHUNK;
  const long end = min(q.numel, start + CHUNK);
  const float rms = sqrtf(sumsq / (float)q.numel);
  [[maybe_unused]] float decay = 0.f;
  if constexpr (EX) {
    if (ex.sc) lr = ex.sc[SC_REL];
    if (ex.partial_p) {
      const float rms_p = sqrtf((redp[0] + redp[1] + redp[2] + redp[3]) / (float)q.numel);
      lr *= fmaxf(ex.eps2, rms_p);
      // every block of the tensor holds the same value; its first block stores it
      if (blockIdx.x == q.blk_off && threadIdx.x == 0) ex.rms_out[pi] = rms_p;
    }
    decay = -ex.wd * lr;
  }
  const float scale = lr / fmaxf(rms / clip, 1.f);
  if (vec4_ok(q)) {
    // the CHUNK / (4 EB) = 4 steps unrolled with every load (g, factors, m, p) issued before the first store: vmcnt
    // counts loads and stores in one in-order queue, so step j + 1's loads behind step j's stores waited for them
    constexpr int NJ = CHUNK / (4 * EB);
    float u[NJ][4];
    float4 mv[NJ], pv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const long i = start + 4 * threadIdx.x + (long)j * 4 * EB;
      if (i < end) {
        ada_u<4>(q, rowmean, (unsigned)i, b2t, eps1, false, u[j]);
        if (q.m) mv[j] = *reinterpret_cast<const float4*>(q.m + i);
        pv[j] = *reinterpret_cast<const float4*>(q.p + i);
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const long i = start + 4 * threadIdx.x + (long)j * 4 * EB;
      if (i >= end) break;
      float4 upd = make_float4(u[j][0] * scale, u[j][1] * scale, u[j][2] * scale, u[j][3] * scale);
      if (q.m) {
        const float4 m = mv[j];
        upd.x = beta1 * m.x + (1.f - beta1) * upd.x;
        upd.y = beta1 * m.y + (1.f - beta1) * upd.y;
        upd.z = beta1 * m.z + (1.f - beta1) * upd.z;
        upd.w = beta1 * m.w + (1.f - beta1) * upd.w;
        *reinterpret_cast<float4*>(q.m + i) = upd;
      }
      float4 p = pv[j];
      if constexpr (EX) {
        if (ex.wd != 0.f) { p.x += decay * p.x; p.y += decay * p.y; p.z += decay * p.z; p.w += decay * p.w; }
      }
      p.x -= upd.x; p.y -= upd.y; p.z -= upd.z; p.w -= upd.w;
      *reinterpret_cast<float4*>(q.p + i) = p;
    }
  } else {
    for (long i = start + threadIdx.x; i < end; i += EB) {
      float u[1];
      ada_u<1>(q, rowmean, (unsigned)i, b2t, eps1, false, u);
      float upd = u[0] * scale;
      if (q.m) {
        upd = beta1 * q.m[i] + (1.f - beta1) * upd;
        q.m[i] = upd;
      }
      if constexpr (EX) {
        if (ex.wd != 0.f) q.p[i] += decay * q.p[i];
      }
      q.p[i] -= upd;
    }
  }
}

// The device step (capturable): ++*step, then the two scalars the host path computes from its Python step count,
// in double as the host does (math.pow / math.sqrt, rounded to float once).  One thread.
__global__ void ada_scalars(int* __restrict__ step, float* __restrict__ sc, double decay_rate, float lr, int relative,
                            int warmup) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int s = *step + 1;
  *step = s;
  sc[SC_B2T] = (float)(1.0 - pow((double)s, decay_rate));
  double rel = lr;
  if (relative) rel = fmin(warmup ? 1e-6 * s : 1e-2, 1.0 / sqrt((double)s));
  sc[SC_REL] = (float)rel;
}

}  // namespace

CFM_EXPORT size_t cfm_adafactor_table_bytes(int n_params) { return (size_t)n_params * sizeof(AdaP); }

CFM_EXPORT int cfm_adafactor_fill_table(void* host_table, const cfm_adafactor_param* params, int n,
                                        cfm_adafactor_totals* totals) {
  CFM_REQUIRE(host_table, CFM_ERR_ARG, "bad args");
  std::vector<cfm_adafactor_totals> before(n > 0 ? n : 0);
  if (const int rc = cfm_adafactor_plan(params, n, before.data(), totals)) return rc;
  static_assert(sizeof(AdaP) == 144, "no padding: the host compares tables byte by byte");
  for (int i = 0; i < n; ++i) {
    const cfm_adafactor_param& q = params[i];
    const cfm_adafactor_totals& b = before[i];
    CFM_REQUIRE(q.p && q.g && q.row && (q.col != nullptr) == (q.factored != 0), CFM_ERR_ARG, "null pointer");
    reinterpret_cast<AdaP*>(host_table)[i] =
        AdaP{q, b.row_tasks, b.cols, b.blocks, b.rowmean_floats, b.rowmean_tasks, b.colpart_tasks, b.part_floats,
             udiv_make((uint32_t)q.R * (uint32_t)q.C), udiv_make((uint32_t)q.C)};
  }
  return CFM_OK;
}

// The launch sequence of one step: the grids from the plan's totals, the variant from the hyper-parameters alone.
CFM_EXPORT int cfm_adafactor_step(const void* dev_table, int n, const cfm_adafactor_totals* tot,
                                  const cfm_adafactor_buffers* buf, const cfm_adafactor_hyper* h, void* stream) {
  CFM_REQUIRE(h, CFM_ERR_ARG, "null hyper-parameters");
  const bool dev = h->flags & CFM_ADA_DEVICE_STEP, scale = h->flags & CFM_ADA_SCALE_PARAMETER;
  CFM_REQUIRE(!dev || (h->step_dev && h->scalars_dev), CFM_ERR_ARG, "device step without step / scalar pointers");
  CFM_REQUIRE(!scale || (buf && buf->partial_p && buf->rms_out), CFM_ERR_ARG,
              "scale_parameter without the p^2 partial / RMS buffers");
  CFM_REQUIRE(dev_table && tot && buf && buf->rowmean && buf->partial && n > 0 &&
                  (tot->colpart_tasks == 0 || buf->part), CFM_ERR_ARG, "bad args");
  const AdaP* t = reinterpret_cast<const AdaP*>(dev_table);
  hipStream_t s = cfm::as_stream(stream);
  const dim3 eb(EB), g_cp((unsigned)tot->colpart_tasks), g_rows((unsigned)((tot->row_tasks + 3) / 4)),
      g_cols((unsigned)((tot->cols + EB - 1) / EB)), g_rm((unsigned)((tot->rowmean_tasks + 3) / 4)),
      g_blk((unsigned)tot->blocks);
  // the passes that read beta2t (statistics, row means, the update's sum of squares): the host's float or the scalars
  auto moments = [&](auto b2) {
    using B2 = decltype(b2);
    if (tot->colpart_tasks > 0)
      hipLaunchKernelGGL(ada_colpart<B2>, g_cp, eb, 0, s, t, n, tot->colpart_tasks, b2, h->eps1, buf->part);
    if (tot->row_tasks > 0)
      hipLaunchKernelGGL(ada_rows<B2>, g_rows, eb, 0, s, t, n, tot->row_tasks, b2, h->eps1);
    if (tot->cols > 0)
      hipLaunchKernelGGL(ada_cols<B2>, g_cols, eb, 0, s, t, n, tot->cols, b2, h->eps1, buf->part);
    if (tot->rowmean_tasks > 0)
      hipLaunchKernelGGL(ada_rowmean, g_rm, eb, 0, s, t, n, tot->rowmean_tasks, buf->rowmean);
    if (scale)
      hipLaunchKernelGGL((ada_sumsq<true, B2>), g_blk, eb, 0, s, t, n, buf->rowmean, b2, h->eps1, buf->partial,
                         SumsqEx<true>{buf->partial_p});
    else
      hipLaunchKernelGGL((ada_sumsq<false, B2>), g_blk, eb, 0, s, t, n, buf->rowmean, b2, h->eps1, buf->partial,
                         SumsqEx<false>{});
  };
  if (dev) {
    hipLaunchKernelGGL(ada_scalars, dim3(1), dim3(64), 0, s, h->step_dev, h->scalars_dev, h->decay_rate, h->lr,
                       (int)((h->flags & CFM_ADA_RELATIVE_STEP) != 0), (int)((h->flags & CFM_ADA_WARMUP_INIT) != 0));
    moments(static_cast<const float*>(h->scalars_dev));
  } else {
    moments(h->beta2t);
  }
  // (the apply pass does not read beta2t: ada_sumsq has updated the second moments)
  if (dev || scale || h->weight_decay != 0.f)     // anything ada_apply<false> does not do
    hipLaunchKernelGGL(ada_apply<true>, g_blk, eb, 0, s, t, n, buf->rowmean, h->beta2t, h->eps1, buf->partial, h->lr,
                       h->beta1, h->clip, ApplyEx<true>{scale ? buf->partial_p : nullptr,
                                                        dev ? h->scalars_dev : nullptr, buf->rms_out, h->eps2,
                                                        h->weight_decay});
  else
    hipLaunchKernelGGL(ada_apply<false>, g_blk, eb, 0, s, t, n, buf->rowmean, h->beta2t, h->eps1, buf->partial, h->lr,
                       h->beta1, h->clip, ApplyEx<false>{});
  return cfm::check_launch("cfm_adafactor_step");
}
