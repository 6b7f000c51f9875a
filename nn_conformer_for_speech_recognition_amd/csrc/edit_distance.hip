// edit_distance.hip — batched Levenshtein distance over token ids on the device: the word error rate's numerator
// (the vocabulary's tokens are words), with the aligned pairs on request.  The fifth CTC-adjacent operation beside
// the loss, the greedy decode, the beam search and the forced alignment; it replaces the host loop of myvocab.wer
// (jiwer's wer, reference runner.py:160,230) and supplies the pairs of the reference's confusion matrix
// (evals.py:64).
//
// Pair p compares hypothesis row p with reference row p / group (group = N: an n-best list against one transcript).
//   D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
// Kernels:
//   ed_recursion<OPS>  one wave per pair, the reference in strips of 64 rows: lane l of strip k owns row
//                      i = 64 k + l + 1 and at step t the column j = t - l + 1 (the anti-diagonal i + j = const moves
//                      through the wave).  Left is the lane's own previous value, up is the lower neighbour's
//                      previous value (one DPP wave shift per step), diagonal is the up value of the step before; the
//                      hypothesis token travels along the lanes by the same shift.  Lane 0 takes the row above the
//                      strip (row 0: j itself; else the previous strip's bottom row, carried in LDS) and the
//                      hypothesis token from registers loaded 16 steps at a time, one chunk ahead.  A pair with
//                      R <= 64 is one strip and touches no LDS; there is no barrier anywhere (one wave per workgroup)
//                      and every trip count is a function of R and H alone.  <true>: the direction of every cell
//                      (0 diagonal, 1 up, 2 left), 2 bits each, 16 steps of a lane packed into one 32-bit word,
//                      stored as [strip][word][lane] (a wave's store is 256 contiguous bytes).
//   ed_backtrace       one wave per pair (a launch of its own, so the directions are visible without fences): walks
//                      from (R, H) to (0, 0), wave-uniform, the 64 lanes holding one [strip][word] line of directions
//                      (8 to 16 moves per load), logs the visited cells in LDS, then emits the pairs in forward order
//                      and counts hits / substitutions / deletions / insertions, all lanes in parallel.
// Tie rule (part of the contract): the first of diagonal, up, left that attains the minimum; i == 0 walks left,
// j == 0 walks up.
#include "ctc_common.h"

namespace {

constexpr int ED_MAX = 1024;   // longest reference / hypothesis
constexpr int CH = 16;         // steps per chunk = cells per direction word

struct EdP {
  const int32_t* ref; int ldr; const int32_t* ref_len;
  const int32_t* hyp; int ldh; const int32_t* hyp_len;
  int group, Rmax, Hmax;
  int W;                        // direction words per lane and strip: ceil((Hmax + 63) / 16)
  int strips;                   // ceil(Rmax / 64)
  uint32_t* dirs;               // (P, strips, W, 64) or nullptr
};

// lengths are device data, clamped to the buffers' extents: a bad value can give a wrong answer, never an access
// outside ref / hyp / the workspace / the outputs
// (ctc_common.h's clamp; ref_len and hyp_len are never null: the entry point requires them)
__device__ __forceinline__ int ref_len_of(const EdP& p, int pair) { return ctc::clamp0(p.ref_len[pair / p.group], p.Rmax); }
__device__ __forceinline__ int hyp_len_of(const EdP& p, int pair) { return ctc::clamp0(p.hyp_len[pair], p.Hmax); }

template <bool OPS>
__global__ __launch_bounds__(64) void ed_recursion(EdP p, int32_t* __restrict__ dist) {
  // row 64 k of the table (columns 0 .. H): written by lane 63 of strip k - 1, read by lane 0 of strip k.  In place:
  // at step t lane 63 writes column t - 62 while lane 0 has already read every column up to t + 1.
  __shared__ int32_t carry[ED_MAX + 1];
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int R = ref_len_of(p, pair), H = hyp_len_of(p, pair);
  const int32_t* r = p.ref + (long)(pair / p.group) * p.ldr;
  const int32_t* h = p.hyp + (long)pair * p.ldh;
  const int nstrips = (R + 63) >> 6;
  int result = H;   // R == 0
  for (int k = 0; k < nstrips; ++k) {
    const bool first = k == 0, last = k + 1 == nstrips;   // uniform
    const int i = 64 * k + lane + 1;                      // this lane's row
    const int nrows = min(64, R - 64 * k);
    const bool row_ok = lane < nrows;
    const int rtok = r[min(i, R) - 1];
    const int nsteps = H > 0 ? H + nrows - 1 : 0;
    uint32_t* dst = OPS ? p.dirs + (((long)pair * p.strips + k) * p.W) * 64 + lane : nullptr;
    int cur = i;        // D[i][0]
    int diag = i - 1;   // D[i-1][0]
    int htok = 0;
    // lane q of a chunk's registers: the row above at column t0 + q + 1 and the hypothesis token of column t0 + q + 1
    auto fetch = [&](int t0, int& top, int& tok) {
      const int c = min(t0 + (lane & (CH - 1)), H - 1);   // column - 1, inside the hypothesis (H >= 1 here)
      top = first ? c + 1 : carry[c + 1];
      tok = h[c];
    };
    int top_c = 0, tok_c = 0, top_n = 0, tok_n = 0;
    if (nsteps > 0) fetch(0, top_c, tok_c);
    for (int t0 = 0; t0 < nsteps; t0 += CH) {
      fetch(t0 + CH, top_n, tok_n);   // clamped: past the end it re-reads the last column
      uint32_t word = 0;
#pragma unroll
      for (int q = 0; q < CH; ++q) {
        const int t = t0 + q;
        const int top_q = __builtin_amdgcn_readlane(top_c, q), tok_q = __builtin_amdgcn_readlane(tok_c, q);
        const int cur_s = wave_shr1(cur), tok_s = wave_shr1(htok);   // all lanes take part in the shifts
        const int up = lane == 0 ? top_q : cur_s;
        htok = lane == 0 ? tok_q : tok_s;
        const int j = t - lane + 1;
        const bool active = row_ok && j >= 1 && j <= H;
        int best = diag + (rtok != htok ? 1 : 0);
        uint32_t dir = 0;
        if (up + 1 < best) { best = up + 1; dir = 1; }
        if (cur + 1 < best) { best = cur + 1; dir = 2; }
        cur = active ? best : cur;
        diag = up;
        if (OPS) word |= (active ? dir : 0u) << (2 * q);
        if (!last && lane == 63 && active) carry[j] = cur;
      }
      if (OPS && row_ok) dst[(long)(t0 / CH) * 64] = word;
      top_c = top_n;
      tok_c = tok_n;
    }
    if (last) result = __shfl(cur, (R - 1) & 63, 64);   // D[R][H] (H == 0: the lane's initial value, R)
    // the next strip's reads of carry come after this strip's writes: same wave, LDS operations complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (lane == 0) dist[pair] = result;
}

// cell log of the walk: i (11 bits) << 13 | j (11 bits) << 2 | move
__global__ __launch_bounds__(64) void ed_backtrace(EdP p, int32_t* __restrict__ counts, int32_t* __restrict__ pair_ref,
                                                   int32_t* __restrict__ pair_hyp, int ldp,
                                                   int32_t* __restrict__ n_pairs) {
  __shared__ uint32_t cells[2 * ED_MAX];
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int R = ref_len_of(p, pair), H = hyp_len_of(p, pair);
  const int32_t* r = p.ref + (long)(pair / p.group) * p.ldr;
  const int32_t* h = p.hyp + (long)pair * p.ldh;
  const uint32_t* dirs = p.dirs + (long)pair * p.strips * p.W * 64;
  int i = R, j = H, n = 0;      // wave-uniform
  int line = -1;                // strip * W + word held in `words` (-1: none)
  uint32_t words = 0;
  while (i > 0 || j > 0) {      // i + j drops by at least 1 per trip: at most R + H trips
    int mv;
    if (i == 0) mv = 2;
    else if (j == 0) mv = 1;
    else {
      const int l = (i - 1) & 63, s = j - 1 + l;
      const int want = ((i - 1) >> 6) * p.W + (s >> 4);
      if (want != line) {
        line = want;
        words = dirs[(long)line * 64 + lane];
      }
      mv = (__builtin_amdgcn_readlane(words, __builtin_amdgcn_readfirstlane(l)) >> (2 * (s & 15))) & 3;
      if (mv == 3) mv = 0;      // never written by the recursion; any of the three moves keeps the walk inside
    }
    if (lane == 0) cells[n] = ((uint32_t)i << 13) | ((uint32_t)j << 2) | (uint32_t)mv;
    ++n;
    i -= mv != 2;
    j -= mv != 1;
  }
  __syncthreads();
  int hits = 0, subs = 0, dels = 0, ins = 0;
  const bool pairs = pair_ref != nullptr;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    const bool ok = k < n;
    const uint32_t c = cells[min(k, n - 1)];
    const int ci = (int)(c >> 13), cj = (int)((c >> 2) & 2047u), mv = (int)(c & 3u);
    const int a = mv != 2 ? r[max(ci, 1) - 1] : -1;   // mv != 2 implies ci >= 1, mv != 1 implies cj >= 1
    const int b = mv != 1 ? h[max(cj, 1) - 1] : -1;
    hits += __popcll(__ballot(ok && mv == 0 && a == b));
    subs += __popcll(__ballot(ok && mv == 0 && a != b));
    dels += __popcll(__ballot(ok && mv == 1));
    ins += __popcll(__ballot(ok && mv == 2));
    if (pairs && ok) {
      pair_ref[(long)pair * ldp + (n - 1 - k)] = a;
      pair_hyp[(long)pair * ldp + (n - 1 - k)] = b;
    }
  }
  if (pairs) {
    for (int k = n + lane; k < ldp; k += 64) {
      pair_ref[(long)pair * ldp + k] = -1;
      pair_hyp[(long)pair * ldp + k] = -1;
    }
    if (lane == 0) n_pairs[pair] = n;
  }
  if (counts && lane == 0) {
    int32_t* c = counts + (long)pair * 4;
    c[0] = hits; c[1] = subs; c[2] = dels; c[3] = ins;
  }
}

void ed_geometry(int Rmax, int Hmax, int& W, int& strips) {
  W = (Hmax + 63 + CH - 1) / CH;
  strips = (Rmax + 63) / 64;
}

}  // namespace

CFM_EXPORT size_t cfm_edit_distance_ws_bytes(int P, int Rmax, int Hmax, int want_ops) {
  if (P <= 0 || Rmax < 0 || Hmax < 0 || !want_ops) return 0;
  int W, strips;
  ed_geometry(Rmax, Hmax, W, strips);
  return (size_t)P * strips * W * 64 * sizeof(uint32_t);
}

CFM_EXPORT int cfm_edit_distance(const int32_t* ref, int ldr, const int32_t* ref_len, int n_ref, const int32_t* hyp,
                                 int ldh, const int32_t* hyp_len, int P, int group, int Rmax, int Hmax, int32_t* dist,
                                 int32_t* counts, int32_t* pair_ref, int32_t* pair_hyp, int ldp, int32_t* n_pairs,
                                 void* ws, void* stream) {
  CFM_REQUIRE(ref_len && hyp_len && dist, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(P >= 0 && n_ref >= 0 && group > 0 && Rmax >= 0 && Hmax >= 0 && ldr >= 0 && ldh >= 0, CFM_ERR_ARG,
              "negative size");
  CFM_REQUIRE(P % group == 0 && P == n_ref * group, CFM_ERR_ARG, "P must be n_ref * group");
  CFM_REQUIRE((ref || Rmax == 0) && (hyp || Hmax == 0), CFM_ERR_ARG, "null ids");
  CFM_REQUIRE((pair_ref != nullptr) == (pair_hyp != nullptr) && (pair_hyp != nullptr) == (n_pairs != nullptr),
              CFM_ERR_ARG, "pair_ref, pair_hyp and n_pairs: all three or none");
  CFM_REQUIRE(Rmax <= ED_MAX && Hmax <= ED_MAX, CFM_ERR_UNSUPPORTED, "Rmax and Hmax must be <= 1024");
  CFM_REQUIRE(Rmax <= ldr && Hmax <= ldh, CFM_ERR_SHAPE, "Rmax <= ldr and Hmax <= ldh required");
  const bool want_ops = counts || pair_ref;
  CFM_REQUIRE(!pair_ref || ldp >= Rmax + Hmax, CFM_ERR_SHAPE, "ldp >= Rmax + Hmax required");
  if (P == 0) return CFM_OK;
  EdP p;
  p.ref = ref; p.ldr = ldr; p.ref_len = ref_len; p.hyp = hyp; p.ldh = ldh; p.hyp_len = hyp_len;
  p.group = group; p.Rmax = Rmax; p.Hmax = Hmax;
  ed_geometry(Rmax, Hmax, p.W, p.strips);
  p.dirs = static_cast<uint32_t*>(ws);
  // Rmax == 0: no cell has a stored direction and the workspace is empty
  CFM_REQUIRE(!want_ops || ws || p.strips == 0, CFM_ERR_ARG, "null workspace");
  hipStream_t s = cfm::as_stream(stream);
  if (want_ops) {
    hipLaunchKernelGGL(ed_recursion<true>, dim3(P), dim3(64), 0, s, p, dist);
    hipLaunchKernelGGL(ed_backtrace, dim3(P), dim3(64), 0, s, p, counts, pair_ref, pair_hyp, ldp, n_pairs);
  } else {
    hipLaunchKernelGGL(ed_recursion<false>, dim3(P), dim3(64), 0, s, p, dist);
  }
  return cfm::check_launch("cfm_edit_distance");
}
