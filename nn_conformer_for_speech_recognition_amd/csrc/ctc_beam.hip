// ctc_beam.hip — CTC prefix beam search on the device, without a language model or with a back-off n-gram fused in.
//
//   cfm_ctc_beam_decode is the alternative to the per-frame argmax of ASRNN.predict (asrnn.py:48-58) and of the
//   Runner's metric / pseudo-label passes (runner.py:150,220,275): instead of following one alignment it sums the
//   alignments of each label prefix.  The surface is modelled on torchaudio's CUDA CTC decoder.
//
// A beam entry is a label prefix l with p_b(l) / p_nb(l), the log-probabilities of its kept alignments ending in
// blank / non-blank.  Per frame with log-probabilities r every entry contributes
//   stay      p_b'(l)   (+)= (p_b (+) p_nb)(l) + r[blank];   p_nb'(l) (+)= p_nb(l) + r[last(l)]   (l non-empty)
//   extend    p_nb'(l+c) (+)= r[c] + (c == last(l) ? p_b(l) : (p_b (+) p_nb)(l))     for c not in {blank, pad}
// ((+) = log-sum-exp); an extension whose result is itself in the beam lands on that entry; the W best survive.
//
// Three launches, no host synchronisation, no communication between workgroups (B utterances, T frames, V classes,
// W beam width):
//   beam_topk      one wave per frame row, the row read once into LDS: its log-sum-exp, r[blank] and the
//                  K = min(W + 1, #tokens) best non-blank / non-pad tokens, sorted (lower id first among equals)
//   beam_search    one workgroup per utterance, the beam in LDS, frames in sequence.  An extension scores
//                  base_i + r[c], so with 0-based beam rank a and token rank b only the pairs (a + 1) * b <= W can
//                  reach the top W: about W (1 + ln W) candidates plus the W stays; the W best by rank counting.
//                  (The tighter (a + 1)(b + 1) <= W with W tokens is NOT sufficient: the repeat-token extension
//                  scores below its bound and merged extensions leave the list, so a beam can lose one dominating
//                  pair.)  Prefix identity is a 64-bit rolling hash plus the length; the extension that merges into
//                  a live entry is found through the hash of that entry's parent prefix and takes r[last] from a
//                  gather of the row, whatever the pruning rule kept.  Scores are kept relative to the frame's best
//                  entry, the offset accumulated in double.  Back-pointers go out with ordinary vector stores.
//   beam_backtrace one wave per utterance: the back-pointer table staged through LDS in chunks of frames, one lane
//                  per hypothesis walking it (once to count, once to write).
//
// cfm_ctc_beam_decode_lm fuses a back-off n-gram LM (order <= 3; lm.py packs it) into the search: shallow fusion, which
// the reference only names (runner.py:78-101 adds a transformer LM's weights under keys that match nothing).  The
// extension becomes r[c] + alpha * lm(c | h(l)) + beta + ..., h(l) the last min(N - 1, |l| + 1) symbols of <s> + l.
// beam_search<true> differs from the kernel above in four places:
//   candidates     an LM term breaks the base_a + r[c_b] ordering the pair rule rests on, so every entry is extended
//                  by the K = token_beam acoustically best tokens: W + W K candidates (<= 1024), owner / start are a
//                  division;
//   LM term        alpha * lm + beta is a function of the prefix alone: it is kept with the entry (lt) so that an
//                  extension merging into a live entry adds the same term; per candidate the probes (u, v, c),
//                  (v, c) and uni[c] are independent loads issued together, each probe reading its 4 slots
//                  unconditionally and selecting afterwards; the context back-offs bo(u, v), bo(v) belong to the
//                  entry and are fetched where r[last] is gathered, into LDS;
//   fault safety   every index formed from a hash, a table word or a token id is masked with the capacity mask or
//                  clamped to [0, V + 1] before it addresses memory: a malformed table gives wrong scores, never an
//                  out-of-range access;
//   sentence end   the final scores add alpha * lm(</s> | h(l)) (eos) and a W-element rank count writes the slot
//                  permutation beam_backtrace follows (null: identity, the no-LM order).
#include "ctc_common.h"

using namespace ctc;

namespace {

constexpr int BEAM_MAX = 128;
constexpr int BT_LDS = 4096;   // back-pointer entries per LDS chunk of the backtrace

// ------------------------------------------------------------------------------------------ n-gram tables
struct LmP {
  const float2* uni;     // (V + 2) {logp, backoff}
  const uint4* tab;      // (mask + 1) slots {key lo, key hi, logp, backoff}
  uint64_t seed;
  uint32_t mask;
  int probe, order, V;
  float alpha, beta;
  int eos;               // add alpha * lm(</s> | h) to the final scores
};

__device__ __forceinline__ uint64_t lm_key2(int v, int c) { return (2ull << 45) | ((uint64_t)v << 15) | (uint64_t)c; }
__device__ __forceinline__ uint64_t lm_key3(int u, int v, int c) {
  return (3ull << 45) | ((uint64_t)u << 30) | ((uint64_t)v << 15) | (uint64_t)c;
}
__device__ __forceinline__ int lm_id(int c, int V) { return min(max(c, 0), V + 1); }

struct LmHit { float lp, bo; bool hit; };
// all four slots are loaded whatever they hold (a load that depends on the previous slot's key would serialise L2
// round trips); the slot index is masked, so any table word is a safe address
__device__ __forceinline__ LmHit lm_probe(const LmP& lm, uint64_t key) {
  uint64_t z = (key ^ lm.seed) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 32)) * 0xBF58476D1CE4E5B9ull;
  z ^= z >> 29;
  const uint32_t h = (uint32_t)z & lm.mask;
  uint4 s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = lm.tab[(h + (uint32_t)j) & lm.mask];
  LmHit r{0.f, 0.f, false};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t k = ((uint64_t)s[j].y << 32) | (uint64_t)s[j].x;
    if (j < lm.probe && k == key) { r.lp = __uint_as_float(s[j].z); r.bo = __uint_as_float(s[j].w); r.hit = true; }
  }
  return r;
}
// lm(c | u, v): u < 0: the context is (v) alone; bo2 = bo(u, v), bo1 = bo(v) (0 where the order has no such context)
__device__ __forceinline__ float lm_score(const LmP& lm, int u, int v, int c, float bo2, float bo1) {
  const int cu = lm_id(u, lm.V), cv = lm_id(v, lm.V), cc = lm_id(c, lm.V);
  const LmHit t = lm_probe(lm, lm_key3(cu, cv, cc));
  const LmHit d = lm_probe(lm, lm_key2(cv, cc));
  const float2 g = lm.uni[cc];
  const float low = (lm.order >= 2 && d.hit) ? d.lp : bo1 + g.x;
  return (lm.order >= 3 && u >= 0 && t.hit) ? t.lp : bo2 + low;
}
// the back-offs of an entry's context: u < 0: no second symbol
__device__ __forceinline__ void lm_context(const LmP& lm, int u, int v, float& bo2, float& bo1) {
  const int cu = lm_id(u, lm.V), cv = lm_id(v, lm.V);
  const LmHit d = lm_probe(lm, lm_key2(cu, cv));
  const float2 g = lm.uni[cv];
  bo1 = lm.order >= 2 ? g.y : 0.f;
  bo2 = (lm.order >= 3 && u >= 0 && d.hit) ? d.bo : 0.f;
}

// ------------------------------------------------------------------------------------------ top-k per row
__global__ __launch_bounds__(256) void beam_topk(const float* __restrict__ x, long sb, long st,
                                                 const int32_t* __restrict__ lens, int B, int T, int V, int blank,
                                                 int pad, int K, int KP, float* __restrict__ row_lse,
                                                 float* __restrict__ row_rb, int32_t* __restrict__ tk,
                                                 float* __restrict__ tlp) {
  extern __shared__ float topk_sm[];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * (blockDim.x >> 6) + w;
  if (row >= (long)B * T) return;   // (no workgroup barrier below: each lane only touches its own LDS elements)
  const int b = (int)(row / T), t = (int)(row % T);
  if (t >= clamp_len(lens, b, T)) return;
  const float* r = x + b * sb + t * st;
  float* key = topk_sm + (size_t)w * V;
  float m = NEG_INF;
  for (int v = lane; v < V; v += 64) {
    const float q = r[v];
    key[v] = q;
    m = fmaxf(m, q);
  }
  m = wave_max(m);
  // the sum and its logarithm in double: the row's lse enters every score of the frame, so it is kept to one fp32
  // rounding (V / 64 additions per lane and one log per row: nothing beside the row read)
  double s = 0.0;
  for (int v = lane; v < V; v += 64) s += (double)expf(key[v] - m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float lse = m == NEG_INF ? 0.f : (float)((double)m + log(s));
  const float xb = __shfl((blank & 63) == lane ? key[blank] : 0.f, blank & 63, 64);
  // taken / excluded elements are NaN
  if ((blank & 63) == lane) key[blank] = NAN;
  if (pad >= 0 && (pad & 63) == lane) key[pad] = NAN;
  float bv = NEG_INF;
  int bi = -1;
  for (int v = lane; v < V; v += 64) {
    const float q = key[v];
    if (q == q && (bi < 0 || q > bv)) { bv = q; bi = v; }
  }
  for (int j = 0; j < K; ++j) {
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (oi >= 0 && (wi < 0 || ov > wv || (ov == wv && oi < wi))) { wv = ov; wi = oi; }
    }
    if (lane == 0) {
      tk[row * KP + j] = wi;
      tlp[row * KP + j] = wi >= 0 ? wv - lse : NEG_INF;
    }
    if (wi >= 0 && (wi & 63) == lane) {
      key[wi] = NAN;
      bv = NEG_INF;
      bi = -1;
      for (int v = lane; v < V; v += 64) {
        const float q = key[v];
        if (q == q && (bi < 0 || q > bv)) { bv = q; bi = v; }
      }
    }
  }
  if (lane == 0) {
    row_lse[row] = lse;
    row_rb[row] = xb - lse;
  }
}

// ------------------------------------------------------------------------------------------ the recursion
struct BeamP {
  const float* x; long sb, st;
  const int32_t* lens;
  int B, T, V, W, K, KP, NC, NP, NE;   // NC = W stays + NE extensions; NP = NC rounded up to a power of two >= 16 (LM: to a multiple of 16)
  const float* row_lse; const float* row_rb; const int32_t* tk; const float* tlp;
  int32_t* bp_parent; int32_t* bp_token;
  float* fin;                          // (B, W) final scores
  int32_t* perm;                       // LM: (B, W) slots in descending final score
  LmP lm;
};

__device__ __forceinline__ uint64_t prefix_mix(uint64_t h, int c) {
  uint64_t z = h + 0x9E3779B97F4A7C15ull * (uint64_t)(c + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// order-preserving image of a float (no NaN): larger float, larger word
__device__ __forceinline__ uint32_t f_order(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// extension candidates of 0-based beam rank i: token ranks j with (i + 1) * j <= W, of the K listed
__host__ __device__ __forceinline__ int ext_count(int i, int W, int K) {
  const int n = W / (i + 1) + 1;
  return n < K ? n : K;
}

template <bool LM>
__global__ __launch_bounds__(256) void beam_search(const BeamP p) {
  extern __shared__ __align__(16) unsigned char beam_sm[];
  const int W = p.W, K = p.K, KP = p.KP, NP = p.NP, NC = p.NC;
  const int tid = threadIdx.x, NT = blockDim.x, b = blockIdx.x;
  uint64_t* key = reinterpret_cast<uint64_t*>(beam_sm);         // [NP]
  uint64_t* hash = key + NP;                                     // [2][W]
  uint64_t* phash = hash + 2 * W;                                // [2][W] hash of the prefix without its last label
  float* cpb = reinterpret_cast<float*>(phash + 2 * W);          // [NP]
  float* cpnb = cpb + NP;                                        // [NP]
  float* ctot = cpnb + NP;                                       // [NP]
  float* pb = ctot + NP;                                         // [2][W]
  float* pnb = pb + 2 * W;                                       // [2][W]
  float* tot = pnb + 2 * W;                                      // [2][W]  -inf: empty slot
  float* rl = tot + 2 * W;                                       // [W]  r[last label] of the current frame
  float* tlp = rl + W;                                           // [2][KP]
  int* tk = reinterpret_cast<int*>(tlp + 2 * KP);                // [2][KP]
  int* len = tk + 2 * KP;                                        // [2][W]
  int* last = len + 2 * W;                                       // [2][W]
  int* start = last + 2 * W;                                     // [W]  first extension candidate of beam rank i
  int* sel = start + W;                                          // [W]  candidate index of the new slot s
  int* parent_of = sel + W;                                      // [W]  slot of entry k's prefix less its last label
  int* owner = parent_of + W;                                    // [NE] beam rank of extension candidate e (no LM)
  // LM: per entry the second-to-last symbol (<s> = V for a one-token prefix, -1 for the empty one), the stored LM
  // term and the two context back-offs; per extension candidate its LM term
  int* prev = owner + (LM ? 0 : p.NE);                           // [2][W]
  float* lt = reinterpret_cast<float*>(prev + 2 * W);            // [2][W]
  float* bo2 = lt + 2 * W;                                       // [W]
  float* bo1 = bo2 + W;                                          // [W]
  float* clt = bo1 + W;                                          // [NE]

  const int Tb = clamp_len(p.lens, b, p.T);
  if constexpr (!LM) {
    if (tid == 0) {
      int acc = 0;
      for (int i = 0; i < W; ++i) { start[i] = acc; acc += ext_count(i, W, K); }
    }
  }
  for (int i = tid; i < 2 * W; i += NT) {
    const bool root = i == 0;
    pb[i] = root ? 0.f : NEG_INF; pnb[i] = NEG_INF; tot[i] = root ? 0.f : NEG_INF;
    hash[i] = 0; phash[i] = 0; len[i] = 0; last[i] = -1;
    if (i < W) { rl[i] = NEG_INF; parent_of[i] = -1; }
    if constexpr (LM) {
      prev[i] = -1; lt[i] = 0.f;
      if (i < W) {
        float b2 = 0.f, b1 = 0.f;
        if (root) lm_context(p.lm, -1, p.lm.V, b2, b1);
        bo2[i] = b2; bo1[i] = b1;
      }
    }
  }
  if (Tb > 0)
    for (int j = tid; j < K; j += NT) {
      tk[j] = p.tk[(long)b * p.T * KP + j];
      tlp[j] = p.tlp[(long)b * p.T * KP + j];
    }
  __syncthreads();
  if constexpr (!LM) {
    for (int i = tid; i < W; i += NT) {
      const int n = ext_count(i, W, K);
      for (int j = 0; j < n; ++j) owner[start[i] + j] = i;
    }
  }
  double off = 0.0;
  float rb_n = Tb > 0 ? p.row_rb[(long)b * p.T] : 0.f, lse_n = Tb > 0 ? p.row_lse[(long)b * p.T] : 0.f;
  __syncthreads();

  for (int t = 0; t < Tb; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const long row = (long)b * p.T + t;
    const float rb = rb_n;
    const bool more = t + 1 < Tb;
    // the next frame's token list and row constants, in flight during this frame's work
    int pk[3];
    float pl[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int j = tid + q * NT;
      const bool on = more && j < K;
      pk[q] = on ? p.tk[(row + 1) * KP + j] : -1;
      pl[q] = on ? p.tlp[(row + 1) * KP + j] : NEG_INF;
    }
    if (more) { rb_n = p.row_rb[row + 1]; lse_n = p.row_lse[row + 1]; }
    const uint64_t* hc = hash + cur * W; const uint64_t* phc = phash + cur * W;
    const float* pbc = pb + cur * W; const float* pnbc = pnb + cur * W; const float* totc = tot + cur * W;
    const int* lenc = len + cur * W; const int* lastc = last + cur * W;
    const int* tkc = tk + cur * KP; const float* tlpc = tlp + cur * KP;

    // candidates: [0, W) stays, [W, NC) extensions (beam rank i, token rank j), [NC, NP) padding
    for (int idx = tid; idx < NP; idx += NT) {
      float a = NEG_INF, c = NEG_INF;
      if (idx < W) {
        if (totc[idx] > NEG_INF) {
          a = totc[idx] + rb;
          if (lastc[idx] >= 0) c = pnbc[idx] + rl[idx];
        }
      } else if (idx < NC) {
        if constexpr (LM) {
          const int e = idx - W, i = e / K, j = e - i * K;
          const int tokn = tkc[j];
          const int li = lastc[i];
          const float term = fmaf(p.lm.alpha, lm_score(p.lm, prev[cur * W + i], li >= 0 ? li : p.lm.V, tokn, bo2[i], bo1[i]),
                                  p.lm.beta);
          clt[e] = term;
          if (totc[i] > NEG_INF && tokn >= 0) c = (tlpc[j] + term) + (tokn == li ? pbc[i] : totc[i]);
        } else {
          const int e = idx - W, i = owner[e], j = e - start[i];
          const int tokn = tkc[j];
          if (totc[i] > NEG_INF && tokn >= 0) c = tlpc[j] + (tokn == lastc[i] ? pbc[i] : totc[i]);
        }
      }
      cpb[idx] = a;
      cpnb[idx] = c;
    }
    // where the beam holds entry k's prefix less its last label (by hash and length: a prefix that left the beam and
    // was re-created sits in a new slot while its old descendants live on).  Thread i keeps its own entries in
    // registers and meets every k through broadcast reads; at most one i matches a k.
    {
      uint64_t hi[2];
      int li[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int i = tid + q * NT;
        const bool live = i < W && totc[i] > NEG_INF;
        hi[q] = live ? hc[i] : 0;
        li[q] = live ? lenc[i] : -2;
      }
#pragma unroll 4
      for (int k = 0; k < W; ++k) {
        const uint64_t want = phc[k];
        const int lk = totc[k] > NEG_INF ? lenc[k] - 1 : -3;
#pragma unroll
        for (int q = 0; q < 2; ++q)
          if (li[q] == lk && hi[q] == want) parent_of[k] = tid + q * NT;
      }
    }
    lds_barrier();
    // an extension that re-creates a live entry k lands on k (and leaves the list if the pruning rule kept it)
    for (int k = tid; k < W; k += NT) {
      const int par = parent_of[k];
      if (par < 0) continue;
      const int e = lastc[k];
      if constexpr (LM)   // the entry's own LM term: the same sum as the candidate's, in the same order
        cpnb[k] = lse2(cpnb[k], (rl[k] + lt[cur * W + k]) + (lastc[par] == e ? pbc[par] : totc[par]));
      else
        cpnb[k] = lse2(cpnb[k], rl[k] + (lastc[par] == e ? pbc[par] : totc[par]));
      const int n = LM ? K : ext_count(par, W, K);
      int hit = -1;
#pragma unroll 4
      for (int j = 0; j < n; ++j)
        if (tkc[j] == e) hit = j;
      if (hit >= 0) cpnb[W + (LM ? par * K : start[par]) + hit] = NEG_INF;
    }
    lds_barrier();
    for (int idx = tid; idx < NP; idx += NT) {
      const float s = lse2(cpb[idx], cpnb[idx]);
      ctot[idx] = s;
      key[idx] = ((uint64_t)f_order(s) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)idx);
    }
    lds_barrier();
    // the W best by rank counting (keys are distinct: equal scores order by candidate index): every thread scans all
    // keys (broadcast LDS reads, two per instruction) against its own, with no barrier inside
    {
      const ulonglong2* k2 = reinterpret_cast<const ulonglong2*>(key);
      for (int i0 = tid; i0 < NP; i0 += 2 * NT) {
        const int i1 = i0 + NT;
        const uint64_t m0 = key[i0], m1 = i1 < NP ? key[i1] : ~0ull;
        int r0 = 0, r1 = 0;
        // eight 16-byte reads in flight per trip (NP is a multiple of 16): one read per trip leaves the scan waiting
        // on LDS latency
        for (int l = 0; l < NP / 2; l += 8) {
          ulonglong2 kk[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) kk[u] = k2[l + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            r0 += (int)(kk[u].x > m0) + (int)(kk[u].y > m0);
            r1 += (int)(kk[u].x > m1) + (int)(kk[u].y > m1);
          }
        }
        if (r0 < W) sel[r0] = i0;
        if (i1 < NP && r1 < W) sel[r1] = i1;
      }
    }
    lds_barrier();
    // the new beam, rebased on its best entry
    float m = ctot[sel[0]];
    if (!(m > NEG_INF)) m = 0.f;
    off += (double)m;
    const float* xn = p.x + b * p.sb + (long)(t + 1) * p.st;
    for (int s = tid; s < W; s += NT) {
      const int idx = sel[s];
      const float sc = ctot[idx];
      const int o = nxt * W + s;
      int par = -1, tokn = -1;
      if (!(sc > NEG_INF)) {
        pb[o] = NEG_INF; pnb[o] = NEG_INF; tot[o] = NEG_INF; hash[o] = 0; phash[o] = 0; len[o] = 0; last[o] = -1;
        rl[s] = NEG_INF;
        if constexpr (LM) { prev[o] = -1; lt[o] = 0.f; bo2[s] = 0.f; bo1[s] = 0.f; }
      } else {
        int nl;
        if (idx < W) {
          par = idx;
          hash[o] = hc[par]; phash[o] = phc[par]; len[o] = lenc[par]; nl = lastc[par];
          if constexpr (LM) { prev[o] = prev[cur * W + par]; lt[o] = lt[cur * W + par]; }
        } else {
          const int e = idx - W;
          if constexpr (LM) {
            par = e / K;
            tokn = tkc[e - par * K];
            prev[o] = lenc[par] > 0 ? lastc[par] : p.lm.V;
            lt[o] = clt[e];
          } else {
            par = owner[e];
            tokn = tkc[e - start[par]];
          }
          hash[o] = prefix_mix(hc[par], tokn); phash[o] = hc[par]; len[o] = lenc[par] + 1; nl = tokn;
        }
        last[o] = nl;
        pb[o] = cpb[idx] - m; pnb[o] = cpnb[idx] - m; tot[o] = sc - m;
        rl[s] = (more && nl >= 0) ? xn[nl] - lse_n : NEG_INF;
        if constexpr (LM) {
          float b2, b1;
          lm_context(p.lm, prev[o], nl >= 0 ? nl : p.lm.V, b2, b1);
          bo2[s] = b2; bo1[s] = b1;
        }
      }
      parent_of[s] = -1;
      p.bp_parent[row * W + s] = par;
      p.bp_token[row * W + s] = tokn;
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int j = tid + q * NT;
      if (j < K) { tk[nxt * KP + j] = pk[q]; tlp[nxt * KP + j] = pl[q]; }
    }
    lds_barrier();
  }
  const float* totf = tot + (Tb & 1) * W;
  if constexpr (LM) {
    // the </s> term, then the slots in descending final score (equal scores: lower slot first)
    for (int s = tid; s < W; s += NT) {
      const int o = (Tb & 1) * W + s;
      const int nl = last[o];
      const float e = p.lm.eos ? lm_score(p.lm, prev[o], nl >= 0 ? nl : p.lm.V, p.lm.V + 1, bo2[s], bo1[s]) : 0.f;
      const float f = totf[s] > NEG_INF ? (float)(off + (double)totf[s] + (double)(p.lm.alpha * e)) : NEG_INF;
      p.fin[(long)b * W + s] = f;
      key[s] = ((uint64_t)f_order(f) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)s);
    }
    lds_barrier();
    for (int s = tid; s < W; s += NT) {
      const uint64_t mine = key[s];
      int r = 0;
      for (int k = 0; k < W; ++k) r += (int)(key[k] > mine);
      p.perm[(long)b * W + r] = s;
    }
  } else {
    for (int s = tid; s < W; s += NT)
      p.fin[(long)b * W + s] = totf[s] > NEG_INF ? (float)(off + (double)totf[s]) : NEG_INF;
  }
}

// ------------------------------------------------------------------------------------------ backtrace
__global__ __launch_bounds__(64) void beam_backtrace(const int32_t* __restrict__ bp_parent,
                                                     const int32_t* __restrict__ bp_token,
                                                     const int32_t* __restrict__ lens, const float* __restrict__ fin,
                                                     const int32_t* __restrict__ perm,   // null: hypothesis h is slot h
                                                     int B, int T, int W, int nbest, int32_t* __restrict__ tokens,
                                                     int32_t* __restrict__ out_len, float* __restrict__ score) {
  __shared__ int32_t sp[BT_LDS], stok[BT_LDS];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int Tb = clamp_len(lens, b, T);
  const int CH = max(1, min(BT_LDS / W, T));
  const long base = (long)b * T * W;
  bool valid[2];
  int L[2] = {0, 0};
  int slot[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int h = lane + 64 * q;
    slot[q] = (perm && h < W) ? min(max(perm[(long)b * W + h], 0), W - 1) : h;
    valid[q] = h < nbest && h < W && Tb > 0 && bp_parent[base + (long)(Tb - 1) * W + slot[q]] >= 0;
  }
  for (int pass = 0; pass < 2; ++pass) {
    int s[2] = {slot[0], slot[1]};
    int pos[2] = {L[0], L[1]};
    for (int t1 = Tb; t1 > 0; t1 -= CH) {
      const int t0 = max(0, t1 - CH), n = (t1 - t0) * W;
      __syncthreads();
      for (int e = lane; e < n; e += 64) {
        sp[e] = bp_parent[base + (long)t0 * W + e];
        stok[e] = bp_token[base + (long)t0 * W + e];
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (!valid[q]) continue;
        const long orow = ((long)b * nbest + lane + 64 * q) * T;
        for (int t = t1 - 1; t >= t0; --t) {
          const int e = (t - t0) * W + s[q];
          const int tokn = stok[e];
          if (tokn >= 0) {
            if (pass == 0) ++L[q];
            else if (pos[q] > 0) tokens[orow + --pos[q]] = tokn;
          }
          s[q] = sp[e];
          if ((unsigned)s[q] >= (unsigned)W) { s[q] = 0; L[q] = 0; valid[q] = false; break; }   // never follows a bad index
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int h = lane + 64 * q;
    if (h >= nbest) continue;
    const bool first_empty = Tb == 0 && h == 0;
    out_len[(long)b * nbest + h] = valid[q] ? L[q] : 0;
    score[(long)b * nbest + h] =
        valid[q] ? fin[(long)b * W + slot[q]] : (first_empty ? (perm ? fin[(long)b * W + slot[q]] : 0.f) : NEG_INF);
  }
  for (int h = 0; h < nbest; ++h) {
    const int q = h >> 6;
    const int Lq = q == 0 ? L[0] : L[1];
    const bool vq = q == 0 ? valid[0] : valid[1];
    const int Lh = __shfl(vq ? Lq : 0, h & 63, 64);
    for (int i = Lh + lane; i < T; i += 64) tokens[((long)b * nbest + h) * T + i] = -1;
  }
}

// the workspace, as byte offsets: both *_ws_bytes functions and run_beam read this.  KP: stride of the token lists
// (W + 1 without an LM, K with one); the LM search adds the slot permutation
struct BeamWs { size_t row_lse, row_rb, tlp, tk, fin, perm, total; };
BeamWs beam_ws(int B, int T, int W, int KP, bool lm) {
  const size_t bt = (size_t)B * T, bw = (size_t)B * W;
  BeamWs w;
  w.row_lse = 0;
  w.row_rb = w.row_lse + sizeof(float) * bt;
  w.tlp = w.row_rb + sizeof(float) * bt;
  w.tk = w.tlp + sizeof(float) * bt * KP;
  w.fin = w.tk + sizeof(int32_t) * bt * KP;
  w.perm = w.fin + sizeof(float) * bw;
  w.total = w.perm + (lm ? sizeof(int32_t) * bw : 0);
  return w;
}

// what both entry points hand to run_beam (fn names the entry point in messages), and what the LM one adds
struct BeamArgs {
  const char* fn;
  const float* logits; long sb, st; const int32_t* lens;
  int B, T, V, blank, pad, beam, nbest;
  int32_t* bp_parent; int32_t* bp_token; int32_t* tokens; int32_t* out_len; float* score;
  void* ws; void* stream;
};
// the shared arguments in the entry points' own order, each stored under its name
BeamArgs beam_args(const char* fn, const float* logits, long sb, long st, const int32_t* lens, int B, int T, int V,
                   int blank, int pad, int beam, int nbest, int32_t* bp_parent, int32_t* bp_token, int32_t* tokens,
                   int32_t* out_len, float* score, void* ws, void* stream) {
  BeamArgs a;
  a.fn = fn; a.logits = logits; a.sb = sb; a.st = st; a.lens = lens;
  a.B = B; a.T = T; a.V = V; a.blank = blank; a.pad = pad; a.beam = beam; a.nbest = nbest;
  a.bp_parent = bp_parent; a.bp_token = bp_token; a.tokens = tokens; a.out_len = out_len; a.score = score;
  a.ws = ws; a.stream = stream;
  return a;
}
struct BeamLmArgs { const cfm_ngram_lm* lm; int token_beam; float alpha, beta; int eos; };

// the three launches of either search; la null: the plain search
int run_beam(const BeamArgs& a, const BeamLmArgs* la) {
  const cfm_ngram_lm* lm = la ? la->lm : nullptr;
  const int B = a.B, T = a.T, V = a.V, W = a.beam;
  CFM_REQUIRE_FN(a.fn, a.logits && a.bp_parent && a.bp_token && a.tokens && a.out_len && a.score && a.ws, CFM_ERR_ARG,
                 "null pointer");
  CFM_REQUIRE_FN(a.fn, B > 0 && T > 0, CFM_ERR_SHAPE, "bad shape");
  CFM_REQUIRE_FN(a.fn, V >= 2 && V <= 16384, CFM_ERR_UNSUPPORTED, "2 <= V <= 16384");
  CFM_REQUIRE_FN(a.fn, W >= 1 && a.nbest >= 1 && a.nbest <= W, CFM_ERR_ARG, "1 <= nbest <= beam");
  CFM_REQUIRE_FN(a.fn, W <= BEAM_MAX, CFM_ERR_UNSUPPORTED, "beam width must be <= 128");
  CFM_REQUIRE_FN(a.fn, a.blank >= 0 && a.blank < V, CFM_ERR_ARG, "blank out of range");
  CFM_REQUIRE_FN(a.fn, a.pad < V, CFM_ERR_ARG, "pad out of range");
  // K tokens per frame, listed with stride KP.  Without an LM the pair rule needs the W + 1 best; with one every
  // entry is extended by the token_beam best
  const int ntok = V - 1 - ((a.pad >= 0 && a.pad != a.blank) ? 1 : 0);
  const int want = lm ? la->token_beam : W + 1;
  const int K = ntok < want ? ntok : want;
  const int KP = lm ? K : W + 1;
  if (lm) {
    CFM_REQUIRE_FN(a.fn, K >= 1, CFM_ERR_UNSUPPORTED, "no token left to emit");
    CFM_REQUIRE_FN(a.fn, W + W * K <= 1024, CFM_ERR_UNSUPPORTED, "beam + beam * token_beam must be <= 1024");
    CFM_REQUIRE_FN(a.fn, K <= 768, CFM_ERR_UNSUPPORTED, "token_beam must be <= 768");
  }
  hipStream_t s = cfm::as_stream(a.stream);
  const size_t bt = (size_t)B * T;
  const BeamWs w = beam_ws(B, T, W, KP, lm != nullptr);
  char* base = static_cast<char*>(a.ws);
  float* row_lse = reinterpret_cast<float*>(base + w.row_lse);
  float* row_rb = reinterpret_cast<float*>(base + w.row_rb);
  float* tlp = reinterpret_cast<float*>(base + w.tlp);
  int32_t* tk = reinterpret_cast<int32_t*>(base + w.tk);
  float* fin = reinterpret_cast<float*>(base + w.fin);
  int32_t* perm = lm ? reinterpret_cast<int32_t*>(base + w.perm) : nullptr;

  const int wpb = V <= 4096 ? 4 : 1;
  hipLaunchKernelGGL(beam_topk, dim3((unsigned)((bt + wpb - 1) / wpb)), dim3(64 * wpb),
                     (size_t)wpb * V * sizeof(float), s, a.logits, a.sb, a.st, a.lens, B, T, V, a.blank,
                     a.pad < 0 ? -1 : a.pad, K, KP, row_lse, row_rb, tk, tlp);

  BeamP p;
  p.x = a.logits; p.sb = a.sb; p.st = a.st; p.lens = a.lens;
  p.B = B; p.T = T; p.V = V; p.W = W; p.K = K; p.KP = KP;
  p.row_lse = row_lse; p.row_rb = row_rb; p.tk = tk; p.tlp = tlp;
  p.bp_parent = a.bp_parent; p.bp_token = a.bp_token; p.fin = fin; p.perm = perm;
  p.lm = LmP{};
  // the LDS layout of beam_search: the arrays both searches have, then owner (plain) or prev, lt, bo2, bo1, clt (LM)
  size_t sh;
  unsigned block;
  if (lm) {
    p.NE = W * K;
    p.NC = W + p.NE;
    p.NP = (p.NC + 15) & ~15;   // the rank counting reads 16 keys per trip; padding costs candidates^2 work
    p.lm.uni = static_cast<const float2*>(lm->unigrams);
    p.lm.tab = static_cast<const uint4*>(lm->table);
    p.lm.seed = lm->seed; p.lm.mask = lm->mask; p.lm.probe = lm->probe; p.lm.order = lm->order; p.lm.V = V;
    p.lm.alpha = la->alpha; p.lm.beta = la->beta; p.lm.eos = la->eos ? 1 : 0;
    sh = sizeof(int) * (2 * (size_t)W) + sizeof(float) * (4 * (size_t)W + p.NE);
    block = (p.NP <= 128 && K <= 192) ? 64 : 256;   // the next frame's token list is prefetched three per thread
  } else {
    int ne = 0;
    for (int i = 0; i < W; ++i) ne += ext_count(i, W, K);
    p.NE = ne;
    p.NC = W + ne;
    int np = 16;
    while (np < p.NC) np <<= 1;
    p.NP = np;
    sh = sizeof(int) * (size_t)(ne > 0 ? ne : 1);
    block = np <= 128 ? 64 : 256;
  }
  sh += sizeof(uint64_t) * ((size_t)p.NP + 4 * W) + sizeof(float) * (3 * (size_t)p.NP + 7 * W + 2 * KP) +
        sizeof(int) * (2 * (size_t)KP + 7 * W);
  CFM_REQUIRE_FN(a.fn, sh <= 64 * 1024, CFM_ERR_UNSUPPORTED, "beam state exceeds the LDS budget");
  if (lm) hipLaunchKernelGGL(beam_search<true>, dim3(B), dim3(block), sh, s, p);
  else hipLaunchKernelGGL(beam_search<false>, dim3(B), dim3(block), sh, s, p);
  hipLaunchKernelGGL(beam_backtrace, dim3(B), dim3(64), 0, s, a.bp_parent, a.bp_token, a.lens, fin,
                     static_cast<const int32_t*>(perm), B, T, W, a.nbest, a.tokens, a.out_len, a.score);
  return cfm::check_launch(a.fn);
}

}  // namespace

CFM_EXPORT size_t cfm_ctc_beam_ws_bytes(int B, int T, int W) {
  if (B <= 0 || T <= 0 || W <= 0) return 0;
  return beam_ws(B, T, W, W + 1, false).total;
}

CFM_EXPORT int cfm_ctc_beam_decode(const float* logits, long sb, long st, const int32_t* lens, int B, int T, int V,
                                   int blank, int pad, int beam, int nbest, int32_t* bp_parent, int32_t* bp_token,
                                   int32_t* tokens, int32_t* out_len, float* score, void* ws, void* stream) {
  return run_beam(beam_args(__func__, logits, sb, st, lens, B, T, V, blank, pad, beam, nbest, bp_parent, bp_token,
                            tokens, out_len, score, ws, stream),
                  nullptr);
}

CFM_EXPORT size_t cfm_ctc_beam_lm_ws_bytes(int B, int T, int W, int K) {
  if (B <= 0 || T <= 0 || W <= 0 || K <= 0) return 0;
  return beam_ws(B, T, W, K, true).total;
}

CFM_EXPORT int cfm_ctc_beam_decode_lm(const float* logits, long sb, long st, const int32_t* lens, int B, int T, int V,
                                      int blank, int pad, int beam, int nbest, int token_beam, float alpha, float beta,
                                      int eos, const cfm_ngram_lm* lm, int32_t* bp_parent, int32_t* bp_token,
                                      int32_t* tokens, int32_t* out_len, float* score, void* ws, void* stream) {
  CFM_REQUIRE(lm && lm->unigrams && lm->table, CFM_ERR_ARG, "null language-model table");
  CFM_REQUIRE(token_beam >= 1, CFM_ERR_ARG, "token_beam must be >= 1");
  CFM_REQUIRE(lm->V == V, CFM_ERR_ARG, "the language model's V differs from the logits'");
  CFM_REQUIRE(lm->order >= 1 && lm->order <= 3, CFM_ERR_UNSUPPORTED, "n-gram order must be 1..3");
  CFM_REQUIRE(lm->probe >= 1 && lm->probe <= 4, CFM_ERR_UNSUPPORTED, "probe length must be 1..4");
  CFM_REQUIRE((lm->mask & (lm->mask + 1u)) == 0u, CFM_ERR_ARG, "table capacity must be a power of two");
  BeamLmArgs la;
  la.lm = lm; la.token_beam = token_beam; la.alpha = alpha; la.beta = beta; la.eos = eos;
  return run_beam(beam_args(__func__, logits, sb, st, lens, B, T, V, blank, pad, beam, nbest, bp_parent, bp_token,
                            tokens, out_len, score, ws, stream),
                  &la);
}
