// attn_plan.h — the one host-side rule of the attention kernels (attention.hip, attention_rel.hip,
// attention_simt.hip): which kernel family runs, how the whole-head kernels are split, where dQ comes from, and the
// byte layout of the backward workspace.  Pure host arithmetic: no kernels, nothing that touches the device.
// cfm_attn_fwd, cfm_attn_bwd_ws_bytes, the backward and cfm_attn_plan all call attn_plan; the launchers of the three
// translation units take its cfm_attn_choice and act on it -- they read no mode global and recompute no offset.
#pragma once
#include "cfm_common.h"

namespace cfm {
extern int g_attn_mode;   // cfm_attn_set_mode's bits (attention.hip); read by the exported entry points only

int attn_simt_fwd_launch(const void* qkv, void* o, float* lse, const int32_t* len, const void* pos, const float* pu,
                         const float* pv, int B, int T, int H, int dk, int dtype, float drop_p, uint64_t seed,
                         hipStream_t s);
// ws: the plan's single dS section (B*H*T*T f32)
int attn_simt_bwd_launch(const void* qkv, const void* o, const void* dout, const float* lse, const int32_t* len,
                         const void* pos, const float* pu, const float* pv, void* dqkv, float* dpos, float* dpu,
                         float* dpv, int B, int T, int H, int dk, int dtype, float drop_p, uint64_t seed, float* ws,
                         hipStream_t s);
int attn_rel_fwd_launch(const cfm_attn_choice& c, const void* qkv, void* o, float* lse, const int32_t* len,
                        const void* pos, const float* pu, const float* pv, int B, int T, int H, int dk, float drop_p,
                        uint64_t seed, hipStream_t s);
// D (rowsum dO*O per head) must already be in the plan's D section of ws
int attn_rel_bwd_launch(const cfm_attn_choice& c, const void* qkv, const void* dout, const float* lse,
                        const int32_t* len, const void* pos, const float* pu, const float* pv, void* dqkv, void* dpos,
                        int dpos_dt, float* dpu, float* dpv, int B, int T, int H, int dk, float drop_p, uint64_t seed,
                        float* ws, hipStream_t s);
}  // namespace cfm

namespace {

constexpr int DKP = 64;           // padded head dim
constexpr int KS = DKP + 8;       // LDS row stride (elements): 144-B rows, conflict-free ds_read_b128
constexpr int TILE = 64;          // keys (fwd/dQ) or queries (dK/dV) per LDS tile
constexpr int HEAD_TMAX = 384;    // whole-head kernels: 12 waves of 32 queries; K+V images 2 * 384 * 144 B = 108 KiB
constexpr int DQH_KS = 96;        // dQ-from-dS whole-head kernel: K image row stride (192-B rows)

// section `i` of the workspace behind the ones placed so far, on a 256-byte boundary
inline void attn_ws_section(cfm_attn_choice& c, int i, size_t bytes) {
  c.ws_off[i] = (c.ws_total + 255) & ~(size_t)255;
  c.ws_size[i] = bytes;
  c.ws_total = c.ws_off[i] + bytes;
}
template <typename T>
inline T* attn_ws_ptr(const cfm_attn_choice& c, int i, float* ws) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + c.ws_off[i]);
}

// The rule.  `who` prefixes the error text (the entry point that asked).
//   path     bf16 with dk <= 64 runs on MFMA: rel-pos -> REL (CFM_ATTN_MODE_REL_SIMT: SIMT), else whole-head for
//            T <= HEAD_TMAX (CFM_ATTN_MODE_TILED: tiled), else tiled.  Everything else (fp32, wide heads): SIMT.
//   vec/vec4 16-B / 8-B loads of qkv and dout rows legal (the forward has no dout: its query repeats qkv's alignment);
//            rel: pvec for pos, and rel_vec = vec && pvec && dk == 64 (CFM_ATTN_MODE_REL_ZERO_FILL: off) picks the
//            branch-free prefetch kernels.  The rel path has no 8-B loads and no timing bits: vec4 and dbg stay 0.
//   qs       workgroups per (b, h) of the whole-head kernels: enough to give every CU one (B*H*qs <= cus), at most 4
//            and at most one per 32-row block (CFM_ATTN_MODE_REL_ZERO_FILL: always one); waves = blocks per workgroup.
//   dq       from the stored dS: rel unless CFM_ATTN_MODE_REL_DQ_RECOMPUTE; whole-head unless
//            CFM_ATTN_MODE_DQ_RECOMPUTE or an offered workspace too small to hold dS^T behind D.
//   dpos     rel: the XCD kernel when rel_vec (CFM_ATTN_MODE_REL_DPOS_R4: the round-4 one), else round-4 non-vec.
//   ws       non-rel MFMA: [D (B*H*T f32)] [dS^T (B*H*Tq*Tq bf16, Tq = ceil(T/32)*32; stored-dS only)]
//            rel: [D] [du/dv partials (B * 4*ceil(T/128) * 2*H*dk f32)] [dS (B*H*T*ldS bf16, ldS = ceil(T/8)*8)]
//                 [per-utterance dpos partials (B*(2T-1)*H*dk f32)]
//            SIMT: [dS (B*H*T*T f32)]
//            q.ws_bytes >= 0 below the total of the chosen layout is CFM_ERR_ARG.
inline int attn_plan(const cfm_attn_query& q, cfm_attn_choice& c, const char* who) {
#define ATTN_PLAN_REQUIRE(cond, code, msg) \
  do { if (!(cond)) return cfm::fail((code), std::string(who) + ": " + (msg)); } while (0)
  const int B = q.B, T = q.T, H = q.H, dk = q.dk, mode = q.mode;
  ATTN_PLAN_REQUIRE(B > 0 && T > 0 && H > 0 && dk > 0 && dk <= 1024, CFM_ERR_SHAPE, "bad shape");
  ATTN_PLAN_REQUIRE(q.dtype == CFM_BF16 || q.dtype == CFM_F32, CFM_ERR_DTYPE, "dtype");
  ATTN_PLAN_REQUIRE(q.rel || q.dtype == CFM_F32 || dk <= DKP, CFM_ERR_UNSUPPORTED, "bf16 head dim must be <= 64");
  ATTN_PLAN_REQUIRE((double)B * H * T * (T + 1) < 8589934592.0, CFM_ERR_SHAPE, "attention dropout index space (2^33)");
  ATTN_PLAN_REQUIRE(q.cus > 0, CFM_ERR_ARG, "cus must be positive");
  c = cfm_attn_choice{};
  const size_t bht = (size_t)B * H * T;
  if (q.dtype != CFM_BF16 || dk > DKP || (q.rel && (mode & CFM_ATTN_MODE_REL_SIMT))) {
    c.path = CFM_ATTN_PATH_SIMT;
    attn_ws_section(c, CFM_ATTN_WS_DS, bht * T * sizeof(float));
  } else {
    const int D3 = 3 * H * dk, a = q.qkv_mod16 | q.dout_mod16;
    c.vec = a % 16 == 0 && dk % 8 == 0 && D3 % 8 == 0;
    c.qs = 1;
    attn_ws_section(c, CFM_ATTN_WS_D, bht * sizeof(float));
    if (q.rel) {
      c.path = CFM_ATTN_PATH_REL;
      c.pvec = q.pos_mod16 % 16 == 0 && dk % 8 == 0;
      c.rel_vec = c.vec && c.pvec && dk == 64 && !(mode & CFM_ATTN_MODE_REL_ZERO_FILL);
      c.dq_stored = !(mode & CFM_ATTN_MODE_REL_DQ_RECOMPUTE);
      c.dpos = !c.rel_vec ? CFM_ATTN_DPOS_R4 : (mode & CFM_ATTN_MODE_REL_DPOS_R4) ? CFM_ATTN_DPOS_R4_VEC : CFM_ATTN_DPOS_XCD;
      attn_ws_section(c, CFM_ATTN_WS_PART, (size_t)B * 4 * cdiv(T, 128) * 2 * H * dk * sizeof(float));
      attn_ws_section(c, CFM_ATTN_WS_DS, bht * ((T + 7) & ~7) * sizeof(bf16));
      attn_ws_section(c, CFM_ATTN_WS_DPOS, (size_t)B * (2 * T - 1) * H * dk * sizeof(float));
    } else {
      c.vec4 = a % 8 == 0 && dk % 4 == 0 && D3 % 4 == 0;
      c.dbg = mode & (CFM_ATTN_MODE_STAGING_ONLY | CFM_ATTN_MODE_SKIP_STORES);
      c.path = T <= HEAD_TMAX && !(mode & CFM_ATTN_MODE_TILED) ? CFM_ATTN_PATH_HEAD : CFM_ATTN_PATH_TILED;
    }
    if (c.path == CFM_ATTN_PATH_HEAD) {
      const int nb = cdiv(T, 32);
      if (!(mode & CFM_ATTN_MODE_REL_ZERO_FILL))
        while (c.qs < 4 && c.qs < nb && (long)B * H * (c.qs + 1) <= q.cus) ++c.qs;
      c.waves = cdiv(nb, c.qs);
      // LDS sized for the full padded length (lengths are device data; len <= T)
      const size_t tk = (size_t)cdiv(T, TILE) * TILE, rows = (size_t)nb * 32;   // K rows: whole 64-key tiles
      const size_t stage = (size_t)c.waves * 32 * 65 * sizeof(float);           // the waves' f32 output stages
      c.lds_head = std::max(2 * tk * KS * sizeof(bf16), stage);
      c.lds_dkdv = 2 * rows * KS * sizeof(bf16) + 2 * rows * sizeof(float) + (size_t)c.waves * nb * 64 * sizeof(unsigned short);
      c.lds_dqs = std::max(tk * DQH_KS * 2 + (size_t)c.waves * TILE * 32 * 2, stage);
      const size_t dsT = (size_t)B * H * rows * rows * sizeof(bf16);
      const size_t full = ((c.ws_total + 255) & ~(size_t)255) + dsT;
      c.dq_stored = !(mode & CFM_ATTN_MODE_DQ_RECOMPUTE) && (q.ws_bytes < 0 || (size_t)q.ws_bytes >= full);
      if (c.dq_stored) attn_ws_section(c, CFM_ATTN_WS_DS, dsT);
    }
  }
  ATTN_PLAN_REQUIRE(q.ws_bytes < 0 || (size_t)q.ws_bytes >= c.ws_total, CFM_ERR_ARG,
                    "workspace of " + std::to_string(q.ws_bytes) + " bytes, " + std::to_string(c.ws_total) + " needed");
#undef ATTN_PLAN_REQUIRE
  return CFM_OK;
}

}  // namespace
