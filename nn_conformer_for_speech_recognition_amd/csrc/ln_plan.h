// ln_plan.h — the one host-side rule of the LayerNorm kernels (layernorm.hip): which kernel family serves a call, at
// which width, whether the dropout-scaled copy g2 comes from the same pass, the grid and the workspace.  Pure host
// arithmetic: no kernels, nothing that touches the device.  Every cfm_layernorm_* entry point, the *_ws_bytes and
// cfm_layernorm_pair_ok functions and cfm_layernorm_plan call ln_plan; the launchers act on its cfm_ln_choice -- they
// test no width, dtype or alignment themselves.
#pragma once
#include "cfm_common.h"

namespace {

constexpr int LN_DMAX = 1024;     // the generic kernels hold a row in 16 registers per lane
// rows a forward wave (or lane group) normalises: every row's load is issued before the first reduction, so a wave
// keeps that many 2-KB row reads in flight (one row per wave left the kernel latency-bound at ~50 % of HBM)
constexpr int LN_FWD_ROWS = 2;

// one wave per row, V = D / 64 features per lane: 0 when D is no such width
inline int ln_wave_v(int D) { return D == 128 ? 2 : D == 256 ? 4 : D == 512 ? 8 : D == 1024 ? 16 : 0; }
// a group of G lanes per row, 8 features per lane (D % 8 == 0, D <= 512): G = the power of two >= D / 8, at least 16
inline int ln_group(int D) {
  if (D <= 0 || D % 8 || D > 512) return 0;
  const int n = D / 8;
  return n <= 16 ? 16 : n <= 32 ? 32 : 64;
}
// workgroups of every backward kernel: ~4 rows per wave, at most 1024
inline int ln_bwd_blocks(long M) {
  const long b = (M + 15) / 16;
  return (int)(b < 1024 ? (b < 1 ? 1 : b) : 1024);
}
inline int ln_mod16(const void* p) { return (int)((uintptr_t)p & 15); }
inline bool ln_dt_ok(int dt) { return dt == CFM_F32 || dt == CFM_BF16; }

// The rule.  `who` prefixes the error text (the entry point that asked).
//   errors   y / z / dy / dz (and fwd_res's delta, the MX forward's x) outside {f32, bf16}: CFM_ERR_DTYPE -- the
//            generic kernels' st_dyn / ld_dyn would take such a code for fp32 just as the wave kernels did.
//            D outside (0, 1024] or M < 0: CFM_ERR_SHAPE.
//   WAVE     D in {128, 256, 512, 1024}: V = D / 64.     GROUP   other D % 8 == 0, D <= 512: G = 16 / 32 / 64.
//            Both need an f32 / bf16 x and every pointer the kernel moves 16-byte vectors through 16-byte aligned;
//            the backward also an fp32 dx and dres, fwd_res a bf16 delta.  Anything else: GENERIC.
//   MX       (y's e4m3 copy) WAVE with V >= 4 and a bf16 y only: D in {256, 512, 1024} and an 8-byte aligned y8, else
//            CFM_ERR_SHAPE (cfm_layernorm_fwd_mx_ex reports y8 as CFM_ERR_ALIGN); no WAVE kernel: CFM_ERR_ALIGN.
//   g2       fused on WAVE V = 8 and on GROUP, when g2 is 16-byte aligned; else the kernel runs without it and
//            cfm_scale_dropout makes g2 from dx.  A backward at D 128 / 256 (V = 2 / 4 have no g2 epilogue) with an
//            aligned g2 runs the GROUP kernel of that width (G = 16 / 32), which has.
//   pair     V = 8 / 4 (D 512 / 256) or GROUP, never GENERIC: no such kernel is CFM_ERR_SHAPE, a misaligned pointer
//            (g2 included) CFM_ERR_ALIGN.  g2 fused except at V = 4.
//   blocks   forward: ceil(M / rows per workgroup), rows = 4 waves * rows per wave (WAVE 1, GROUP 64 / G, GENERIC 1)
//            * LN_FWD_ROWS (GENERIC: 1); backward: ln_bwd_blocks(M).
//   ws       bwd: blocks rows of [dgamma | dbeta] partials (2 D floats) + one spare row; bwd_pair: 2 * blocks rows.
inline int ln_plan(const cfm_ln_query& q, cfm_ln_choice& c, const char* who) {
#define LN_PLAN_REQUIRE(cond, code, msg) \
  do { if (!(cond)) return cfm::fail((code), std::string(who) + ": " + (msg)); } while (0)
  const int op = q.op, D = q.D;
  const bool fwd = op == CFM_LN_FWD || op == CFM_LN_FWD_RES || op == CFM_LN_FWD_PAIR;
  const bool pair = op == CFM_LN_FWD_PAIR || op == CFM_LN_BWD_PAIR;
  LN_PLAN_REQUIRE(fwd || op == CFM_LN_BWD || op == CFM_LN_BWD_PAIR, CFM_ERR_ARG, "unknown op");
  c = cfm_ln_choice{};
  LN_PLAN_REQUIRE(ln_dt_ok(fwd ? q.dt_y : q.dt_dy), CFM_ERR_DTYPE, fwd ? "y / z: f32 or bf16" : "dy / dz: f32 or bf16");
  LN_PLAN_REQUIRE(op != CFM_LN_FWD_RES || ln_dt_ok(q.dt_delta), CFM_ERR_DTYPE, "delta: f32 or bf16");
  LN_PLAN_REQUIRE(!(op == CFM_LN_FWD && q.want_mx) || ln_dt_ok(q.dt_x), CFM_ERR_DTYPE, "x: f32 or bf16");
  LN_PLAN_REQUIRE(q.M >= 0 && (pair || (D > 0 && D <= LN_DMAX)), CFM_ERR_SHAPE, "D must be in (0, 1024], M >= 0");
  const int V = ln_wave_v(D), G = V ? 0 : ln_group(D);
  if (pair) {
    LN_PLAN_REQUIRE(V == 8 || V == 4 || G, CFM_ERR_SHAPE,
                    "no fused pair kernel for this width / dtype (cfm_layernorm_pair_ok)");
    const int a = fwd ? q.x_mod16 | q.y_mod16 | q.z_mod16 | q.gamma_mod16 | q.beta_mod16 | q.gamma2_mod16 | q.beta2_mod16
                      : q.dy_mod16 | q.dres_mod16 | q.x_mod16 | q.dx_mod16 | q.gamma_mod16 | q.beta_mod16 |
                            q.gamma2_mod16 | (q.want_g2 ? q.g2_mod16 : 0);
    LN_PLAN_REQUIRE(a % 16 == 0, CFM_ERR_ALIGN,
                    fwd ? "16-B aligned x / y / z / gamma / beta" : "16-B aligned dz / dres / x / dx / gamma / beta / g2");
    c.family = V ? CFM_LN_WAVE : CFM_LN_GROUP;
    c.width = V ? V : G;
    c.g2_fused = !fwd && q.want_g2 && V != 4;
  } else if (fwd) {
    const bool res = op == CFM_LN_FWD_RES;
    LN_PLAN_REQUIRE(!q.want_mx || (q.dt_y == CFM_BF16 && V >= 4), CFM_ERR_SHAPE,
                    "MX copy: bf16 y, D in {256, 512, 1024}");
    LN_PLAN_REQUIRE(!q.want_mx || q.y8_mod16 % 8 == 0, res ? CFM_ERR_SHAPE : CFM_ERR_ALIGN, "MX copy: 8-B aligned y8");
    const int a = q.x_mod16 | q.y_mod16 | q.gamma_mod16 | q.beta_mod16 | (res ? q.delta_mod16 | q.xout_mod16 : 0);
    // x + delta in the fast kernels: the fp32 stream plus the module's bf16 output
    const bool fast = a % 16 == 0 && (res ? q.dt_x == CFM_F32 && q.dt_delta == CFM_BF16 : ln_dt_ok(q.dt_x));
    c.family = !fast ? CFM_LN_GENERIC : V ? CFM_LN_WAVE : G ? CFM_LN_GROUP : CFM_LN_GENERIC;
    c.width = c.family == CFM_LN_WAVE ? V : c.family == CFM_LN_GROUP ? G : 0;
    LN_PLAN_REQUIRE(!q.want_mx || c.family == CFM_LN_WAVE || q.M == 0, CFM_ERR_ALIGN,
                    "MX copy: 16-B aligned x / delta / xout / y / gamma / beta");
  } else {
    const int a = q.dy_mod16 | q.x_mod16 | q.dres_mod16 | q.dx_mod16 | q.gamma_mod16;
    const bool fast = a % 16 == 0 && ln_dt_ok(q.dt_x) && q.dt_dx == CFM_F32 && q.dt_dres == CFM_F32;
    const bool g2 = q.want_g2 && q.g2_mod16 % 16 == 0;      // a g2 the kernels could store
    const int Gb = ln_group(D);                             // (D 128 / 256 / 512 are lane-group widths too)
    if (fast && V && (V == 8 || !(g2 && Gb))) {
      c.family = CFM_LN_WAVE;
      c.width = V;
      c.g2_fused = g2 && V == 8;
    } else if (fast && Gb) {
      c.family = CFM_LN_GROUP;
      c.width = Gb;
      c.g2_fused = g2;
    } else {
      c.family = CFM_LN_GENERIC;
    }
  }
  if (fwd) {
    const long rows = c.family == CFM_LN_WAVE    ? 4L * LN_FWD_ROWS
                      : c.family == CFM_LN_GROUP ? 4L * (64 / c.width) * LN_FWD_ROWS
                                                 : 4L;
    c.blocks = (int)((q.M + rows - 1) / rows);
  } else {
    c.blocks = ln_bwd_blocks(q.M);
    c.ws_bytes = pair ? (size_t)c.blocks * 4 * D * sizeof(float) : ((size_t)c.blocks + 1) * 2 * D * sizeof(float);
  }
#undef LN_PLAN_REQUIRE
  return CFM_OK;
}

}  // namespace
