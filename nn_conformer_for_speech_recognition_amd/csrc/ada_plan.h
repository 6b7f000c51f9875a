// ada_plan.h — the one host-side rule of the Adafactor step (optim.hip): what every parameter of a group adds to each
// launch and where its share begins: cfm_adafactor_plan, pure host arithmetic.  The kernels take the constants below.
#pragma once
#include "cfm_common.h"

namespace {

constexpr int CHUNK = 4096;      // elements per block in the elementwise passes
constexpr int RB = 32;           // rows per column-partial task (wide factored tensors)
constexpr int KMAX = 40;         // 64-column groups a lane keeps in registers: wide means 64 <= C <= 2560
constexpr int ROWS_PER_TASK = 256;   // rows of a narrow factored tensor per wave (ada_rows; lane = 4 rows)

__host__ __device__ __forceinline__ bool is_wide(int C) { return C >= 64 && C <= 64 * KMAX; }

// the phases whose work is spread over the parameters (find_param searches the AdaP offset of one)
enum AdaPhase { ADA_ROWS, ADA_COLS, ADA_BLOCKS, ADA_ROWMEAN, ADA_COLPART };

}  // namespace

// The rule (DESIGN.md 8q tabulates what each total counts).  before[i] (may be null) is every total in front of
// parameter i, so the owner of item k of a phase is the LAST parameter whose offset is <= k: one with no items of that
// phase shares its offset with its successor and is never found.  (Exported from here: one .hip includes this file.)
CFM_EXPORT int cfm_adafactor_plan(const cfm_adafactor_param* ps, int n, cfm_adafactor_totals* before,
                                  cfm_adafactor_totals* totals) {
  CFM_REQUIRE(ps && totals && n > 0, CFM_ERR_ARG, "bad args");
  cfm_adafactor_totals& tot = *totals = cfm_adafactor_totals{};
  for (int i = 0; i < n; ++i) {
    const cfm_adafactor_param& q = ps[i];
    CFM_REQUIRE(q.numel < (1L << 31), CFM_ERR_SHAPE, "tensor too large (2^31 elements)");
    if (before) before[i] = tot;
    tot.blocks += (q.numel + CHUNK - 1) / CHUNK;
    if (!q.factored) continue;
    const long nb = q.nb, nrb = (q.R + RB - 1) / RB;
    tot.cols += nb * q.C;
    tot.rowmean_floats += nb;
    tot.rowmean_tasks += q.R >= 64 ? nb : (nb + 63) / 64;
    const long cp = is_wide(q.C) ? nb * nrb : 0;      // wide C: column-partial tasks; any other C: row tasks
    tot.colpart_tasks += cp;
    tot.part_floats += cp * q.C;
    tot.row_tasks += is_wide(q.C) ? 0 : (nb * q.R + ROWS_PER_TASK - 1) / ROWS_PER_TASK;
  }
  return CFM_OK;
}
