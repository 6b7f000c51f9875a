// gemm_wgrad.hip -- the grouped weight gradients: table fill, the XCD-aware plan (a pure host function), the planned
// and plain launches of the GROUP form of gemm_pipe_kernel (kWgradGroup) and the split tasks' slab reduce.
#include "gemm_variants.h"

#include <algorithm>
#include <vector>

namespace {

// sum the K-slice slabs of every split task of a planned grouped launch, in slice order (deterministic):
// dW (N x K, row-major) = sum_s slab[s], db (N) = sum_s acs_slab[s]; block b of task t: 1024 elements of dW and
// (b < N / 256) 256 elements of db; task of a block = the last one whose red0 <= b (unsplit tasks own no blocks)
__global__ __launch_bounds__(256) void wgrad_split_reduce_kernel(const WgTask* __restrict__ tab, int ntasks) {
  const long b = blockIdx.x;
  int lo = 0, hi = ntasks - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].red0 <= b) lo = mid; else hi = mid - 1;
  }
  const WgTask& t = tab[lo];
  const int S = t.p.split_k, N = t.p.M, K = t.p.N;
  const long lb = b - t.red0;
  const long per = (long)N * K;
  const long w = (lb * 256 + threadIdx.x) * 4;
  if (w < per) {
    const float* src = t.p.slab + w;
    float4 s = *reinterpret_cast<const float4*>(src);
    for (int k = 1; k < S; ++k) {
      const float4 a = *reinterpret_cast<const float4*>(src + k * per);
      s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
    }
    *reinterpret_cast<float4*>(t.dw + w) = s;
  }
  const long n = lb * 256 + threadIdx.x;
  if (t.db && n < N) {
    float s = t.p.acs_slab[n];
    for (int k = 1; k < S; ++k) s += t.p.acs_slab[k * (long)N + n];
    t.db[n] = s;
  }
}

}  // namespace

CFM_EXPORT size_t cfm_wgrad_group_task_bytes(void) { return sizeof(WgTask); }
// grouped weight-gradient launch: kWgradGroup (gemm_variants.h: 256 x 256 output tiles, BK 32, 4-deep ring)
CFM_EXPORT long cfm_wgrad_group_tiles(int N, int K) { return (long)cdiv(N, 256) * cdiv(K, WG_BN); }

// fill task i of a HOST table: dW (N x K, fp32) = dYᵀ X over M tokens, dY (M x N) / X (M x K) bf16
// row-major; db (N, fp32, may be NULL) = sum_rows dY; tile0 = first workgroup id of the task
CFM_EXPORT int cfm_wgrad_group_fill(void* host_tab, int i, const void* dy, const void* x, float* dw, float* db, int M,
                                    int N, int K, long tile0) {
  CFM_REQUIRE(host_tab && dy && x && dw && i >= 0, CFM_ERR_ARG, "null pointer");
  CFM_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && K % 8 == 0, CFM_ERR_SHAPE, "N, K multiples of 8");
  CFM_REQUIRE((long)M * N * 2 < (1L << 31) && (long)M * K * 2 < (1L << 31), CFM_ERR_SHAPE, "operands < 2 GiB");
  CFM_REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)dw % 16 == 0, CFM_ERR_ALIGN,
              "16-B aligned operands");
  WgTask t{};
  t.p = plain_params(N, K, M, dw, K, CFM_F32);
  t.p.k_per_split = split_k_for(t.p, BK16);
  t.p.vec_c = vec_epilogue_ok(t.p);
  t.p.acs_slab = db;   // single K slice: the column sums go straight to db
  t.oa = PipeOp{(const bf16*)dy, N, 0, N, (unsigned)((long)M * N * 2)};
  t.ob = PipeOp{(const bf16*)x, K, 0, K, (unsigned)((long)M * K * 2)};
  t.tile0 = tile0;
  t.tiles_n = cdiv(K, WG_BN);
  reinterpret_cast<WgTask*>(host_tab)[i] = t;
  return CFM_OK;
}

// the same for a planned launch: task i of the table as cfm_wgrad_group_fill, and when split > 1 (the plan's
// task_split[i]) its K range cut into `split` slices of whole 32-token steps whose fp32 partials go to the workspace
// ws (cfm_wgrad_group_ws_floats(N, K, split) floats: split dW slabs, then split db rows), summed into dw / db by the
// reduce pass; red0 = the task's first reduce block (running sum of cfm_wgrad_group_red_blocks over earlier tasks)
CFM_EXPORT long cfm_wgrad_group_ws_floats(int N, int K, int split) {
  return split > 1 ? (long)split * ((long)N * K + N) : 0;
}
CFM_EXPORT long cfm_wgrad_group_red_blocks(int N, int K, int split) {
  if (split <= 1) return 0;
  const long a = cdiv((long)N * K, 1024), b = cdiv(N, 256);
  return a > b ? a : b;
}
CFM_EXPORT int cfm_wgrad_group_fill_split(void* host_tab, int i, const void* dy, const void* x, float* dw, float* db,
                                          int M, int N, int K, int split, float* ws, long red0) {
  const int rc = cfm_wgrad_group_fill(host_tab, i, dy, x, dw, db, M, N, K, 0);
  if (rc != CFM_OK) return rc;
  CFM_REQUIRE(split >= 1 && split <= 15, CFM_ERR_ARG, "split in 1..15");
  WgTask& t = reinterpret_cast<WgTask*>(host_tab)[i];
  t.red0 = red0;
  t.dw = dw;
  t.db = db;
  if (split > 1) {
    CFM_REQUIRE(ws && (uintptr_t)ws % 16 == 0, CFM_ERR_ALIGN, "16-B aligned workspace");
    CFM_REQUIRE((long)split * N * K < (1L << 31), CFM_ERR_SHAPE, "split slabs too large");
    t.p.split_k = split;
    t.p.k_per_split = ((M + split - 1) / split + 31) / 32 * 32;
    t.p.slab = ws;
    t.p.acs_slab = db ? ws + (long)split * N * K : nullptr;
    t.red_blocks = (int)cfm_wgrad_group_red_blocks(N, K, split);
  }
  return CFM_OK;
}

// Plan a grouped launch of ntasks GEMMs of task_tiles[i] output tiles each (cfm_wgrad_group_tiles) on nxcd XCDs
// of `cus` CUs (one workgroup per CU: the kernel holds a 128-KiB ring):
//  * tasks (cut into pieces of at most `cus` tiles) are packed first-fit-decreasing into bins of `cus` tiles;
//  * each XCD x gets R = (full bins) / nxcd full bins -- workgroup ids x, x + nxcd, ... in bin order, so a bin's
//    tiles start together on one XCD and every dY / X slice a bin reads is streamed into that XCD's L2 once;
//  * the tiles of the remaining bins (the ragged last round) are split over S = min(8, nxcd * cus / tail) K slices
//    (task_split[i] = S for their tasks, 1 otherwise) and dealt to the XCDs slice by slice, so the last round
//    fills the chip instead of running a few tiles alone; with S < 2 (or a task cut across main and tail bins)
//    they run unsplit as extra bins.
// Writes grid words to sched (capacity cap; WG_SCHED_EMPTY pads the shorter XCD lists) and returns the grid size,
// or a negative error code.
CFM_EXPORT long cfm_wgrad_group_plan(const long* task_tiles, int ntasks, int nxcd, int cus, unsigned* sched,
                                     long cap, int* task_split) {
  if (!task_tiles || !sched || !task_split || ntasks <= 0 || ntasks > 4095 || nxcd <= 0 || cus <= 0)
    return cfm::fail(CFM_ERR_ARG, "cfm_wgrad_group_plan: bad arguments");
  struct Piece { int task, off, n; };
  std::vector<Piece> pieces;
  for (int i = 0; i < ntasks; ++i) {
    if (task_tiles[i] <= 0 || task_tiles[i] > 65535)
      return cfm::fail(CFM_ERR_SHAPE, "cfm_wgrad_group_plan: tiles per task in 1..65535");
    for (int o = 0; o < task_tiles[i]; o += cus) pieces.push_back({i, o, (int)std::min<long>(cus, task_tiles[i] - o)});
    task_split[i] = 1;
  }
  std::stable_sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.n > b.n; });
  std::vector<std::vector<Piece>> bins;
  std::vector<int> fill;
  for (const Piece& pc : pieces) {
    size_t k = 0;
    while (k < bins.size() && fill[k] + pc.n > cus) ++k;
    if (k == bins.size()) { bins.emplace_back(); fill.push_back(0); }
    bins[k].push_back(pc);
    fill[k] += pc.n;
  }
  std::vector<int> full, rest;
  for (size_t k = 0; k < bins.size(); ++k) (fill[k] == cus ? full : rest).push_back((int)k);
  const int R = (int)full.size() / nxcd;
  for (size_t k = (size_t)R * nxcd; k < full.size(); ++k) rest.push_back(full[k]);
  full.resize((size_t)R * nxcd);
  std::vector<std::vector<unsigned>> lists(nxcd);
  auto emit_bin = [&](std::vector<unsigned>& l, int k, int ks) {
    for (const Piece& pc : bins[k])
      for (int t = 0; t < pc.n; ++t) l.push_back(wg_sched_word(pc.task, ks, pc.off + t));
  };
  for (int x = 0; x < nxcd; ++x)
    for (int r = 0; r < R; ++r) emit_bin(lists[x], full[(size_t)x * R + r], 0);
  long tail = 0;
  std::vector<char> in_main(ntasks, 0), in_tail(ntasks, 0);
  for (int k : full) for (const Piece& pc : bins[k]) in_main[pc.task] = 1;
  for (int k : rest) for (const Piece& pc : bins[k]) { in_tail[pc.task] = 1; tail += pc.n; }
  bool cut = false;
  for (int i = 0; i < ntasks; ++i) cut |= in_main[i] && in_tail[i];
  const int S = tail > 0 && !cut ? (int)std::min<long>(8, (long)nxcd * cus / tail) : 1;
  if (S >= 2) {
    std::vector<unsigned> parts;   // slice-major: XCD x gets a contiguous run (one slice per XCD when S == nxcd)
    for (int ks = 0; ks < S; ++ks)
      for (int k : rest) emit_bin(parts, k, ks);
    const long np = (long)parts.size();
    for (long q = 0; q < np; ++q) lists[(int)(q * nxcd / np)].push_back(parts[q]);
    for (int i = 0; i < ntasks; ++i) if (in_tail[i]) task_split[i] = S;
  } else {
    for (size_t j = 0; j < rest.size(); ++j) emit_bin(lists[j % nxcd], rest[j], 0);
  }
  size_t len = 0;
  for (auto& l : lists) len = std::max(len, l.size());
  const long grid = (long)len * nxcd;
  if (grid > cap) return cfm::fail(CFM_ERR_ARG, "cfm_wgrad_group_plan: schedule capacity too small");
  for (size_t j = 0; j < len; ++j)
    for (int x = 0; x < nxcd; ++x) sched[j * nxcd + x] = j < lists[x].size() ? lists[x][j] : WG_SCHED_EMPTY;
  return grid;
}

// planned launch: dev_sched (grid words from cfm_wgrad_group_plan, on the device) over the table of
// cfm_wgrad_group_fill_split tasks, then the reduce pass over the split tasks' slabs (red_blocks = the sum of the
// tasks' cfm_wgrad_group_red_blocks; 0: no split task)
CFM_EXPORT int cfm_wgrad_group_sched(const void* dev_tab, int ntasks, const unsigned* dev_sched, long grid,
                                     long red_blocks, unsigned long long* probe, void* stream) {
  CFM_REQUIRE(dev_tab && dev_sched && ntasks > 0 && grid > 0 && grid < (1L << 31) && red_blocks >= 0 &&
              red_blocks < (1L << 31), CFM_ERR_ARG, "bad plan");
  GemmP gp{};
  gp.probe = probe;
  GatherA ga{};
  ga.group_tab = dev_tab;
  ga.group_n = ntasks;
  ga.group_sched = dev_sched;
  hipStream_t s = cfm::as_stream(stream);
  hipLaunchKernelGGL((kWgradGroup<>),
                     dim3((unsigned)grid), dim3(512), 0, s, gp, PipeOp{}, PipeOp{}, ga);
  if (red_blocks > 0)
    hipLaunchKernelGGL(wgrad_split_reduce_kernel, dim3((unsigned)red_blocks), dim3(256), 0, s,
                       reinterpret_cast<const WgTask*>(dev_tab), ntasks);
  return cfm::check_launch("cfm_wgrad_group_sched");
}

CFM_EXPORT int cfm_wgrad_group_probed(const void* dev_tab, int ntasks, long total_tiles, unsigned long long* probe,
                                      void* stream) {
  CFM_REQUIRE(dev_tab && ntasks > 0 && total_tiles > 0 && total_tiles < (1L << 31), CFM_ERR_ARG, "bad table");
  GemmP gp{};
  gp.probe = probe;
  GatherA ga{};
  ga.group_tab = dev_tab;
  ga.group_n = ntasks;
  hipLaunchKernelGGL((kWgradGroup<>),
                     dim3((unsigned)total_tiles), dim3(512), 0, cfm::as_stream(stream), gp, PipeOp{}, PipeOp{}, ga);
  return cfm::check_launch("cfm_wgrad_group");
}

CFM_EXPORT int cfm_wgrad_group(const void* dev_tab, int ntasks, long total_tiles, void* stream) {
  return cfm_wgrad_group_probed(dev_tab, ntasks, total_tiles, nullptr, stream);
}

