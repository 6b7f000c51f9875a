/* cfm.h — C ABI of the MI355X-native Conformer encoder hot path (libcfm.so).
 *
 * Plain C: raw device pointers, sizes and a hipStream_t passed as void*.  No torch types.
 * Every entry point is stream-ordered (no host synchronisation), allocates no device memory
 * (callers pass workspaces), keeps no pointer after return, and returns 0 on success or a
 * negative CFM_ERR_* code; cfm_get_last_error() returns the thread's last message.
 *
 * The reference (icadriani/nn_conformer_for_speech_recognition) has no FFI: its hot path is a
 * composition of torch.nn modules.  Each entry point below names the reference module/op it
 * replaces (file:line under /root/reference, or torchaudio semantics restated in
 * oracle/conformer.py); INTEGRATION.md shows the ctypes binding the host side uses.
 *
 * Layouts: activations are token-major (row = b*T + t, feature contiguous), matching
 * torchaudio's (B, T, D) interface after its internal transpose.  dtype codes: CFM_F32 / CFM_BF16.
 */
#ifndef CFM_H
#define CFM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFM_F32 0
#define CFM_BF16 1
#define CFM_FP8 2   /* OCP e4m3fn (gfx950), GEMM operands only (cfm_gemm, cfm_quant_fp8) */

#define CFM_OK 0
#define CFM_ERR_ARG (-1)
#define CFM_ERR_SHAPE (-2)
#define CFM_ERR_DTYPE (-3)
#define CFM_ERR_ALIGN (-4)
#define CFM_ERR_UNSUPPORTED (-5)
#define CFM_ERR_LAUNCH (-6)

#define CFM_ACT_NONE 0
#define CFM_ACT_SILU 1

int cfm_version(void);
const char* cfm_get_last_error(void);

/* Graph-safe dropout streams.  Binds a DEVICE uint64 step counter for this process (nullptr
   unbinds).  While bound, every dropout-capable kernel (GEMM epilogue, scale_dropout, attention)
   reads the counter when it RUNS and uses seed + counter * 0x9E3779B97F4A7C15 instead of the
   seed passed at launch, so a training step captured once into a HIP graph draws fresh masks on
   every replay after the caller increments the counter on the stream.  Backward kernels see the
   same counter value as their forward within a step, so masks regenerate bit-identically.
   Replaces the per-call torch RNG state of nn.Dropout (asrnn.py:31, torchaudio Conformer). */
int cfm_rng_bind(const uint64_t* counter);

/* Measurement probes (bench.py roofline timing, also inside a captured HIP graph where HIP events
   cannot be read back on ROCm).  A probe slot is 4 x u64 {start, end, total, count}: mode 0
   resets start = ~0, end = 0 (before the probed launch, which records its first-start / last-end
   into start / end, see cfm_gemm_desc.probe); mode 1 adds end - start to total and 1 to count
   (after it).  Modes 2 / 3 take an 8 x u64 slot {start, end, total, count, stamp, total_incl, -, -}:
   mode 2 is mode 0 plus stamp = the wall clock when this one-lane kernel runs, mode 3 is mode 1 plus
   total_incl += (the wall clock when this one-lane kernel runs) - stamp: stamp-to-stamp around the
   probed launch.  Minus the same interval of an EMPTY pair (mode 2 directly followed by mode 3:
   the two one-lane kernels' own dispatch), it is the time the launch adds to a serial stream --
   its dispatch ramp, execution and end-of-kernel completion, what rocprofv3's kernel trace counts.
   Ticks of the constant-rate GPU wall clock at cfm_wallclock_khz() kHz. */
int cfm_probe_slot(unsigned long long* slot, int mode, void* stream);
int cfm_wallclock_khz(void);

/* y[i] = (dy)x[i] for n elements (dtype conversion; fp32 master weights -> bf16 compute copies). */
int cfm_cast(const void* x, int dtype_x, void* y, int dtype_y, long n, void* stream);

/* Many casts in one launch (the per-step bf16 shadow of every weight matrix): `tasks` is a
   DEVICE array of ntasks cfm_cast_task; task t owns blocks [blk0, blk0 + ceil(n / 2048)) of a grid of
   `nblocks` blocks (blk0 ascending, tasks back to back).  Replaces one cfm_cast launch per weight. */
typedef struct {
  const void* src;
  void* dst;
  long n;
  long blk0;
} cfm_cast_task;
int cfm_cast_batch(const cfm_cast_task* tasks, int ntasks, long nblocks, int dtype_x, int dtype_y,
                   void* stream);

/* Transposed casts in one launch: dst (cols x rows) = (dy) src (rows x cols)^T, row-major both,
   and (when dst_n != NULL) the plain copy dst_n (rows x cols) = (dy) src from the same read.
   Task t owns blocks [blk0, blk0 + ceil(rows/64) * ceil(cols/64)) (64 x 64 tiles).  Used for the
   per-step K-major bf16 copies W^T of the weight matrices, so the data-gradient GEMMs dX = dY W
   read both operands K-major (replaces the MN-major B path of those GEMMs; no reference
   counterpart -- autograd's mm backward, torch/csrc/autograd/FunctionsManual.cpp mm_mat1_backward). */
typedef struct {
  const void* src;   /* fp32 */
  void* dst;         /* transposed copy */
  void* dst_n;       /* optional row-major copy (NULL: none) */
  long rows, cols;
  long blk0;
} cfm_castT_task;
int cfm_cast_transpose_batch(const cfm_castT_task* tasks, int ntasks, long nblocks, int dtype_x, int dtype_y,
                             void* stream);

/* ---------------------------------------------------------------- SpecAugment
 * Replaces ASRNN.SpecAugment / time_warping / frequency_masking / time_masking
 * (lib/standard/asrnn.py:91-192).  The random draws stay on the host (python `random`, the
 * reference's own RNG, in the reference's order); this kernel applies them in ONE pass:
 * y[b,f,t] = x[b,f,Wt_b(t)] (warp passes composed), then the masks when intended != 0
 * (the reference's masks are no-ops as shipped, asrnn.py:141,165).
 * params (device int32): [n_warp, n_freq, n_time, 0,
 *                         n_warp x B x (w, w0, tau), n_freq x (f0, f), n_time x B x (t0, t)]
 * x, y: (B, F, T) fp32, may not alias. */
int cfm_specaug_apply(const float* x, float* y, int B, int F, int T, const int32_t* params,
                      int n_params, int intended, float mask_value, void* stream);

/* ---------------------------------------------------------------- log-mel front-end
 * Replaces the CPU feature step of lib/standard/speechcommands.py:113-119:
 * librosa.feature.melspectrogram(y, sr, n_mels) (periodic Hann, center=True zero padding, |rfft|^2,
 * Slaney mel bank) -> np.where(mel < 1e-10, 0, log(mel)) -> per-utterance min-max (normalize != 0),
 * frames past 1 + lens[b] / hop zero (the collate's padding, speechcommands.py:188).
 * wave (B, ld_wave) fp32, lens (B,) int32 samples; n_fft a power of two in [16, 4096];
 * window (n_fft,) fp32; twiddle (n_fft/2) complex fp32 pairs exp(-2 pi i k / n_fft);
 * filter m = mel_w[mel_off[m] ...+ mel_cnt[m]) applied to power bins mel_lo[m] ...;
 * out (B, n_mels, nT) fp32; ws >= cfm_logmel_ws_bytes(B, nT). */
size_t cfm_logmel_ws_bytes(int B, int nT);
int cfm_logmel_fwd(const float* wave, long ld_wave, const int32_t* lens, int B, int n_fft, int hop,
                   const float* window, const float* twiddle, const int32_t* mel_lo, const int32_t* mel_cnt,
                   const int32_t* mel_off, const float* mel_w, int n_mels, int nT, int normalize, float* out,
                   float* ws, void* stream);

/* ---------------------------------------------------------------- GEMM (MFMA)
 * C[z][m][n] = epilogue( alpha * sum_k A(m,k) * B(n,k) )  for z in [0, batch).
 * Serves every dense contraction of the encoder (torch.nn.Linear / 1x1 Conv1d forward,
 * input-grad and weight-grad): FFN (torchaudio _FeedForwardModule), MHSA in/out projections
 * (nn.MultiheadAttention), point-wise convs (_ConvolutionModule), the front-end projection
 * (asrnn.py:208 / frame projection) and the projection block (asrnn.py:73-89).
 *   A(m,k) = A[m*lda + k] if a_kmajor else A[k*lda + m]
 *   B(n,k) = B[n*ldb + k] if b_kmajor else B[k*ldb + n]
 * (A / B rows may overlap, ld below the row length, only with allow_overlap: read-only windowed views,
 *  cfm_ffold_*.)
 * Epilogue, in order: v = alpha*acc + bias[n];  v *= act'(pre[m,n]) if act_grad;
 *   if act == SILU { pre[m,n] = v (if pre != NULL); v = silu(v) };  v *= dropout(seed, idx);
 *   v *= out_scale;  v += residual[m,n];  C = v  (or atomically C += v when split_k > 1).
 * dtype_ab is the operand type (fp32 operands run on the exact-f32 MFMA path). */
typedef struct cfm_gemm_desc {
  int M, N, K, batch;
  int dtype_ab;
  const void* A; long lda; long stride_a; int a_kmajor;
  const void* B; long ldb; long stride_b; int b_kmajor;
  void* C; long ldc; long stride_c; int dtype_c;
  float alpha;
  const float* bias;
  int act;                 /* CFM_ACT_NONE | CFM_ACT_SILU */
  int act_grad;            /* multiply by silu'(pre) (backward of a SILU epilogue) */
  void* pre; int dtype_pre;
  float drop_p; uint64_t drop_seed; uint64_t drop_offset;
  float out_scale;
  const void* residual; long ldr; int dtype_r;
  int split_k;             /* >1: C must be fp32 with a plain epilogue (alpha, bias) */
  float* workspace;        /* split_k > 1: NULL -> partial sums are atomically added into a
                              pre-initialised C; else >= split_k*batch*M*N floats of slabs that a
                              second pass reduces into C (deterministic, no pre-initialisation) */
  unsigned long long* probe; /* optional timing slot (measurement only): the launch atomically
                              min-records its first workgroup's start and max-records its last
                              workgroup's end (s_memrealtime ticks) into probe[0] / probe[1] */
  float* a_colsum;         /* optional (bf16 LDS-DMA path, MN-major A, split_k > 1 with workspace, batch 1):
                              a_colsum[m] = sum_k A(m, k) -- the bias gradient of a weight-gradient GEMM
                              dW = dY^T X (A = dY^T) -- from the staged A tiles; workspace then needs
                              split_k*M more floats.  NULL: off. */
  const void* rowdot_with; /* optional (bf16 C, LDS-DMA path, N % 64 == 0, batch 1, no split): per row m = b*T + t and
                              64-column group g, rowdot_out[(b * N/64 + g) * T + t] = sum_n C[m][n] * rowdot_with[m*ldc + n]
                              over the bf16-rounded C -- attention's D = rowsum(dO * O) per head (dk = 64) from the
                              out-projection data-gradient GEMM that produces dO.  NULL: off. */
  float* rowdot_out;
  int rowdot_T;
  /* dtype_ab == CFM_FP8: device scalars multiplied into alpha (the per-tensor dequantisation scales
     written by cfm_quant_fp8); NULL: 1 */
  const float* alpha_a_dev;
  const float* alpha_b_dev;
  /* nonzero: A / B rows may overlap (lda / ldb below the row length: the folded front-end's read-only windowed
     view of the packed mels, cfm_ffold_*).  0: lda >= (a_kmajor ? K : M) and ldb >= (b_kmajor ? K : N) are
     enforced (CFM_ERR_SHAPE), so a wrongly transposed view fails instead of reading overlapping rows. */
  int allow_overlap;
  /* dtype_ab == CFM_FP8 with MX operands (both or neither): the e8m0 block scales of A and B as cfm_quant_mx
     writes them ([M][K/32] / [N][K/32] bytes, one per 32 consecutive K elements of a row); the block-scaled MFMA
     applies them per 32-element run (alpha_*_dev must be NULL).  K % 128 == 0, K <= 2048. */
  const uint8_t* mx_a;
  const uint8_t* mx_b;
  /* optional second output (MX fp8 launches with the FFN-up epilogue -- bias + SiLU + bf16 pre + dropout, bf16 C,
     ldc == N, N % 32 == 0): the MX e4m3 copy of the bf16 C, exactly cfm_quant_mx of it -- mx_out (M x N e4m3),
     mx_out_scales (M x N/32 e8m0) -- the next fp8 GEMM's operand, written by the same epilogue.  NULL: off. */
  void* mx_out;
  uint8_t* mx_out_scales;
} cfm_gemm_desc;
int cfm_gemm(const cfm_gemm_desc* d, void* stream);
/* Per-tensor fp8 (e4m3fn) quantisation for the fp8 GEMM path (configs[4]; no reference counterpart -- the
   reference computes in fp32): y = e4m3(x * 2^k), k the largest with amax(|x|) * 2^k <= 448, *inv_scale = 2^-k (device scalar for
   cfm_gemm_desc.alpha_*_dev); amax_ws: cfm_quant_fp8_ws_bytes() of scratch.  x fp32 or bf16, 16-B aligned. */
size_t cfm_quant_fp8_ws_bytes(void);
int cfm_quant_fp8(const void* x, int dtype_x, long n, void* y, float* inv_scale, unsigned* amax_ws, void* stream);
/* Batched cfm_quant_fp8 over a device table of tensors (the per-step fp8 copies of a model's forward GEMM
   weights, configs[4]): TWO launches for the whole list instead of two per tensor; per tensor the same
   current scaling, scale and e4m3 bytes as cfm_quant_fp8 (the max is order-independent: bit-identical).
   Replaces the per-weight quantisation loop of the fp8 path (no reference counterpart: the reference has
   no fp8).  tasks: device array; blk0 = prefix sum of cfm_quant_fp8_batch_blocks(n) over the tasks;
   amax_ws: nblocks floats of scratch. */
typedef struct {
  const void* x;      /* fp32 or bf16 (dtype_x of the call), 16-B aligned */
  void* y;            /* e4m3 bytes, 8-B aligned */
  float* inv_scale;   /* dequantisation factor 2^-k (device scalar) */
  long n;
  long blk0;
} cfm_q8_task;
long cfm_quant_fp8_batch_blocks(long n);
int cfm_quant_fp8_batch(const cfm_q8_task* tasks, int ntasks, long nblocks, int dtype_x, float* amax_ws,
                        void* stream);
/* y = float(x) * inv_scale (inv_scale NULL: 1) -- the dequantised view, for tests. */
int cfm_dequant_fp8(const void* x, long n, const float* inv_scale, float* y, void* stream);
/* MX e4m3 quantisation (OCP microscaling; configs[4]'s fp8 path, no reference counterpart): every 32
   consecutive elements of a row share one e8m0 scale byte s = 127 - k, k the largest integer with
   amax(block) * 2^k <= 448 (0 for an all-zero block), and y = e4m3(x * 2^k) (round to nearest even).
   x: rows x K (row stride ldx elements, fp32 or bf16, 16-B aligned), K % 32 == 0; y: rows x K bytes
   (row stride K); s: rows x K/32 bytes (row-major).  One pass, no tensor-wide amax: the operand form of
   cfm_gemm_desc.mx_a / mx_b. */
int cfm_quant_mx(const void* x, int dtype_x, long rows, int K, long ldx, void* y, uint8_t* s, void* stream);
/* Batched cfm_quant_mx over a device table (the per-step MX copies of the forward GEMM weights): ONE launch;
   blk0 = prefix sum of cfm_quant_mx_batch_blocks(rows, K); rows of each tensor contiguous (ldx = K). */
typedef struct {
  const void* x;      /* fp32 or bf16 (dtype_x of the call), 16-B aligned */
  void* y;            /* e4m3 bytes, 8-B aligned */
  uint8_t* s;         /* e8m0 block scales, rows x K/32 */
  long rows;
  int K;
  int pad;
  long blk0;
} cfm_mx_task;
long cfm_quant_mx_batch_blocks(long rows, int K);
int cfm_quant_mx_batch(const cfm_mx_task* tasks, int ntasks, long nblocks, int dtype_x, void* stream);
/* y[i] = e4m3(x[i]) * 2^(s[i / 32] - 127) -- the dequantised view of an MX tensor (n % 32 == 0), for tests. */
int cfm_dequant_mx(const void* x, const uint8_t* s, long n, float* y, void* stream);
/* Grouped weight gradients: every dW_i (N_i x K_i, fp32) = dY_i^T X_i over the same M tokens (dY_i (M x N_i),
   X_i (M x K_i) bf16 row-major) and optionally db_i = sum_rows dY_i, in ONE launch of 256x128 tiles that each
   run the whole token reduction (no split-K).  The caller fills a HOST table (cfm_wgrad_group_fill, one
   entry of cfm_wgrad_group_task_bytes() per GEMM, tile0 = running sum of cfm_wgrad_group_tiles), copies it
   to the device and launches total_tiles workgroups.  Replaces the per-GEMM split-K weight gradients of
   the encoder backward (torch autograd's per-Linear mm for grad_weight, FunctionsManual.cpp). */
size_t cfm_wgrad_group_task_bytes(void);
long cfm_wgrad_group_tiles(int N, int K);
int cfm_wgrad_group_fill(void* host_table, int i, const void* dy, const void* x, float* dw, float* db, int M,
                         int N, int K, long tile0);
int cfm_wgrad_group(const void* dev_table, int ntasks, long total_tiles, void* stream);
/* Grouped deterministic column reductions: the small deferred reductions of a backward pass (LayerNorm
   dgamma|dbeta partial rows -- torch's LayerNorm backward weight/bias sums --, depthwise-conv weight/bias
   partials) in ONE launch.  Host table of cfm_colreduce_group_task_bytes() per task (block0 = running sum of
   cfm_colreduce_group_blocks(N)); mode 0: out[n] = sum_p part[p*ldp + n]; mode 1: the depthwise-conv
   [K+1][C] sums scattered to dw (C x K) and db (C). */
size_t cfm_colreduce_group_task_bytes(void);
long cfm_colreduce_group_blocks(long N);
int cfm_colreduce_group_fill(void* host_table, int i, const float* part, int nparts, long N, long ldp, float* out,
                             float* out2, int mode, int C, int K, long block0);
int cfm_colreduce_group(const void* dev_table, int ntasks, long total_blocks, void* stream);
/* the same launch with a timing slot (as cfm_gemm_desc.probe: first-workgroup start / last-workgroup end) */
int cfm_wgrad_group_probed(const void* dev_table, int ntasks, long total_tiles, unsigned long long* probe,
                           void* stream);
/* Planned grouped weight gradients (the encoder backward's default): cfm_wgrad_group_plan packs the tasks'
   tiles (task_tiles[i] = cfm_wgrad_group_tiles(N_i, K_i)) into rounds of one tile per CU per XCD (nxcd XCDs of
   cus CUs) made of whole tasks -- the tiles sharing a dY or X column slice co-resident on one XCD, which then
   streams the slice through its L2 once -- and splits the tiles of the ragged last round over K slices
   (task_split[i] > 1), so that round fills the chip.  It writes one schedule word per workgroup (sched, capacity
   cap) and returns the grid size (< 0: error).  Fill the table with cfm_wgrad_group_fill_split (split = the
   plan's task_split[i]; ws = cfm_wgrad_group_ws_floats(N, K, split) floats of fp32 workspace for a split task;
   red0 = running sum of cfm_wgrad_group_red_blocks), copy table and schedule to the device and launch
   cfm_wgrad_group_sched (red_blocks = the total): the GEMM launch, then the deterministic slab reduction of the
   split tasks into dw / db.  probe: optional timing slot (as cfm_wgrad_group_probed). */
long cfm_wgrad_group_plan(const long* task_tiles, int ntasks, int nxcd, int cus, unsigned* sched, long cap,
                          int* task_split);
long cfm_wgrad_group_ws_floats(int N, int K, int split);
long cfm_wgrad_group_red_blocks(int N, int K, int split);
int cfm_wgrad_group_fill_split(void* host_table, int i, const void* dy, const void* x, float* dw, float* db, int M,
                               int N, int K, int split, float* ws, long red0);
int cfm_wgrad_group_sched(const void* dev_table, int ntasks, const unsigned* dev_sched, long grid, long red_blocks,
                          unsigned long long* probe, void* stream);
/* cfm_gemm_set_mode: the kernel-selection word, for A/B measurements and the tests that compare variants bit for
   bit.  These enumerators are the one description of its bits (nn_conformer_for_speech_recognition_amd/_lib.py
   mirrors them as GEMM_MODE_*); bits without a name are read by nothing. */
enum cfm_gemm_mode {
  CFM_GEMM_MODE_STAGED256 = 1 << 0,       /* keeps the 256-row register-staged bf16 tiles allowed */
  CFM_GEMM_MODE_PIPE = 1 << 1,            /* keeps the LDS-DMA kernels (pipeline, warp-specialised, conv2) allowed */
  CFM_GEMM_MODE_DEFAULT = 3,              /* STAGED256 | PIPE */
  CFM_GEMM_MODE_SKIP_STORES = 1 << 3,     /* timing: LDS-DMA kernels skip the epilogue's stores (outputs invalid) */
  CFM_GEMM_MODE_SEL_SHIFT = 4,            /* bits 4-6: force one bf16 pipeline variant, CFM_GEMM_SEL_* << SEL_SHIFT */
  CFM_GEMM_MODE_SEL_MASK = 7 << 4,
  CFM_GEMM_MODE_GENERIC_DROPOUT = 1 << 10, /* keeps the generic dropout hash path of the epilogue */
  CFM_GEMM_MODE_NO_192S8_RULE = 1 << 12,  /* skips the 192-row rule for 513..1536-wide outputs of short reductions */
  CFM_GEMM_MODE_SKIP_MAINLOOP = 1 << 13,  /* timing: LDS-DMA kernels skip the main loop (epilogue only) */
  CFM_GEMM_MODE_GENERIC_EPILOGUE = 1 << 14, /* keeps the generic epilogue rows instead of the compile-time kinds */
  CFM_GEMM_MODE_KEEP_SHARED_DMA = 1 << 19, /* keeps the 4-deep 192-row pipeline where the warp-specialised kernel runs */
  CFM_GEMM_MODE_KEEP_PIPE192 = 1 << 21,   /* keeps the two-per-CU 192-row pipeline for 513..1536-wide outputs */
  CFM_GEMM_MODE_KEEP_128WIDE = 1 << 22,   /* keeps 128-wide tiles for 129..160-column outputs (skips the 64 x 160 tile) */
  CFM_GEMM_MODE_KEEP_WS192 = 1 << 23      /* keeps the 192-row warp-specialised tiles where 96-row ones would run */
};
/* values of the selector field (only the variants a layout has are forced; anything else means auto) */
enum cfm_gemm_sel {
  CFM_GEMM_SEL_AUTO = 0,
  CFM_GEMM_SEL_PIPE256 = 1,               /* 256 x 128, BK 64, one workgroup per CU */
  CFM_GEMM_SEL_PIPE256S = 2,              /* 256 x 128, BK 32, two per CU */
  CFM_GEMM_SEL_192 = 5,                   /* 192 x 128: warp-specialised (K-major x K-major) or the 4-deep pipeline */
  CFM_GEMM_SEL_PIPE192S8 = 7              /* 192 x 128, BK 32, two per CU */
};
int cfm_gemm_set_mode(int mode);

/* The kernel a cfm_gemm call runs (csrc/gemm_variants.h documents each variant's geometry). */
enum cfm_gemm_variant {
  CFM_GEMM_V_NONE = 0,                    /* M == 0 or N == 0: nothing is launched */
  CFM_GEMM_V_STAGED_BF16_256,             /* register-staged bf16, 256 x 128 tiles */
  CFM_GEMM_V_STAGED_BF16_128,             /* register-staged bf16, 128 x 128 tiles */
  CFM_GEMM_V_STAGED_F32_128,              /* register-staged fp32, 128 x 128 tiles */
  CFM_GEMM_V_STAGED_F32_64,               /* register-staged fp32, 64 x 64 tiles */
  CFM_GEMM_V_PIPE64X160,                  /* LDS-DMA pipeline, 64 x 160 tiles */
  CFM_GEMM_V_WS192,                       /* warp-specialised, 192 x 128 tiles */
  CFM_GEMM_V_WS96,                        /* warp-specialised, 96 x 128 tiles */
  CFM_GEMM_V_PIPE192,                     /* pipeline, 192 x 128, BK 64, 4-deep ring */
  CFM_GEMM_V_PIPE192S8,                   /* pipeline, 192 x 128, BK 32, two per CU */
  CFM_GEMM_V_PIPE256,                     /* pipeline, 256 x 128, BK 64 */
  CFM_GEMM_V_PIPE256S,                    /* pipeline, 256 x 128, BK 32, two per CU */
  CFM_GEMM_V_FP8_192,                     /* per-tensor fp8, 192 x 128 */
  CFM_GEMM_V_FP8_256S,                    /* per-tensor fp8, 256 x 128, two per CU */
  CFM_GEMM_V_MX192,                       /* MX fp8, 192 x 128 */
  CFM_GEMM_V_MX256S                       /* MX fp8, 256 x 128, two per CU */
};
/* The staged epilogue a launch carries: GENERIC is the run-time epilogue rows, every other kind a body fixed at
   compile time (csrc/gemm_epilogue.h). */
enum cfm_gemm_epilogue {
  CFM_GEMM_EPI_GENERIC = 0, CFM_GEMM_EPI_BF16 = 1, CFM_GEMM_EPI_BF16_BIAS = 2, CFM_GEMM_EPI_BF16_SILU = 3,
  CFM_GEMM_EPI_BF16_ACTG = 4, CFM_GEMM_EPI_BF16_RD = 5, CFM_GEMM_EPI_F32 = 6, CFM_GEMM_EPI_F32_RES = 7,
  CFM_GEMM_EPI_BF16_SILU_MX = 8, CFM_GEMM_EPI_BF16_RES = 9, CFM_GEMM_EPI_F32R_BF16 = 10, CFM_GEMM_EPI_BF16_DELTA = 11
};
typedef struct {
  int variant;                            /* cfm_gemm_variant */
  int epilogue;                           /* cfm_gemm_epilogue */
  unsigned grid_x, grid_y, grid_z;
  unsigned block;
} cfm_gemm_choice;
/* What cfm_gemm(d) would launch under `mode` (< 0: the current cfm_gemm_set_mode value) on a device of `cus`
   compute units: the same validation and selection as cfm_gemm, the same error codes, and no launch -- it calls
   no GPU API and reads only the values and alignment of the descriptor's pointers. */
int cfm_gemm_plan(const cfm_gemm_desc* d, int mode, int cus, cfm_gemm_choice* out);

/* out[n] (+)= sum_m x[m*ld + n]  — bias gradients (sum over tokens).  ws: >= 4*N*256 bytes. */
/* out[n] (+)= sum_p part[p * ldp + n] for n < N: the deterministic second level of every partial-row
   reduction (LayerNorm dgamma|dbeta partials left by cfm_layernorm_bwd with NULL dgamma/dbeta, so the
   weight-gradient reduction can run on another stream). */
int cfm_colreduce(const float* part, int nparts, long N, long ldp, float* out, int accumulate, void* stream);
int cfm_colsum(const void* x, int dtype_x, long M, int N, long ld, float* out, int accumulate,
               float* ws, void* stream);

/* ---------------------------------------------------------------- LayerNorm (nn.LayerNorm(D))
 * Forward: y = (x-mean)*rstd*gamma + beta; saves mean/rstd per row.
 * Backward: dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) + dres, g = dy*gamma;
 * dgamma/dbeta accumulate (+=) over rows.  ws: >= 8*D*nblk bytes, see cfm_layernorm_ws_bytes. */
int cfm_layernorm_fwd(const void* x, int dtype_x, const float* gamma, const float* beta, void* y,
                      int dtype_y, float* mean, float* rstd, long M, int D, float eps, void* stream);
/* The same forward (fp32 x, bf16 y) with a second output: y's MX e4m3 copy -- y8 (M x D e4m3) and s8
   (M x D/32 e8m0), exactly cfm_quant_mx of the bf16 y -- for the fp8 forward GEMM that consumes it
   (configs[4]); D in {256, 512, 1024}. */
int cfm_layernorm_fwd_mx(const float* x, const float* gamma, const float* beta, void* y, void* y8, uint8_t* s8,
                         float* mean, float* rstd, long M, int D, float eps, void* stream);
/* The same with x of dtype_x (CFM_F32 or CFM_BF16: the bf16 mode's bf16 residual stream). */
int cfm_layernorm_fwd_mx_ex(const void* x, int dtype_x, const float* gamma, const float* beta, void* y, void* y8,
                            uint8_t* s8, float* mean, float* rstd, long M, int D, float eps, void* stream);
/* The residual add of the module before a LayerNorm, done by the LayerNorm: xout = x + delta (fp32; delta of dtype_d,
   CFM_BF16 -- the module's GEMM output with bias, dropout and out_scale, no residual -- or CFM_F32), then
   y = LN(xout) as cfm_layernorm_fwd, and, with y8 / s8 non-null, y's MX copy as cfm_layernorm_fwd_mx.  Replaces the
   residual-stream GEMM epilogue `x + out_scale * dropout(h W^T + b)` (torchaudio ConformerLayer, ffn / attention /
   conv residual adds; asrnn.py:214) followed by the next module's LayerNorm.  xout must not alias x or
   delta. */
int cfm_layernorm_fwd_res(const float* x, const void* delta, int dtype_d, float* xout, const float* gamma,
                          const float* beta, void* y, int dtype_y, void* y8, uint8_t* s8, float* mean, float* rstd,
                          long M, int D, float eps, void* stream);
size_t cfm_layernorm_ws_bytes(long M, int D);   /* (blocks + 1) * 8*D bytes (cfm_layernorm_plan); 0 for a refused D / M */
int cfm_layernorm_bwd(const void* dy, int dtype_dy, const void* x, int dtype_x, const float* gamma,
                      const float* mean, const float* rstd, const void* dres, int dtype_dres,
                      void* dx, int dtype_dx, float* dgamma, float* dbeta, float* ws, long M, int D,
                      void* stream);
/* The same plus g2 (bf16, M x D) = dx * g2_scale * dropout(g2_p, g2_seed, element index) -- exactly
   cfm_scale_dropout(dx, ..., offset 0) -- written by the same pass: the next module's (residual-
   dropout) input gradient in the encoder backward.  g2 == NULL: identical to cfm_layernorm_bwd. */
int cfm_layernorm_bwd_drop(const void* dy, int dtdy, const void* x, int dtx, const float* gamma,
                           const float* mean, const float* rstd, const void* dres, int dtres, void* dx,
                           int dtdx, float* dgamma, float* dbeta, float* ws, long M, int D, void* g2,
                           float g2_scale, float g2_p, uint64_t g2_seed, void* stream);

/* Two LayerNorms back to back (an encoder layer's final_layer_norm followed by the next layer's ffn1 LayerNorm) as one
   kernel per direction.  Forward: y = LN(x; gamma1, beta1) (fp32) and z = LN(y; gamma2, beta2) (dtype_z), with both
   rows of statistics -- y, z and the statistics are bit-identical to two cfm_layernorm_fwd calls, and y is never read
   back.  Backward: dz (dtype_dz) is the gradient of z, dres (fp32, nullable) the gradient reaching y directly;
   dx = LN1'(dres + LN2'(dz)) with y recomputed from x, g2 as cfm_layernorm_bwd_drop's.  dgb1 / dgb2: [dgamma | dbeta]
   (2*D floats each) of the first / second LayerNorm; NULL leaves that pair's partial rows in ws for the caller to
   reduce -- nb = ws_bytes / (16*D) rows of 2*D floats for the first pair at ws, the same for the second at
   ws + nb*2*D.
   cfm_layernorm_pair_ok: 1 when fused kernels exist for width D and dtype_z (D 512, 256, and the lane-group widths
   D % 8 == 0, D < 512, D != 128), else 0 -- then make the two calls; pure host logic, no GPU API (cfm_layernorm_plan
   of a CFM_LN_FWD_PAIR query).  All pointers 16-B aligned (CFM_ERR_ALIGN otherwise). */
int cfm_layernorm_pair_ok(int D, int dtype_z);
size_t cfm_layernorm_fwd_pair_ws_bytes(long M, int D);   /* 0: the forward needs no workspace */
int cfm_layernorm_fwd_pair(const float* x, const float* gamma1, const float* beta1, const float* gamma2,
                           const float* beta2, float* y, void* z, int dtype_z, float* mean1, float* rstd1,
                           float* mean2, float* rstd2, long M, int D, float eps, void* stream);
size_t cfm_layernorm_bwd_pair_ws_bytes(long M, int D);   /* 0 where cfm_layernorm_pair_ok(D, ...) is 0 */
int cfm_layernorm_bwd_pair(const void* dz, int dtype_dz, const float* dres, const float* x, const float* gamma1,
                           const float* beta1, const float* mean1, const float* rstd1, const float* gamma2,
                           const float* mean2, const float* rstd2, float* dx, float* dgb1, float* dgb2, float* ws,
                           long M, int D, void* g2, float g2_scale, float g2_p, uint64_t g2_seed, void* stream);

/* What the LayerNorm entry points above launch, as a pure host function (csrc/ln_plan.h): every cfm_layernorm_* call,
   cfm_layernorm_ws_bytes, cfm_layernorm_bwd_pair_ws_bytes and cfm_layernorm_pair_ok act on this one rule. */
enum cfm_ln_op {
  CFM_LN_FWD = 0,                         /* cfm_layernorm_fwd, cfm_layernorm_fwd_mx(_ex) (want_mx) */
  CFM_LN_FWD_RES = 1,                     /* cfm_layernorm_fwd_res */
  CFM_LN_BWD = 2,                         /* cfm_layernorm_bwd, cfm_layernorm_bwd_drop (want_g2) */
  CFM_LN_FWD_PAIR = 3,
  CFM_LN_BWD_PAIR = 4
};
enum cfm_ln_family {
  CFM_LN_GENERIC = 0,                     /* any D <= 1024, any alignment: one wave per row, 4-byte strided elements */
  CFM_LN_WAVE = 1,                        /* D = 64 * width: one wave per row, width features per lane */
  CFM_LN_GROUP = 2                        /* D % 8 == 0, D <= 512: width lanes per row, 8 features per lane */
};
typedef struct {
  int op;                                 /* cfm_ln_op */
  int D;
  int64_t M;
  /* dtype codes of the operands the op has (the others are ignored): x; y (pair: z); dy (pair: dz); dx; dres
     (CFM_F32 when there is none); fwd_res's delta */
  int dt_x, dt_y, dt_dy, dt_dx, dt_dres, dt_delta;
  /* the pointers' addresses modulo 16, 0 for the ones the op does not have or that are NULL.  gamma / beta: the
     (first) LayerNorm's; gamma2 / beta2: the pair's second; y: the pair's fp32 y, z its second output */
  int x_mod16, y_mod16, z_mod16, gamma_mod16, beta_mod16, gamma2_mod16, beta2_mod16;
  int delta_mod16, xout_mod16, y8_mod16;  /* fwd_res: delta, xout; the MX copy's y8 */
  int dy_mod16, dres_mod16, dx_mod16, g2_mod16;
  int want_mx;                            /* forward: also y's MX e4m3 copy (y8, s8) */
  int want_g2;                            /* backward: also g2 = bf16(dx * scale * dropout) */
} cfm_ln_query;
typedef struct {
  int family;                             /* cfm_ln_family */
  int width;                              /* WAVE: V = D / 64 in {2, 4, 8, 16}; GROUP: G in {16, 32, 64}; GENERIC: 0 */
  int g2_fused;                           /* g2 written by the LayerNorm kernel; 0: a cfm_scale_dropout pass over dx */
  int blocks;                             /* workgroups (of 256 threads) of the LayerNorm kernel */
  size_t ws_bytes;                        /* backward workspace (cfm_layernorm_ws_bytes / _bwd_pair_ws_bytes); forward 0 */
} cfm_ln_choice;
/* Calls no GPU API.  CFM_ERR_ARG for a null pointer or an unknown op; otherwise the code the entry point returns for
   the same input before it launches anything: CFM_ERR_DTYPE for a y / z / dy / dz (delta, the MX forward's x) that is
   neither CFM_F32 nor CFM_BF16, CFM_ERR_SHAPE for D outside (0, 1024], M < 0, an MX copy off D in {256, 512, 1024} /
   bf16 y, or a pair width without fused kernels, CFM_ERR_ALIGN for an MX copy or a pair with a pointer off 16 bytes.
   The single-LayerNorm entry points never fail on alignment or x / dx / dres dtypes: such calls run GENERIC. */
int cfm_layernorm_plan(const cfm_ln_query* q, cfm_ln_choice* out);

/* y = act(x*scale [dropout]) + residual, elementwise helpers used at residual joins. */
int cfm_scale_dropout(const void* x, int dtype_x, void* y, int dtype_y, long n, float scale,
                      float drop_p, uint64_t seed, uint64_t offset, void* stream);

/* dx = dy * silu'(pre) elementwise (backward of a SILU GEMM epilogue when the gradient feeds a
 * weight-gradient GEMM directly, e.g. the projection block asrnn.py:84-87). */
int cfm_silu_bwd(const void* dy, int dtype_dy, const void* pre, int dtype_pre, void* dx, int dtype_dx,
                 long n, void* stream);

/* ---------------------------------------------------------------- Convolution module
 * _ConvolutionModule (torchaudio; restated oracle/conformer.py ConvModuleRef):
 *   a = pw1(LN(x)) (cfm_gemm), g = GLU(a) (dim = channel), y = depthwise_conv_K(g) + b,
 *   z = SiLU(BatchNorm1d(y)) (train: batch statistics over B*T incl. padded frames),
 *   out = pw2(z) (cfm_gemm, + residual).
 * a: (B*T, 2C) token-major; w_dw: (C, K) fp32; y: (B*T, C) fp32.
 * cfm_glu_dwconv_fwd also produces per-channel partial (sum, sumsq) into ws for BN. */
size_t cfm_convmod_ws_bytes(int B, int T, int C, int K);
/* rows of cfm_glu_dwconv_bwd's [nparts][K+1][C] weight-gradient partials in ws (mode 1 of cfm_colreduce_group) */
long cfm_convmod_nparts(int B, int T);
int cfm_glu_dwconv_fwd(const void* a, int dtype_a, const float* w_dw, const float* b_dw, float* y,
                       int B, int T, int C, int K, float* ws, void* stream);
/* z = silu(bn(y)).  training: batch stats finalised from the partial sums cfm_glu_dwconv_fwd left
 * in ws (same B, T, C), running stats updated (momentum, unbiased var); eval: running stats.
 * Writes mean/invstd (C each) for the backward. */
int cfm_bn_silu_fwd(const float* y, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float momentum, float eps, int training, float* mean,
                    float* invstd, void* z, int dtype_z, int B, int T, int C, const float* ws,
                    void* stream);
/* backward of z = silu(bn(y)): dy = BN-bwd(dz*silu'(bn(y))); dgamma, dbeta (=) written. */
int cfm_bn_silu_bwd(const void* dz, int dtype_dz, const float* y, const float* gamma,
                    const float* beta, const float* mean, const float* invstd, int training,
                    float* dy, float* dgamma, float* dbeta, long M, int C, float* ws, void* stream);
/* SyncBatchNorm split of cfm_bn_silu_fwd / cfm_bn_silu_bwd (the host all-reduces `sums` / the dbeta|dgamma
   sums between the halves; M_total = rows over all replicas).  Replaces torch.nn.SyncBatchNorm over the
   ConvModule's BatchNorm1d (torchaudio conformer, asrnn.py:29) under data parallelism. */
int cfm_bn_silu_fwd_sums(const float* ws, int B, int T, int C, float* sums, void* stream);
int cfm_bn_silu_fwd_apply(const float* y, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, float momentum, float eps, const float* sums, long M_total, float* mean,
                          float* invstd, void* z, int dtz, long M, int C, void* stream);
int cfm_bn_silu_bwd_sums(const void* dz, int dtdz, const float* y, const float* gamma, const float* beta,
                         const float* mean, const float* invstd, long M, int C, float* ws, float* dbeta, float* dgamma,
                         void* stream);
int cfm_bn_silu_bwd_apply(const void* dz, int dtdz, const float* y, const float* gamma, const float* beta,
                          const float* mean, const float* invstd, const float* dbeta_total, const float* dgamma_total,
                          long M_total, float* dy, long M, int C, void* stream);
/* Generic BatchNorm1d over (M, C) rows with optional SiLU after the normalisation (act = 1) —
 * the projection block's BatchNorm1d(256) (lib/standard/asrnn.py:32,88).  ws: cfm_bn_ws_bytes(C). */
size_t cfm_bn_ws_bytes(int C);
int cfm_bn_fwd(const float* y, const float* gamma, const float* beta, float* running_mean,
               float* running_var, float momentum, float eps, int training, float* mean, float* invstd,
               void* z, int dtype_z, long M, int C, int act, float* ws, void* stream);
int cfm_bn_bwd(const void* dz, int dtype_dz, const float* y, const float* gamma, const float* beta,
               const float* mean, const float* invstd, int training, int act, float* dy, float* dgamma,
               float* dbeta, long M, int C, float* ws, void* stream);
/* backward of y = dwconv(GLU(a)): da (B*T, 2C), dw (C,K) (=), db (C) (=). */
int cfm_glu_dwconv_bwd(const float* dy, const void* a, int dtype_a, const float* w_dw, void* da,
                       int dtype_da, float* dw, float* db, int B, int T, int C, int K, float* ws,
                       void* stream);
/* With dw == NULL, cfm_glu_dwconv_bwd leaves the depthwise weight/bias partial sums in ws; this
   reduces them (deterministically) into dw (C x K) and db (C) -- on any stream ordered after it. */
int cfm_glu_dwconv_bwd_wgrad(float* ws, int B, int T, int C, int K, float* dw, float* db, void* stream);
/* cfm_bn_silu_bwd_apply folded into cfm_glu_dwconv_bwd: the BatchNorm1d + SiLU input gradient
 *   dy = gamma*invstd*(du - dbeta*invM - yhat*dgamma*invM)   (training; eval: gamma*invstd*du)
 * is formed inside the depthwise backward from dz, y and the stats, never stored (torchaudio
 * ConformerLayer conv_module BatchNorm1d -> SiLU -> depthwise).  dbeta / dgamma:
 * from cfm_bn_silu_bwd_sums (or their SyncBatchNorm all-reduced totals with invM = 1 / rows summed
 * over).  K must be one of 3, 5, 7, 15, 31, 33.  dw == NULL: partials left in ws as above. */
int cfm_glu_dwconv_bwd_bn(const void* dz, int dtype_dz, const float* y, const float* gamma, const float* beta,
                          const float* mean, const float* invstd, const float* dbeta, const float* dgamma,
                          float invM, int training, const void* a, int dtype_a, const float* w_dw, void* da,
                          int dtype_da, float* dw, float* db, int B, int T, int C, int K, float* ws, void* stream);
/* use_group_norm=True: torch.nn.GroupNorm(1, C, eps, affine) in place of the BatchNorm1d (torchaudio
 * _ConvolutionModule; oracle/conformer.py ConvModuleRef).  Statistics are per sample b over ALL T*C elements of
 * that sample, padded frames included (nothing is masked, as for BatchNorm), variance biased, no running
 * statistics, train == eval.  One-pass (sum, sumsq) statistics like the BatchNorm path: finalised in double from
 * the [2][nparts][C] partials cfm_glu_dwconv_fwd left in ws (rows b*ceil(T/64) .. of sample b), fixed summation
 * order, no atomics.
 *   fwd:  z = silu((y - mean[b]) * rstd[b] * gamma[c] + beta[c]);  mean, rstd: (B) fp32, saved for the backward.
 *   bwd:  yhat = (y - mean[b]) * rstd[b],  du = dz * silu'(yhat*gamma[c] + beta[c]),
 *         dbeta[c] = sum_{b,t} du,  dgamma[c] = sum_{b,t} du*yhat,
 *         k1[b] = (1/(T*C)) sum_{t,c} gamma[c]*du,  k2[b] = (1/(T*C)) sum_{t,c} gamma[c]*du*yhat,
 *         dy = rstd[b] * (gamma[c]*du - k1[b] - yhat*k2[b]).
 * coef: caller-provided (B, 2) fp32 buffer of (k1[b], k2[b]) rows -- NOT part of ws, because the depthwise
 * backward that reads it overwrites ws with its weight-gradient partials. */
int cfm_gn_silu_fwd(const float* y, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                    void* z, int dtype_z, int B, int T, int C, const float* ws, void* stream);
/* one pass over dz and y: dbeta, dgamma (C each, =) and coef (B, 2); ws: cfm_convmod_ws_bytes (used for the
 * [2][nparts][C] partials of (sum du, sum du*yhat)). */
int cfm_gn_silu_bwd_sums(const void* dz, int dtype_dz, const float* y, const float* gamma, const float* beta,
                         const float* mean, const float* rstd, int B, int T, int C, float* ws, float* dbeta,
                         float* dgamma, float* coef, void* stream);
/* cfm_glu_dwconv_bwd with dy formed inside the depthwise kernel from dz, y, the statistics and coef (after
 * cfm_gn_silu_bwd_sums), never stored.  K must be one of 3, 5, 7, 15, 31, 33.  dw == NULL: partials left in ws
 * for cfm_glu_dwconv_bwd_wgrad. */
int cfm_glu_dwconv_bwd_gn(const void* dz, int dtype_dz, const float* y, const float* gamma, const float* beta,
                          const float* mean, const float* rstd, const float* coef, const void* a, int dtype_a,
                          const float* w_dw, void* da, int dtype_da, float* dw, float* db, int B, int T, int C, int K,
                          float* ws, void* stream);
/* unfused fallback (any K): the sums above, then dy (B*T, C) fp32 written; cfm_glu_dwconv_bwd follows it. */
int cfm_gn_silu_bwd(const void* dz, int dtype_dz, const float* y, const float* gamma, const float* beta,
                    const float* mean, const float* rstd, float* dy, float* dgamma, float* dbeta, float* coef,
                    int B, int T, int C, float* ws, void* stream);

/* Which kernels the conv-module entry points above launch (csrc/convmod.hip), as a pure host function. */
enum cfm_convmod_op {
  CFM_CONVMOD_OP_FWD = 0,                 /* cfm_glu_dwconv_fwd */
  CFM_CONVMOD_OP_BWD = 1,                 /* cfm_glu_dwconv_bwd */
  CFM_CONVMOD_OP_BWD_BN = 2,              /* cfm_glu_dwconv_bwd_bn */
  CFM_CONVMOD_OP_BWD_GN = 3               /* cfm_glu_dwconv_bwd_gn */
};
enum cfm_convmod_family {
  CFM_CONVMOD_FAM_UNSUPPORTED = 0,        /* the entry point returns CFM_ERR_UNSUPPORTED */
  CFM_CONVMOD_FAM_VEC = 1,                /* 4 channels per lane through LDS: bf16 a (and da), C % 4 == 0, compiled K */
  CFM_CONVMOD_FAM_SCALAR_KT = 2,          /* one channel per lane, K a template parameter (3, 5, 7, 15, 31, 33) */
  CFM_CONVMOD_FAM_SCALAR_KRT = 3          /* one channel per lane, K at run time (any odd K <= 63; no folded backward) */
};
enum cfm_convmod_apply {
  CFM_CONVMOD_APPLY_NONE = 0,             /* no z pointer in the query */
  CFM_CONVMOD_APPLY_SCALAR = 1,           /* grid-stride, one element per thread per iteration: any C, any alignment */
  CFM_CONVMOD_APPLY_VEC8 = 2              /* 8 elements per thread: C % 8 == 0, y and z 16-byte aligned */
};
typedef struct {
  int op;                                 /* cfm_convmod_op */
  int norm;                               /* the apply kernel's norm: 0 BatchNorm (cfm_bn_silu_fwd, cfm_bn_fwd), 1 GroupNorm */
  int dtype_a, dtype_da, dtype_dz, dtype_z;
  long M;                                 /* rows of y / z (B*T) */
  int C, K;
  const void* y;                          /* only the alignment of y and z is read; z NULL: no apply kernel asked for */
  const void* z;
  int force_scalar;                       /* < 0: the CFM_DWCONV_SCALAR environment switch as the library read it; 0 / 1 */
} cfm_convmod_query;
typedef struct {
  int family;                             /* cfm_convmod_family of the depthwise kernel of `op` */
  int dz16;                               /* folded vectorised backward: 1 when dz is staged as bf16 */
  int apply;                              /* cfm_convmod_apply */
} cfm_convmod_choice;
/* The selection the launchers themselves make (they call the same routine); calls no GPU API.  Returns CFM_OK with
   family UNSUPPORTED for a kernel size no kernel of `op` exists for, CFM_ERR_ARG for a null pointer or an unknown op. */
int cfm_convmod_plan(const cfm_convmod_query* q, cfm_convmod_choice* out);

/* ---------------------------------------------------------------- Attention
 * nn.MultiheadAttention(need_weights=False, key_padding_mask) core (torchaudio ConformerLayer
 * self_attn), optionally with Transformer-XL relative positions (transformers
 * Wav2Vec2ConformerSelfAttention, scores=((q+u)k^T + (q+v)p_{T-1-i+j}^T)/sqrt(dk)).
 * qkv: (B*T, 3*H*dk) rows [q | k | v]; o: (B*T, H*dk); lse: (B*H*T) fp32 log-sum-exp per query
 * (saved for backward); lengths: (B) int32 valid keys.  pos (rel only): (2T-1, H*dk) projected
 * table; pos_u / pos_v: (H*dk) fp32.  dtype: CFM_BF16 (MFMA) or CFM_F32. */
/* cfm_attn_set_mode: A/B switches (measurement and cross-check tests only); default 0.  These enumerators are
   the one description of the bits (mirrored as ATTN_MODE_* in _lib.py). */
enum cfm_attn_mode {
  CFM_ATTN_MODE_TILED = 1 << 0,           /* skips the whole-head kernels (T <= 384): the tiled ones run */
  CFM_ATTN_MODE_STAGING_ONLY = 1 << 1,    /* timing: the whole-head forward stops after staging (outputs invalid) */
  CFM_ATTN_MODE_SKIP_STORES = 1 << 2,     /* timing: the whole-head forward skips its output stores */
  CFM_ATTN_MODE_REL_SIMT = 1 << 4,        /* keeps bf16 relative-position attention on the SIMT kernels */
  CFM_ATTN_MODE_REL_ZERO_FILL = 1 << 6,   /* keeps the rel-pos kernels' zero-filling tile loads; one forward row block */
  CFM_ATTN_MODE_REL_DPOS_R4 = 1 << 7,     /* keeps the round-4 rel-pos dpos kernel */
  CFM_ATTN_MODE_REL_DQ_RECOMPUTE = 1 << 9, /* keeps the recomputing rel-pos dQ2 kernel (default: dQ from the stored dS) */
  CFM_ATTN_MODE_DQ_RECOMPUTE = 1 << 10,   /* keeps the recomputing whole-head dQ kernel (default: the stored dS) */
  CFM_ATTN_MODE_DKDV_TWO_PASS = 1 << 11   /* keeps the two-pass whole-head dK/dV kernel (default: one sweep) */
};
int cfm_attn_set_mode(int mode);

/* What the attention entry points below launch and how the backward workspace is laid out, as a pure host function
   (csrc/attn_plan.h): cfm_attn_fwd, cfm_attn_bwd_ws_bytes, cfm_attn_bwd and cfm_attn_bwd_ex act on this one rule. */
enum cfm_attn_path {
  CFM_ATTN_PATH_SIMT = 0,                 /* fp32, bf16 heads wider than 64, bf16 rel-pos under CFM_ATTN_MODE_REL_SIMT */
  CFM_ATTN_PATH_HEAD = 1,                 /* bf16 MFMA, one (or qs) workgroups per (b, h): T <= 384 */
  CFM_ATTN_PATH_TILED = 2,                /* bf16 MFMA, 128 queries per workgroup: T > 384 or CFM_ATTN_MODE_TILED */
  CFM_ATTN_PATH_REL = 3                   /* bf16 MFMA relative-position kernels */
};
enum cfm_attn_dpos {
  CFM_ATTN_DPOS_NONE = 0,                 /* not the rel-pos MFMA path */
  CFM_ATTN_DPOS_XCD = 1,                  /* 128 relative rows per workgroup, (b, h) pairs dealt to XCDs (rel_vec only) */
  CFM_ATTN_DPOS_R4_VEC = 2,               /* round-4 kernel, branch-free loads (CFM_ATTN_MODE_REL_DPOS_R4) */
  CFM_ATTN_DPOS_R4 = 3                    /* round-4 kernel, zero-filling loads (rel_vec off) */
};
enum cfm_attn_ws {                        /* sections of the backward workspace, in address order */
  CFM_ATTN_WS_D = 0,                      /* D = rowsum(dO * O): B*H*T f32 (MFMA paths) */
  CFM_ATTN_WS_PART = 1,                   /* rel: du / dv partials, B * 4*ceil(T/128) * 2*H*dk f32 */
  CFM_ATTN_WS_DS = 2,                     /* head: dS^T, B*H*Tq*Tq bf16 (Tq = ceil(T/32)*32), only when dQ reads it;
                                             rel: dS, B*H*T*ldS bf16 (ldS = ceil(T/8)*8); SIMT: dS, B*H*T*T f32 */
  CFM_ATTN_WS_DPOS = 3                    /* rel: per-utterance dpos partials, B*(2T-1)*H*dk f32 */
};
typedef struct {
  int B, T, H, dk, dtype;
  int rel;                                /* nonzero: relative positions */
  int qkv_mod16, dout_mod16, pos_mod16;   /* the pointers' addresses modulo 16 (forward: dout_mod16 = qkv_mod16;
                                             no rel-pos: pos_mod16 = 0) */
  int mode;                               /* cfm_attn_mode bits */
  int cus;                                /* compute units of the device */
  int64_t ws_bytes;                       /* backward workspace offered; < 0: unknown, report the full need */
} cfm_attn_query;
typedef struct {
  int path;                               /* cfm_attn_path */
  int vec, vec4;                          /* 16-byte / 8-byte loads of qkv and dout rows (vec4: non-rel MFMA only) */
  int pvec, rel_vec;                      /* rel: 16-byte loads of pos; the branch-free prefetch kernels run */
  int dbg;                                /* the timing bits of mode the non-rel MFMA kernels read */
  int qs, waves;                          /* head: workgroups per (b, h), 32-row blocks (waves) per workgroup */
  int dq_stored;                          /* head, rel: dQ from the dS the dK/dV kernel stores (0: recomputed) */
  int dpos;                               /* cfm_attn_dpos */
  size_t lds_head, lds_dkdv, lds_dqs;     /* head: dynamic LDS of the forward / recomputing dQ, dK/dV, dQ-from-dS */
  size_t ws_off[4], ws_size[4];           /* byte offset and size per cfm_attn_ws section (size 0: absent); every
                                             offset is a multiple of 256 */
  size_t ws_total;                        /* end of the last section = cfm_attn_bwd_ws_bytes */
} cfm_attn_choice;
/* Calls no GPU API.  CFM_ERR_ARG for a null pointer, cus <= 0 or ws_bytes >= 0 below ws_total of the chosen layout;
   the shape / dtype errors of cfm_attn_fwd otherwise.  On the whole-head path a ws_bytes that holds D (B*H*T floats)
   but not dS^T behind it selects the recomputing dQ kernel, as CFM_ATTN_MODE_DQ_RECOMPUTE does. */
int cfm_attn_plan(const cfm_attn_query* q, cfm_attn_choice* out);

int cfm_attn_fwd(const void* qkv, void* o, float* lse, const int32_t* lengths, const void* pos,
                 const float* pos_u, const float* pos_v, int B, int T, int H, int dk, int dtype,
                 float drop_p, uint64_t seed, void* stream);
/* The plan's ws_total under the mode in force (0 for a shape the plan rejects). */
size_t cfm_attn_bwd_ws_bytes(int B, int T, int H, int dk, int rel, int dtype);
/* ws_bytes: the size of ws.  The launcher lays ws out by the plan for that size under the mode in force at the
   call, so it never writes past ws_bytes: less than the path's minimum (non-rel MFMA: B*H*T floats; rel-pos: the
   whole rel layout; SIMT: B*H*T*T floats) is CFM_ERR_ARG and nothing is launched.  On the non-rel whole-head path
   (T <= 384) a ws that also holds dS^T (cfm_attn_bwd_ws_bytes under mode 0) makes dQ come from the dS^T the dK/dV
   kernel stores; a smaller one runs the recomputing dQ kernel.  dpos is fp32 and D is computed. */
int cfm_attn_bwd(const void* qkv, const void* o, const void* dout, const float* lse,
                 const int32_t* lengths, const void* pos, const float* pos_u, const float* pos_v,
                 void* dqkv, float* dpos, float* dpos_u, float* dpos_v, int B, int T, int H,
                 int dk, int dtype, float drop_p, uint64_t seed, float* ws, size_t ws_bytes, void* stream);
/* cfm_attn_bwd with the projected-table gradient dpos written in dtype_dpos: CFM_F32, or CFM_BF16 on the rel-pos
   MFMA path (each fp32 column sum rounded as cfm_cast rounds it -- the compute-dtype copy the dW_pos GEMM reads,
   without an fp32 dpos and a cast pass).  d_ready 1: D = rowsum(dO * O) is already in the first B*H*T floats of ws
   (cfm_gemm_desc.rowdot_* of the GEMM that produced dout) and the D kernel is skipped; bf16 MFMA paths only.
   d_ready 0: D is computed. */
int cfm_attn_bwd_ex(const void* qkv, const void* o, const void* dout, const float* lse,
                    const int32_t* lengths, const void* pos, const float* pos_u, const float* pos_v,
                    void* dqkv, void* dpos, int dtype_dpos, float* dpos_u, float* dpos_v, int B, int T,
                    int H, int dk, int dtype, float drop_p, uint64_t seed, int d_ready, float* ws,
                    size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- ConvSubSampling
 * lib/convsubsampling.py:16-45: Conv2d(1->C1, 7x7, s2) -> Conv2d(C1->C2, 3x3, s2), no padding.
 * conv1: x (B, F, T) fp32 -> h1 NHWC (B, F1, T1, C1) dtype_h; w1 (C1, 49), b1 (C1).
 * conv2: implicit GEMM over h1 -> h2 (B, T2, F2, C2) "frame-major" (row = (b,t2), features
 *        (f2, c2)) so the frame projection reads it as a plain (B*T2, F2*C2) matrix.
 *        w2r: (C2, 3*3*C1) reordered [c2][kh][kw][c1], dtype of h1. */
int cfm_conv1_fwd(const float* x, const float* w1, const float* b1, void* h1, int dtype_h, int B,
                  int F, int T, int C1, void* stream);
int cfm_conv2_fwd(const void* h1, const void* w2r, const float* b2, void* h2, int dtype_h2,
                  int dtype, int B, int F1, int T1, int C1, int C2, void* stream);
/* grads: dh1 from dh2 (transposed conv), dw2r (=), db2 via cfm_colsum; dw1 (=) and db1 (=). */
int cfm_conv2_bwd_data(const void* dh2, const void* w2r, void* dh1, int dtype, int B, int F1,
                       int T1, int C1, int C2, void* stream);
/* The same on the LDS-DMA GEMM pipeline: `ws` (cfm_conv2_bwd_data_ws_bytes) receives the per-parity-
   class K-major packing of w2r; NULL ws (or fp32) falls back to cfm_conv2_bwd_data. */
size_t cfm_conv2_bwd_data_ws_bytes(int C1, int C2);
int cfm_conv2_bwd_data_ws(const void* dh2, const void* w2r, void* dh1, int dtype, int B, int F1,
                          int T1, int C1, int C2, void* ws, void* stream);
int cfm_conv2_bwd_weight(const void* dh2, const void* h1, float* dw2r, int dtype, int B, int F1,
                         int T1, int C1, int C2, void* stream);
/* conv2 weight gradient with deterministic split-K slabs in `ws` (cfm_conv2_bwd_weight_ws_bytes bytes; NULL ->
 * one K slice): no atomics, no memset (graph-replay safe).  Replaces Conv2d.backward's weight gradient of
 * lib/convsubsampling.py:37. */
size_t cfm_conv2_bwd_weight_ws_bytes(int B, int F1, int T1, int C1, int C2);
int cfm_conv2_bwd_weight_ws(const void* dh2, const void* h1, float* dw2r, int dtype, int B, int F1,
                            int T1, int C1, int C2, float* ws, void* stream);
size_t cfm_conv1_bwd_ws_bytes(int B, int F, int T, int C1);
int cfm_conv1_bwd_weight(const void* dh1, int dtype_h, const float* x, float* dw1, float* db1,
                         int B, int F, int T, int C1, float* ws, void* stream);

/* ---------------------------------------------------------------- folded front-end ('frame' projection)
 * ConvSubSampling is two biased Conv2d with NO nonlinearity between them (lib/convsubsampling.py:41-43),
 * and in the 'frame' projection mode it feeds the per-frame Linear (the standard_linear of
 * asrnn.py:28,208 applied to every subsampled frame) before any dropout: the three are ONE linear map
 * of an Ke x Ke window of the mels, Ke = k1 + (k2 - 1) s1 (11), stride Se = s1 s2 (4):
 *   h[b, t2, o] = bfull[o] + sum_{f < Ke, r < F} Wfull[o][f][r] x[b, r, Se t2 + f]
 *   W_eff[c2][e][f] = sum_{c1, a, b} W2[c2][c1][a][b] W1[c1][e - s1 a][f - s1 b]       (the 11x11 conv)
 *   Wfull[o][f][r]  = sum_{f2, c2} Wp[o][f2 C2 + c2] W_eff[c2][r - Se f2][f]
 * so the step computes a (B*T2) x D x (Ke F) GEMM instead of conv1 -> conv2 -> Linear (~280 GFLOP
 * forward at Conformer-L / 15 s; the folded GEMM is 22 GFLOP with the hi + lo bf16 split of x).  The
 * GEMM reads x through a strided view: the packed input xt holds each utterance's frames as rows of Cx
 * channels (time-major; bf16 hi then lo rows of Fp, or fp32), row t2 of the view starts at frame Se t2
 * and spans Ke frames (lda = Se Cx < K: overlapping rows).  Utterance slots are Tslot = Se T2p frames
 * (T2p = T2 + padding rows), so the weight-gradient GEMM H = G^T X over all B*T2p padded rows (G zero
 * on the padding rows) is one single-stride product; the parameter gradients then follow from
 * H (D x Kp) and S = sum_rows G by the transposed contractions (cfm_ffold_bwd_weights).
 * Replaces Conv2d.forward/backward x2 and nn.Linear.forward/backward of that sequence. */
typedef struct {
  int B, F, T;        /* mels (B, F, T) fp32 */
  int C1, C2, D;      /* conv1 / conv2 channels, projection width */
  int k1, s1, k2, s2; /* square kernels, the same stride on both axes (nn.Conv2d, no padding) */
  int dtype;          /* GEMM operand type: CFM_BF16 or CFM_F32 */
  int hilo;           /* bf16: 1 = x as hi + lo bf16 rows (K doubles, ~16-bit x), 0 = hi only */
  /* filled by cfm_ffold_geometry: */
  int F2, T2, Ke, Se, Fp, Cx, Kp, lda, T2p, Tslot;
  long xt_elems;      /* elements of the packed input (B * Tslot * Cx + tail slack) */
  long ws_floats;     /* floats of the composed-weight workspace */
} cfm_ffold_geo;
int cfm_ffold_geometry(cfm_ffold_geo* g);
/* x (B, F, T) fp32 -> xt (xt_elems, dtype): frame t of utterance b at row b*Tslot + t (zero past T). */
int cfm_ffold_pack(const float* x, void* xt, const cfm_ffold_geo* g, void* stream);
/* w1 (C1, 1, k1, k1), b1 (C1), w2 (C2, C1, k2, k2), b2 (C2), wp (D, F2*C2) (features (f2, c2)), bp (D)
 * -> wfull (D, Kp) dtype (columns f*Cx + h*Fp + r, zero past Ke*Cx), bfull (D) fp32; ws (ws_floats) keeps
 * W_eff / b_eff for the backward. */
int cfm_ffold_compose(const float* w1, const float* b1, const float* w2, const float* b2, const float* wp,
                      const float* bp, void* wfull, float* bfull, float* ws, const cfm_ffold_geo* g,
                      void* stream);
/* H (D, Kp) fp32 = G^T X over the padded rows, S (D) = column sums of G (G: the gradient of h after the
 * dropout backward) -> dw1, db1, dw2, db2, dwp (same shapes as the weights; fp32, overwritten).  dbp = S. */
int cfm_ffold_bwd_weights(const float* H, const float* S, const float* w1, const float* b1, const float* w2,
                          const float* wp, float* ws, float* dw1, float* db1, float* dw2, float* db2, float* dwp,
                          const cfm_ffold_geo* g, void* stream);

/* ---------------------------------------------------------------- Adafactor (runner.py:36)
 * transformers.Adafactor as one multi-tensor step over a device-side parameter table.  A parameter
 * is nb matrices of R x C (col == NULL, factored == 0: a 1-D tensor, its full second moment in
 * `row`).  cfm_adafactor_plan is the one rule of what each parameter adds to each launch (host
 * arithmetic on the geometry, never the pointers).  cfm_adafactor_fill_table writes all n entries
 * of a host buffer of cfm_adafactor_table_bytes(n) through it; the totals size the buffers and go
 * to cfm_adafactor_step with the device copy of the table. */
typedef struct { float* p; const float* g; float* m; float* row; float* col;
                 long numel; int nb, R, C, factored; } cfm_adafactor_param;
typedef struct {
  long row_tasks, cols, blocks;         /* ada_rows waves, ada_cols threads, blocks of 4096 elements */
  long rowmean_tasks, colpart_tasks;    /* ada_rowmean waves, ada_colpart blocks (C in 64..2560) */
  long rowmean_floats, part_floats;     /* floats of rowmean and of part (may be NULL when 0) */
} cfm_adafactor_totals;
/* partial: blocks floats, per-block u^2 sums (RMS summed in block order, deterministic);
 * partial_p: the same of p^2, and rms_out: n floats, both SCALE_PARAMETER only. */
typedef struct { float *rowmean, *part, *partial, *partial_p, *rms_out; } cfm_adafactor_buffers;
size_t cfm_adafactor_table_bytes(int n_params);
/* before (may be NULL): n entries, the totals in front of each parameter = its offsets in the table */
int cfm_adafactor_plan(const cfm_adafactor_param* params, int n, cfm_adafactor_totals* before,
                       cfm_adafactor_totals* totals);
int cfm_adafactor_fill_table(void* host_table, const cfm_adafactor_param* params, int n,
                             cfm_adafactor_totals* totals);
/* The step; the kernel variants it launches are a function of the hyper-parameters alone.  Per tensor
 *   lr_p = rel * (SCALE_PARAMETER ? max(eps2, RMS(p)) : 1),   RMS(p) = ||p|| / sqrt(numel) of p
 *          before this step (written to rms_out[i], i = table index; per-block sums of p^2 in
 *          partial_p, summed in block order as `partial` is),
 *   p += -weight_decay * lr_p * p  before  p -= update.
 * Without DEVICE_STEP rel = lr and beta2t is the field (the host has resolved a relative step
 * already; RELATIVE_STEP / WARMUP_INIT are not read).  With DEVICE_STEP
 * one extra launch increments *step_dev (int32) and writes scalars_dev[0] = beta2t =
 * 1 - step^decay_rate and scalars_dev[1] = rel = RELATIVE_STEP ? min(WARMUP_INIT ? 1e-6 step :
 * 1e-2, 1/sqrt(step)) : lr (both computed in double, rounded once), which the other kernels read:
 * no host value depends on the step, so one captured launch sequence replays as successive steps.
 * flags == 0 and weight_decay == 0 launch the six kernels of the reference's configuration. */
enum cfm_adafactor_flags {
  CFM_ADA_SCALE_PARAMETER = 1 << 0,
  CFM_ADA_RELATIVE_STEP = 1 << 1,
  CFM_ADA_WARMUP_INIT = 1 << 2,
  CFM_ADA_DEVICE_STEP = 1 << 3
};
typedef struct {
  double decay_rate;   /* DEVICE_STEP only */
  float lr, beta1, beta2t, eps1, eps2, clip, weight_decay;
  int flags;           /* cfm_adafactor_flags */
  int* step_dev;       /* DEVICE_STEP: one int32, incremented by the call */
  float* scalars_dev;  /* DEVICE_STEP: 2 floats */
} cfm_adafactor_hyper;
int cfm_adafactor_step(const void* dev_table, int n, const cfm_adafactor_totals* totals,
                       const cfm_adafactor_buffers* buffers, const cfm_adafactor_hyper* hyper, void* stream);

/* ---------------------------------------------------------------- CTC head (runner.py:35,142-143)
 * Replaces torch.nn.CTCLoss(blank=hp.blank_idx, zero_infinity=True) on
 * log_softmax(final_fc(...)) (asrnn.py:45,256): log-softmax, alpha/beta recursions and the
 * gradient w.r.t. the logits, without host synchronisation (graph-capturable).
 * logits fp32, row (b, t) at logits + b*sb + t*st, classes contiguous (sb/st cover both the
 * reference's time-major (T, B, V) and batch-major layouts).  Feeding log-probabilities instead
 * of logits gives torch's result too (log_softmax is idempotent; the gradient is then exactly
 * torch's grad w.r.t. log_probs).  targets int32: utterance b at targets + tgt_off[b] (tgt_off
 * != NULL: torch's concatenated 1-D form) or targets + b*ldt (padded (B, ldt)); Smax >= every
 * target length.  in_len / tgt_len int32 on the device.
 * fwd: nll[b] = -log p(target_b | x_b), 0 where infinite and zero_infinity (torch semantics);
 *      ws: cfm_ctc_ws_bytes(B, T, Smax) bytes, read again by the backward.
 * bwd: grad[b, t, v] = (softmax - posterior) * grad_out[b * grad_out_stride] * r_b with
 *      r_b = 1 / (B * max(L_b, 1)) for reduction 1 (mean), 1 for 0 (none) / 2 (sum); zero for
 *      t >= in_len[b] and for zeroed infinite losses.  Output layout gsb/gst, dtype_grad f32|bf16.
 *      The backward checks B, T, V, Smax, ldt and blank as the forward does (same codes, its own name in the
 *      message): it rejects only calls whose forward, which fills the workspace it reads, was rejected too. */
size_t cfm_ctc_ws_bytes(int B, int T, int Smax);
int cfm_ctc_loss_fwd(const float* logits, long sb, long st, const int32_t* targets, int ldt,
                     const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int B,
                     int T, int V, int Smax, int blank, int zero_infinity, float* nll, float* ws,
                     void* stream);
int cfm_ctc_loss_bwd(const float* logits, long sb, long st, const int32_t* targets, int ldt,
                     const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int B,
                     int T, int V, int Smax, int blank, int zero_infinity, const float* ws,
                     const float* grad_out, int grad_out_stride, int reduction, void* grad_logits,
                     int dtype_grad, long gsb, long gst, void* stream);

/* reduction='mean' of the forward's nll (torch.nn.CTCLoss: mean over b of nll[b] / max(tgt_len[b], 1)) as
 * ONE launch: *loss (fp32 scalar).  nonfinite (nullable): incremented by 1 when the mean is not finite (a
 * device step counter of bad steps, read once after a run).  Replaces the four element-wise passes of the
 * reduction and the host-side finiteness check's seven. */
int cfm_ctc_mean(const float* nll, const int32_t* tgt_len, int B, float* loss, int32_t* nonfinite,
                 void* stream);

/* Alpha / beta recursion health (no reference counterpart: the device recursion's own guard).  Each of the
 * recursion's inter-wave waits is bounded; a wait that gives up marks its direction aborted and the forward then
 * makes that utterance's nll NaN (so the loss and the logits gradient are NaN, never silently wrong).
 * cfm_ctc_bind_abort_counter(counter): int32 device counter (NULL unbinds) incremented once per aborted
 * utterance by every later cfm_ctc_loss_fwd -- told apart from genuine non-finite losses.
 * cfm_ctc_set_debug(mask): test hook, forces the abort path of the alpha (bit 0) / beta (bit 1) recursion. */
int cfm_ctc_bind_abort_counter(int32_t* counter);
int cfm_ctc_set_debug(int force_abort_mask);

/* Greedy decode: ASRNN.predict (asrnn.py:48-58, torch.argmax over classes: first maximum,
 * NaN wins) -> ids (B, T) int64; optionally (out, out_len != NULL) the Vocab.decode id filter
 * (myvocab.py:211-231): frames t < lens[b] (lens NULL: all T), ids equal to `blank` or `pad`
 * dropped (pad < 0: none), repeats collapsed first if `collapse` (the reference does not);
 * out (B, T) int32 padded with -1, out_len (B) int32. */
int cfm_ctc_greedy_decode(const float* logits, long sb, long st, const int32_t* lens, int B, int T,
                          int V, int blank, int pad, int collapse, int64_t* ids, int32_t* out,
                          int32_t* out_len, void* stream);

/* CTC prefix beam search without a language model: the alternative to the argmax decode of ASRNN.predict
 * (asrnn.py:48-58) and of the Runner's metric and pseudo-label passes (runner.py:150,220,275), which follow one
 * alignment; the beam sums the alignments of each label prefix.  The surface is modelled on torchaudio's CUDA CTC
 * decoder.  logits fp32, row (b, t) at b*sb + t*st (logits or log-probabilities: log-softmax is applied); lens int32
 * on the device (nullable, clamped to [0, T], never read back); 1 <= nbest <= beam <= 128, 2 <= V <= 16384,
 * 0 <= blank < V, pad in [0, V) or < 0 for none (never emitted).  The `beam` prefixes of highest p_b (+) p_nb survive
 * each frame, in descending order; the first nbest after lens[b] frames are the hypotheses:
 *   tokens (B, nbest, T) int32 padded with -1, out_len (B, nbest), score (B, nbest) = log p_b (+) p_nb (natural log);
 *   lens[b] == 0: one empty hypothesis of score 0; missing hypotheses: length 0, score -inf.
 * bp_parent / bp_token (B, T, beam) int32, caller-allocated: slot s of frame t came from slot bp_parent of frame
 * t - 1 (frame 0: slot 0, the empty prefix) by appending bp_token (-1: prefix unchanged); bp_parent == -1: empty
 * slot; slots in descending score order; frames t >= lens[b] unspecified.  ws: cfm_ctc_beam_ws_bytes(B, T, beam).
 * Three launches, no host synchronisation (graph-capturable); results are bit-identical from run to run. */
size_t cfm_ctc_beam_ws_bytes(int B, int T, int W);
int cfm_ctc_beam_decode(const float* logits, long sb, long st, const int32_t* lens, int B, int T, int V,
                        int blank, int pad, int beam, int nbest, int32_t* bp_parent, int32_t* bp_token,
                        int32_t* tokens, int32_t* out_len, float* score, void* ws, void* stream);

/* The same search with a back-off n-gram language model (order <= 3) fused in at every extension: shallow fusion,
 * for the argmax call sites runner.py:150,220,275.  The reference names LM fusion only (runner.py:78-101: a
 * transformer LM whose weights are added under keys that match nothing, never realised); this is the n-gram form.
 *   extend  p_nb'(l+c) (+)= r[c] + alpha * lm(c | h(l)) + beta + (c == last(l) ? p_b(l) : (p_b (+) p_nb)(l))
 * with h(l) the last min(order - 1, |l| + 1) symbols of <s> + l (<s> = V, </s> = V + 1) and lm the natural-log
 * back-off probability; stays are unchanged, blank and pad are never scored.  Every live entry is extended by the
 * K = min(token_beam, #tokens) acoustically best tokens of the frame (raw fp32 logits, lower id first among equals),
 * merges are taken over all tokens; beam + beam * K <= 1024 and K <= 768 (CFM_ERR_UNSUPPORTED otherwise).  The beam
 * ranks on the fused score and `score` is the fused score; eos != 0 adds alpha * lm(</s> | h(l)) to the final scores
 * and orders the hypotheses by them (bp_* slots stay in the last frame's order); lens[b] == 0: one empty hypothesis
 * of score alpha * lm(</s> | <s>) (0 without eos).
 * cfm_ngram_lm (device pointers; nn_conformer_for_speech_recognition_amd/lm.py packs it): unigrams (V + 2) x {float
 * logp, float backoff}; table (mask + 1) x 16-byte slots {uint64 key, float logp, float backoff}, open-addressed,
 * mask + 1 a power of two, every key within `probe` <= 4 slots of its home
 *   z = (key ^ seed) * 0x9E3779B97F4A7C15; z = (z ^ z >> 32) * 0xBF58476D1CE4E5B9; home = (z ^ z >> 29) & mask;
 * key = n << 45 | a << 30 | b << 15 | c for the n-gram (a, b, c) (a bigram: a = 0), empty slots all ones.  Every
 * index the kernel forms from a hash, a table word or a token id is masked or clamped before use: a malformed table
 * gives wrong scores, never an out-of-range access.  ws: cfm_ctc_beam_lm_ws_bytes(B, T, beam, K).  Three launches,
 * no host synchronisation (graph-capturable), bit-identical from run to run; with alpha = beta = 0, no eos and
 * token_beam = beam + 1 the results are cfm_ctc_beam_decode's. */
typedef struct cfm_ngram_lm {
  const void* unigrams;
  const void* table;
  uint64_t seed;
  uint32_t mask;
  int probe;
  int order;
  int V;
} cfm_ngram_lm;
size_t cfm_ctc_beam_lm_ws_bytes(int B, int T, int W, int K);
int cfm_ctc_beam_decode_lm(const float* logits, long sb, long st, const int32_t* lens, int B, int T, int V,
                           int blank, int pad, int beam, int nbest, int token_beam, float alpha, float beta, int eos,
                           const cfm_ngram_lm* lm, int32_t* bp_parent, int32_t* bp_token, int32_t* tokens,
                           int32_t* out_len, float* score, void* ws, void* stream);

/* CTC forced alignment: the best single alignment (Viterbi path) of a GIVEN transcript, where the loss sums all of
 * them and the decoders search for the transcript.  The reference has no counterpart; the surface is modelled on
 * torchaudio.functional.forced_align, batched and with per-token spans.  logits, sb / st, targets / ldt / tgt_off,
 * in_len, tgt_len, Smax and blank as cfm_ctc_loss_fwd (logits or log-probabilities: log-softmax is applied; lengths
 * and labels are device data, clamped, never read back; 2 * Smax + 1 <= 1024, CFM_ERR_UNSUPPORTED above 511 labels;
 * targets may be NULL when Smax == 0).  Over the states blank, l1, blank, l2, ..., blank (S_b = 2 L_b + 1):
 *   v[t, s] = lpe[t, s] + max(v[t-1, s], v[t-1, s-1], v[t-1, s-2] if s is a label other than label s-2),
 *   v[0, 0] = lpe[0, 0], v[0, 1] = lpe[0, 1];  equal predecessors prefer stay, then s-1, then s-2, and at the last
 *   frame the final blank S_b - 1 wins a tie against S_b - 2 (the tie rule is part of the contract).
 * Outputs, caller-allocated:
 *   alignments (B, T) int32  the label (blank included) of each frame t < in_len[b]; -1 beyond
 *   scores (B, T) fp32       its log-probability; 0 beyond
 *   score (B) fp32           the path's log-probability (natural log)
 *   starts, ends (B, Smax) int32, token_scores (B, Smax) fp32 (all three or none, NULL): per target position
 *     u < L_b the first frame of its label, one past the last, and the sum of `scores` over the span in frame order
 *     (one thread, no atomics); -1 / -1 / 0 for u >= L_b.
 * An utterance with in_len[b] < L_b + (adjacent equal labels) has no alignment (so has in_len 0 with L_b > 0, and
 * a best path whose score is not finite): score -inf, alignments -1, scores 0, spans -1 / -1 / 0.  in_len 0 with
 * L_b 0: score 0.  L_b 0: every frame blank.  ws: cfm_ctc_align_ws_bytes(B, T, Smax).  Three launches (emissions,
 * recursion, backtrace), no host synchronisation (graph-capturable), no wait on another wave's progress anywhere;
 * results are bit-identical from run to run. */
size_t cfm_ctc_align_ws_bytes(int B, int T, int Smax);
int cfm_ctc_forced_align(const float* logits, long sb, long st, const int32_t* targets, int ldt,
                         const int32_t* tgt_off, const int32_t* in_len, const int32_t* tgt_len, int B, int T, int V,
                         int Smax, int blank, int32_t* alignments, float* scores, float* score, int32_t* starts,
                         int32_t* ends, float* token_scores, void* ws, void* stream);

/* CTC likelihood of an n-best list and the expected risk over it (MWER training, Prabhavalkar et al. 2018; n-best
 * rescoring): N hypotheses per utterance against the utterance's ONE emission matrix.  The reference has no
 * counterpart.  logits, sb / st, in_len, blank as cfm_ctc_loss_fwd (logits or log-probabilities: log-softmax is
 * applied).  J = B * N problems, problem j = b * N + n: hypothesis row hyp + j * ldh (int32 ids), hyp_len[j] labels;
 * hyp_len[j] < 0: the hypothesis is missing; hyp_len[j] > max_labels: it is left out the same way.  Lengths and ids
 * are device data, clamped, never read back.  1 <= N <= 128 (CFM_ERR_ARG below, CFM_ERR_UNSUPPORTED above),
 * max_labels <= min(ldh, 511) (CFM_ERR_SHAPE / CFM_ERR_UNSUPPORTED); hyp may be NULL when max_labels == 0.
 *   ll (J) fp32     log P_ctc(y_j | x_b), natural log, over all alignments; -inf for an infeasible hypothesis
 *                   (in_len[b] < L + adjacent equal labels, so also in_len 0 with L > 0), a result that is not finite,
 *                   and a missing or over-long hypothesis; in_len 0 with L 0: 0
 *   live            ll finite (hence present and within max_labels)
 *   post (J) fp32   softmax of ll over the live n of the utterance; 0 elsewhere
 *   loss (B) fp32   sum_n post * (risk - rbar), rbar the plain mean of risk (J, fp32) over the live n; 0 with fewer
 *                   than two live hypotheses.  risk and loss: both or neither (NULL: ll and post only)
 *   c = post * ((risk - rbar) - loss), sum_n c = 0; equal risks give c == 0 exactly (rbar is formed in double)
 * cfm_ctc_nbest_bwd after cfm_ctc_nbest_fwd with risk, same arguments and the same ws untouched in between:
 *   grad_logits[b, t, v] (fp32, row (b, t) at b*gsb + t*gst, every row written whole)
 *     = grad_loss[b * grad_stride] * sum_n c[b, n] * occ_n[t, v]   for t < in_len[b]
 * with occ_n[t, v] the posterior probability that hypothesis n's alignment emits class v at frame t
 * (exp(alpha + beta - lpe - ll) summed over the states of class v).  d ll / d logits = occ - softmax(logits); the
 * softmax term is multiplied by sum_n c = 0 and is never formed.  Exactly 0: frames t >= in_len[b], classes that are
 * neither the blank nor a label of a hypothesis with c != 0, utterances with fewer than two live hypotheses or equal
 * risks.  grad_stride 1, or 0 for one scalar.
 * The recursions keep alpha, beta and ll in double and take their exponentials and logarithms in fp32 on O(1)
 * differences, so a frame's error does not grow with |log p| (csrc/ctc_nbest.hip, "Precision").
 * ws: cfm_ctc_nbest_ws_bytes(B, T, N, max_labels), 8-byte aligned (CFM_ERR_ALIGN): per (j, t, state) one double of
 * alpha and one float that holds the emission after the forward and the occupancy after the backward, J * T *
 * (2 max_labels + 1) cells in all.  Forward: three launches (emissions with the row statistics once per (b, t) row, alpha, weights); backward:
 * two (beta / occupancy, gradient rows).  No host synchronisation (graph-capturable), no wait on another wave's
 * progress anywhere, no floating-point atomics: every sum runs in an order fixed by the inputs (n order, then state
 * order), so results are bit-identical from run to run. */
size_t cfm_ctc_nbest_ws_bytes(int B, int T, int N, int max_labels);
int cfm_ctc_nbest_fwd(const float* logits, long sb, long st, const int32_t* in_len, int B, int T, int V,
                      const int32_t* hyp, int ldh, const int32_t* hyp_len, int N, int max_labels, int blank,
                      const float* risk, float* ll, float* post, float* loss, void* ws, void* stream);
int cfm_ctc_nbest_bwd(const float* logits, long sb, long st, const int32_t* in_len, int B, int T, int V,
                      const int32_t* hyp, int ldh, const int32_t* hyp_len, int N, int max_labels, int blank, void* ws,
                      const float* grad_loss, int grad_stride, float* grad_logits, long gsb, long gst, void* stream);

/* RNN-T (transducer) loss over a dense lattice of joint logits, and its gradient (Graves 2012; the interface of
 * torchaudio.functional.rnnt_loss).  The reference has no counterpart.  logits (B, T, U1, V) fp32, dense, U1 = Umax + 1
 * (log-softmax over V is applied); targets int32, row b at targets + b * ldt, ldt >= U1 - 1, holding no blanks
 * (NULL allowed when U1 == 1); in_len, tgt_len (B) int32 on the device, clamped there to [0, T] and [0, U1 - 1], the
 * labels to [0, V - 1], never read back: a bad value can give a wrong answer, never an access outside a buffer.
 * With T_b, U_b the clamped lengths, lp = log_softmax(logits), b(t,u) = lp[t,u,blank], y(t,u) = lp[t,u,label_{u+1}]:
 *   alpha(0,0) = 0;  alpha(t,u) = lse(alpha(t-1,u) + b(t-1,u), alpha(t,u-1) + y(t,u-1))
 *   beta(T_b-1,U_b) = b(T_b-1,U_b);  beta(t,u) = lse(beta(t+1,u) + b(t,u), beta(t,u+1) + y(t,u))
 *   ll[b] = alpha(T_b-1,U_b) + b(T_b-1,U_b) (= beta(0,0)), natural log; the loss is -ll[b]
 *   ll[b] = -inf when T_b == 0 (the utterance takes no part) or when the value is not finite
 * cfm_rnnt_loss_bwd after cfm_rnnt_loss_fwd, same arguments and the same ws untouched in between; with
 * gamma(t,u) = exp(alpha + beta - ll), for the valid cells t < T_b, u <= U_b:
 *   dlogits[b,t,u,v] = grad_loss[b] * ( softmax(logits)[b,t,u,v] * gamma(t,u)
 *                      - [v == blank] exp(alpha(t,u) + b(t,u) + beta(t+1,u) - ll)      (at (T_b-1, U_b): gamma)
 *                      - [v == label_{u+1}, u < U_b] exp(alpha(t,u) + y(t,u) + beta(t,u+1) - ll) )
 * the gradient of sum_b grad_loss[b] * (-ll[b]).  Every valid row of it sums to 0 over v (beta(t,u) is the log-sum of
 * the two subtracted exponents).  Outside the valid cells, and for an utterance with ll = -inf, the rows are exact
 * zeros: the whole dlogits buffer is written, and the logits outside the valid cells are never read.
 * alpha, beta and ll are double with fp32 exp / log on O(1) differences (csrc/ctc_nbest.hip, "Precision").
 * B, T, U1, V > 0 and ldt >= U1 - 1 (CFM_ERR_SHAPE); non-null pointers and 0 <= blank < V (CFM_ERR_ARG); U1 <= 1024,
 * V >= 2 and B * T * U1 < 2^31 (CFM_ERR_UNSUPPORTED); ws: cfm_rnnt_ws_bytes(B, T, U1) bytes, 8-byte aligned
 * (CFM_ERR_ALIGN): per cell of the (T + U1 - 1) x U1 diagonal-major lattice two doubles (alpha, beta) and two floats
 * (b, y), plus a float per logits row.  Forward: two launches (emissions: the only pass over the logits; alpha and
 * beta side by side, the alpha block writing ll); backward: one.  No host synchronisation
 * (graph-capturable), no wait on another wave's progress, no atomics: results are bit-identical from run to run. */
size_t cfm_rnnt_ws_bytes(int B, int T, int U1);
int cfm_rnnt_loss_fwd(const float* logits, const int32_t* targets, int ldt, const int32_t* in_len,
                      const int32_t* tgt_len, int B, int T, int U1, int V, int blank, float* ll, void* ws,
                      void* stream);
int cfm_rnnt_loss_bwd(const float* logits, const int32_t* targets, int ldt, const int32_t* in_len,
                      const int32_t* tgt_len, int B, int T, int U1, int V, int blank, const void* ws,
                      const float* grad_loss, float* dlogits, void* stream);

/* Time-synchronous greedy search of a transducer head (transducer.TransducerHead), one launch, one workgroup per
 * utterance (csrc/rnnt_greedy.hip).  The reference has no counterpart.  All fp32, contiguous: ep (B, T, J) =
 * enc_proj(enc) with bias; gtab (V, 4H) = embedding.weight W_ih^T + b_ih + b_hh (the LSTM cell's input half of token
 * v is row v); w_hh (4H, H); w_pp (J, H), b_pp (J): pred_proj; w_out (V, J), b_out (V): out.  lengths (B) int32 on the
 * device, clamped there to [0, T] and never read back, or NULL (T).  Per utterance, T_b the clamped length:
 *   (h, c) = cell(0, 0, gtab[blank]);  pp = w_pp h + b_pp
 *   for t < T_b, at most max_symbols times:
 *     logits = w_out tanh(ep[b,t] + pp) + b_out;  tok = argmax, ties to the LOWEST index (torch's rule)
 *     scores[b] += log_softmax(logits)[tok], formed as (x - m) - log sum exp(x - m), accumulated in double
 *     tok == blank: the frame is closed.  Otherwise tok is emitted at frame t (an utterance that has emitted W
 *     tokens stops there), (h, c) = cell(h, c, gtab[tok]) -- gates = gtab[tok] + w_hh h, order i, f, g, o,
 *     c = sigmoid(f) c + sigmoid(i) tanh(g), h = sigmoid(o) tanh(c) -- and pp is recomputed.
 * A frame closed by the max_symbols cap adds no blank term to the score.
 * Outputs, every element written: tokens (B, W) and frames (B, W) int32 padded with -1 (frames: the frame each token
 * was emitted at), counts (B) int32, scores (B) fp32.
 * A logit's operation order depends on neither its row nor the utterance's place in the batch: identical rows of w_out
 * with identical biases give bit-equal logits.  No communication between workgroups, no atomics, no spin; trip counts
 * are bounded by T_b * max_symbols; no host synchronisation (graph-capturable); results are bit-identical from run to
 * run.  B, T, V, H, J, W > 0 (CFM_ERR_SHAPE); non-null pointers (lengths excepted), 0 <= blank < V and
 * max_symbols >= 1 (CFM_ERR_ARG); V >= 2, H <= 1024 with H % 8 == 0, J <= 1024 (CFM_ERR_UNSUPPORTED): no launch. */
int cfm_rnnt_greedy(const float* ep, const float* gtab, const float* w_hh, const float* w_pp, const float* b_pp,
                    const float* w_out, const float* b_out, const int32_t* lengths, int B, int T, int V, int H, int J,
                    int blank, int max_symbols, int W, int32_t* tokens, int32_t* frames, int32_t* counts,
                    float* scores, void* stream);

/* Batched edit distance (Levenshtein) over token ids: the numerator of the word error rate -- the vocabulary's tokens
 * are words -- in place of the host loop of jiwer's wer (reference runner.py:160,230), and the aligned pairs the
 * reference's confusion matrix is built from (evals.py:64).  Pair p < P compares hypothesis row p (hyp + p * ldh,
 * hyp_len[p] ids) with reference row p / group (ref + (p / group) * ldr, ref_len[p / group] ids); P == n_ref * group,
 * group = N scores an n-best list against one transcript.  Lengths are device data, clamped on the device to
 * [0, Rmax] and [0, Hmax] and never read back; ids past a row's length are never read into a result.
 * Rmax <= ldr, Hmax <= ldh (CFM_ERR_SHAPE), both <= 1024 (CFM_ERR_UNSUPPORTED above); null, negative or
 * P != n_ref * group arguments return CFM_ERR_ARG before any launch (ref / hyp may be NULL when Rmax / Hmax is 0).
 * With r the reference (R ids) and h the hypothesis (H ids):
 *   D[i][0] = i, D[0][j] = j,
 *   D[i][j] = min(D[i-1][j-1] + (r[i-1] != h[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)   for i, j >= 1,
 *   dist[p] = D[R][H].
 * Tie rule of the alignment (part of the contract): a cell's direction is the FIRST of diagonal (hit or
 * substitution), up (deletion: a reference token without a partner), left (insertion) that attains the minimum;
 * on the border i == 0 walks left and j == 0 walks up; the backtrace starts at (R, H).  From that one path:
 *   counts (P, 4) int32 or NULL   hits, substitutions, deletions, insertions:
 *                                 hits + subs + dels = R, hits + subs + ins = H, subs + dels + ins = dist
 *   pair_ref, pair_hyp (P, ldp) int32 and n_pairs (P) int32 (all three or none, NULL), ldp >= Rmax + Hmax:
 *                                 the path's pairs in forward order, -1 on the gap side, n_pairs[p] <= R + H of
 *                                 them; entries past n_pairs[p] are -1 on both sides.
 * counts == NULL and no pair outputs (want_ops = 0): one launch, no direction matrix is stored and ws may be NULL /
 * 0 bytes (the training-metric path).  Otherwise ws holds the direction matrix, 2 bits per cell (16 anti-diagonal
 * steps of a row per 32-bit word, rows padded by the 63-step skew of a 64-row strip), and a backtrace launch follows
 * the recursion.  ws: cfm_edit_distance_ws_bytes(P, Rmax, Hmax, want_ops).  No host synchronisation
 * (graph-capturable), one wave per pair and no wait on another wave's progress anywhere; results are bit-identical
 * from run to run. */
size_t cfm_edit_distance_ws_bytes(int P, int Rmax, int Hmax, int want_ops);
int cfm_edit_distance(const int32_t* ref, int ldr, const int32_t* ref_len, int n_ref, const int32_t* hyp, int ldh,
                      const int32_t* hyp_len, int P, int group, int Rmax, int Hmax, int32_t* dist, int32_t* counts,
                      int32_t* pair_ref, int32_t* pair_hyp, int ldp, int32_t* n_pairs, void* ws, void* stream);

/* BiLSTM decoder recurrence: replaces the cuDNN/MIOpen recurrence of the
 * reference's nn.LSTM (asrnn.py:38 construct, :252 call on the 2-D encoder output = ONE unbatched
 * sequence of L = B*T_enc steps).  Gate order i, f, g, o (torch).  One cooperative launch per pass;
 * the input part x W_ih^T + b_ih + b_hh (gx) and the weight / input gradients are cfm_gemm calls.
 *   gx (L, ndir*4H) fp32, whh (ndir, 4H, H) fp32, y (L, ndir*H) = torch's output layout,
 *   gates (L, ndir*4H) post-activation, c (L, ndir*H) cell states (both saved for the backward),
 *   dg (L, ndir*4H) pre-activation gate gradients.  H % 8 == 0, H <= 1024, ndir 1 or 2.
 * ws: cfm_lstm_ws_bytes(H, ndir) of 16-B aligned device scratch (two error flags + the tagged-word
 * exchange rings; one workspace serves a forward and its backward): after a pass, ((int*)ws)[0] (fwd) /
 * ((int*)ws)[1] (bwd) != 0 means a step wait hit its 2-s limit. */
size_t cfm_lstm_ws_bytes(int H, int ndir);
int cfm_lstm_fwd(const float* gx, const float* whh, float* y, float* gates, float* c, int L, int H,
                 int ndir, void* ws, void* stream);
int cfm_lstm_bwd(const float* dy, const float* whh, const float* gates, const float* c, float* dg,
                 int L, int H, int ndir, void* ws, void* stream);

/* Batched LSTM recurrence (csrc/lstm_batched.hip): B independent sequences of up to T steps side by side, the
 * recurrence of nn.LSTM on a 3-D input with packed-sequence semantics.  Gate order, widths and limits are those of
 * cfm_lstm_fwd (H % 8 == 0, H <= 1024, ndir 1 or 2); any B >= 1 and T >= 1.
 *   Every per-step array has B*T rows, fp32: gx, gates, dg (., ndir*4H); y, c, hprev, dy (., ndir*H).  The row of
 *   (b, t) is b*stride_b + t*stride_t: batch-major (B, T, .) is stride_b = T, stride_t = 1; time-major (T, B, .) is
 *   stride_b = 1, stride_t = B (the strides must address exactly the B*T rows).
 *   whh (ndir, 4H, H) as for cfm_lstm_fwd; whh_t (ndir, H, 4H): each direction's W_hh transposed (the backward
 *   product then reads weight rows along its reduction, like the forward).  whh, whh_t, y and dg 16-B aligned.
 *   lengths (B) int32 on the device, or NULL for all T; each entry is clamped to [0, T] by the kernels and never
 *   read back.  Sequence b runs t = 0 .. len_b-1 (forward direction) and t = len_b-1 .. 0 (reverse direction: the
 *   packed sequence reversed, not the padded buffer), both from a zero state.
 *   hprev (may be NULL): the state that fed each step, h_{t-1} (forward half) / h_{t+1} (reverse half), 0 at a
 *   sequence's first step per direction -- the operand of the dW_hh GEMM, dW_hh[dir] = dg[:, dir]^T hprev[:, dir].
 * Padding positions (t >= len_b): y = 0, hprev = 0 and dg = 0 are stored, exactly, in both directions; gates and c
 * are left unwritten; gx, dy and the previous contents of any buffer are never read there (selects, no 0/1
 * multiplications), so nothing at a valid position depends on a padding value.  len_b = 0: all padding.
 * One plain kernel launch per time step, issued in a stream-ordered loop of T launches by the entry point, each
 * covering all B sequences and both directions: no cooperative launch and no wait on another workgroup, hence no
 * error flag to poll, and both calls are HIP-graph-capturable.  fp32 throughout, no atomics: two runs are
 * bit-identical, and a sequence's results do not depend on its index in the batch.
 * ws: cfm_lstm_batched_ws_bytes(B, T, H, ndir) bytes of device scratch for the backward, which carries the cell
 * gradient dc_{t+-1} f_{t+-1} per (b, unit) there between its launches (B*ndir*H floats, no initialisation needed);
 * the forward uses none (ws may be NULL). */
size_t cfm_lstm_batched_ws_bytes(int B, int T, int H, int ndir);
int cfm_lstm_batched_fwd(const float* gx, const float* whh, const int32_t* lengths, float* y, float* gates, float* c,
                         float* hprev, int B, int T, long stride_b, long stride_t, int H, int ndir, void* ws,
                         void* stream);
int cfm_lstm_batched_bwd(const float* dy, const float* whh_t, const float* gates, const float* c,
                         const int32_t* lengths, float* dg, int B, int T, long stride_b, long stride_t, int H,
                         int ndir, void* ws, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CFM_H */
