// Internal declarations shared by the translation units of libbot7hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "argbest.h"
#include "bot7hip.h"

// Tile constants.  Every matrix dimension that a GEMM-class kernel sees is padded to these.
constexpr int B7_NPAD = 128;  // observations padded to a multiple of this (post kernel's n-tile)
constexpr int B7_PANEL = 64;  // Cholesky panel width / small-GEMM tile
constexpr int B7_PERSIST_NMAX = 4096;  // largest padded N of the persistent Cholesky (64 panels: flag block, the vector job's LDS)
constexpr int B7_MROWS = 256; // chunk rows are multiples of this (largest candidates-per-block of any post variant)
constexpr int B7_MAX_D = 96;  // LDS budget of the covariance kernel: (64 + 2*32) rows x (dpad+1) doubles at dpad = 96

// The exchange table of a candidate-sharded nomination (comm.hip): one fixed-width record of 64-bit words per rank, so
// that ONE all-reduce carries the arg-max pair, the winner's grid row (what bots/abstract.lua:118-121 steals into
// `pending`), the shard's row count and a failure flag.  The width does not depend on the grid's dims: every rank issues
// the same collective whatever it holds (an empty shard has no grid to take dims from).
constexpr int B7_TAB_VAL = 0;     // bits of the local maximum
constexpr int B7_TAB_IDX = 1;     // its 1-based GLOBAL index; 0 = this shard is empty
constexpr int B7_TAB_STATUS = 2;  // 0 = fine; otherwise -(B7_ERR_*) of the rank that could not score its shard
constexpr int B7_TAB_ROWS = 3;    // candidate rows this shard holds
constexpr int B7_TAB_ROW0 = 4;    // d doubles: the grid row of the local maximum
constexpr int B7_TAB_W = B7_TAB_ROW0 + B7_MAX_D;
constexpr int B7_MAX_WORLD = 64;

// Padded input dimension of the feature kernels (rff.hip, ts_refine.hip), one instantiation per class
__host__ __device__ constexpr int rff_dpad(int d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 64 ? 64 : 96; }

// Padded input dimension: the covariance kernel is instantiated per class so its MFMA chain unrolls.
static inline int b7_dpad_class(int d) {
  return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : d <= 48 ? 48 : d <= 64 ? 64 : 96;
}

// Device result block of a fit: int info[4] | double nll_terms[1 + 256] | the persistent schedule's hand-off flags (up to
// nb = 32 panels), so that ONE memset ahead of a persistent launch zeroes info and flags together.
constexpr size_t B7_INFO_HEAD_BYTES = 16 + sizeof(double) * 257 + 8;                       // 2080: a multiple of 16
constexpr size_t B7_PERSIST_FLAG_WORDS_MAX = 16 + 2 * 64 * 64 + 2 * 64;                    // FLAG_HDR + 2 nb^2 + 2 nb, nb <= 64
constexpr size_t B7_INFO_BYTES = B7_INFO_HEAD_BYTES + 4 * B7_PERSIST_FLAG_WORDS_MAX;

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

// A pinned host buffer that grows on demand (b7_pin_ensure); dev: its device address when it is mapped, else null.
struct PinBuf {
  void *host = nullptr, *dev = nullptr;
  size_t bytes = 0;
};

// ---- the two fixed staging blocks of a context ------------------------------------------------------------
// What a fit reports to the host: the pivot report (first failing pivot, 1-based, 0 if none | hand-off time-out code) and the
// likelihood terms (sum log L_ii, then r_k' alpha_k per response column).
struct FitBlock { int info[4]; double terms[257]; };
// Direction numbers of the Sobol sequence (sobol.hip), uploaded into the scratch block.
constexpr int SOBOL_DIMS = 40;  // table rows (the reference admits dims < 40, grids/sobol.lua:36)
constexpr int SOBOL_BITS = 30;  // log_max, grids/sobol.lua:32
struct SobolTable {
  uint32_t v[SOBOL_DIMS][SOBOL_BITS];
};

// c->pinned: 16 KiB of pinned, device-mapped host memory.  Kernels write into it through c->pinned_dev, or a copy lands in it
// without pageable staging; the host reads after a stream synchronisation.
constexpr size_t B7_PINNED_BYTES = 16384;
struct PinnedBlock {
  FitBlock fit;                       // a fit's report (gp_api.hip: fit_hyp_core); the Bayesian linear head's, its first 16 bytes
  alignas(256) ArgBest best;             // launch_finish's arg-max (argbest.h), written by the kernel through the mapped address
  alignas(4096) double fmin[256];     // f_min of several response columns on their way to the device (stage_fmin)
  alignas(4096) double vec[B7_MAX_D + 3];  // a small vector on its way to the device: a fit's lengthscales (the one-launch fit reads
                                           // amp, noise and mean behind them), a grid map's per-column shift / scale
  alignas(4096) double tr[5 * B7_MAX_D];   // the trust-region map's center | lo | span | shift | hi on their way to the device
};
static_assert(offsetof(PinnedBlock, fit) == 0 && offsetof(PinnedBlock, best) == 2304 && offsetof(PinnedBlock, fmin) == 4096 &&
                  offsetof(PinnedBlock, vec) == 8192 && offsetof(PinnedBlock, tr) == 12288 && sizeof(PinnedBlock) <= B7_PINNED_BYTES &&
                  sizeof(ArgBest) == 16 && offsetof(ArgBest, i) == 8,
              "pinned block: kernels and copies address these slots");

// c->scratch: 64 KiB of device memory, never regrown.
constexpr size_t B7_SCRATCH_BYTES = 64 * 1024;
struct ScratchBlock {
  // THE LENGTHSCALES OF THE CURRENT FIT LIVE HERE UNTIL THE NEXT FIT: fit_hyp_core uploads them (or launch_fit_small leaves them,
  // through its hyp_out), and b7_gp_append / b7_gp_fantasize scale new points with them.  A nomination's batched fits keep theirs
  // in c->bhyp and declare the context's fit slot empty instead.
  double lenscale[256];
  double fmin[256];                   // f_min of several response columns (stage_fmin, b7_ei_compute)
  SobolTable sobol;                   // launch_sobol
  double minmax[2 * B7_MAX_D];        // a generated grid's mins | maxes (sobol.hip: upload_minmax)
  alignas(4096) double colvec[2 * B7_MAX_D];  // column minima | maxima out (b7_grid_colrange), a grid map's per-column vector in
  double trvec[5 * B7_MAX_D];         // the trust-region map's center | lo | span | shift | hi, d entries each (trust_region.hip)
};
static_assert(offsetof(ScratchBlock, lenscale) == 0 && offsetof(ScratchBlock, fmin) == 2048 && offsetof(ScratchBlock, sobol) == 4096 &&
                  offsetof(ScratchBlock, minmax) == 4096 + sizeof(SobolTable) && offsetof(ScratchBlock, colvec) == 12288 &&
                  offsetof(ScratchBlock, trvec) == 12288 + sizeof(double) * 2 * B7_MAX_D && sizeof(ScratchBlock) <= B7_SCRATCH_BYTES,
              "scratch block: the layout every earlier build used");

constexpr int B7_ACC_NONE = 0, B7_ACC_LINEAR = 1, B7_ACC_LOG = 2;  // b7_ctx::acc_kind

struct PhaseStat {
  double ms = 0.0;
  int64_t launches = 0;
};

// A score's parameters as the kernels take them (score.hip), built by score_params (nominate.hip) and nowhere else: S hyper
// samples' mean / variance on the device, sample s at mu + s * stride.  fmin == nullptr: one response column, its f_min in fmin0.
// S == 0: no score.  With S > 0 it is also a nomination's batched score, not launched yet: the exchange step runs it fused with
// score:div, the arg-max and the record (score.hip: score_finish_slot_kernel).  A value of the call that made it, never of the
// context: no later call can meet a pending score.
// A kind reads ONE of fmin (EI, LogEI) and ystar (MES: y*[S][nlev] on the device, sample s at ystar + s * nlev; mes.hip); they share
// a slot, and nlev sits in what was padding, so the argument layout of the EI / CB / LogEI kernels is what it was.
struct ScoreParams {
  int kind = 0, S = 0, upper = 0, nlev = 0;  // kind: B7_SCORE_*
  const double *mu = nullptr, *var = nullptr;
  union {
    const double *fmin = nullptr;
    const double *ystar;
  };
  long long stride = 0;
  double fmin0 = 0.0, tradeoff = 0.0, sign = 0.0;
};

// b7_eval_nominate_refine (refine.hip, score.hip): the starts' state on the device, downloaded whole at the end of a call
struct RefState {
  double x[B7_REFINE_MAX_STARTS][B7_MAX_D], g[B7_REFINE_MAX_STARTS][B7_MAX_D];  // point and marginal gradient
  double v[B7_REFINE_MAX_STARTS], eta[B7_REFINE_MAX_STARTS], score[B7_REFINE_MAX_STARTS];  // marginal value, step, the grid's score at the start
  long long idx[B7_REFINE_MAX_STARTS];  // the grid row it started from (0-based)
  int status[B7_REFINE_MAX_STARTS];     // B7_REFINE_* bits
  int active[B7_REFINE_MAX_STARTS];     // the queries in flight are this start's ladder (else: the start itself, four times)
};

// b7_ts_nominate_refine (ts_refine.hip): every start of every path of the last call, on the host
struct TsRefLast {
  bool valid = false, traced = false;
  int q = 0, P = 0, d = 0, iters = 0;
  std::vector<double> x, v;     // [q][16][d], [q][16]
  std::vector<long long> idx;   // [q][16] the grid rows the starts began at (0-based)
  std::vector<int> status;      // [q][16] B7_REFINE_* bits
};

// What the last path-drawing call left on a context: filled once, by ts_paths_core (rff.hip: b7_ts_nominate, b7_ts_paths) or by
// b7_blr_ts_nominate (blr_ts.hip), read by everything that picks from, refines or downloads the kept paths.  A call that draws
// paths starts by setting who = TS_NONE, so a failed call leaves none.  The DNGO head's paths are laid out like a GP's ([M][q]), its
// ts_draw holds eps [q][z] | weight [q][z], F = z and N = d = 0.
enum { TS_NONE = 0, TS_GP = 1, TS_BLR = 2 };  // TsPaths::who
struct TsPaths {
  int who = TS_NONE;
  int64_t M = 0;
  int q = 0, S = 0, F = 0, N = 0, d = 0;
  int ns = 0;          // min(S, q): the hyper samples that own a path
  uint64_t epoch = 0;  // the context's epoch when the paths were made
  std::vector<double> hyp;  // a GP's ns hyper samples: lenscale_sq d | amp | noise | mean each
  // the pieces of c->ts_work that outlive the call.  alpha (a GP's): sample s's columns at alpha + s alpha_stride ([Npad][yld], yld =
  // 1 or the sample's columns rounded up to 64; column p is v_j of path j = s + S p).  pmin / taken [q], part [nblk]: the arg-mins'
  const double *alpha = nullptr;
  int64_t alpha_stride = 0;
  double *pmin = nullptr;
  long long *taken = nullptr;
  ArgBest *part = nullptr;
  int nblk = 0;
};
struct b7_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_fit = nullptr;  // behind the fit report's copy: b7_gp_predict_hyp waits for it, not for the prediction
  // streams_order (context.hip): the other contexts' streams of a call -> this one (slot m - 1 for the m-th), and back (the last slot)
  hipEvent_t ev_order[1 + B7_TS_FEAS_CMAX] = {};
  std::string err;
  int cus = 0;

  // ---- candidate grid (row-major M x d), ping-pong for stable row removal
  DevBuf grid[2];
  int grid_cur = 0;
  int64_t M = 0;
  int d = 0;

  // ---- fit state
  bool fitted = false;
  bool have_data = false;  // b7_gp_set_data has put X_obs / Y_obs on the device
  int model_kind = 0;  // 0 = GP regressor, 1 = Bayesian linear head (DNGO): selects the predict path
  int N = 0, Npad = 0, dfit = 0, dpad = 0, ycols = 0;
  int yld = 1;   // leading dimension of alpha: 1 for one column, else ycols rounded up to 64 (zero padded)
  double amp = 0, noise = 0, mean = 0;
  b7_gp_opts opts;
  int kernel = B7_KERNEL_ARDSE;  // covariance kernel of every K this context forms (b7_gp_set_kernel): the launchers pick the instance
  DevBuf xobs;   // N x d raw observations
  DevBuf w;      // dpad inverse squared lengthscales (0 in the padding)
  DevBuf zsc;    // Npad x dpad: observations scaled by w (0 in the padding)
  DevBuf zss;    // Npad: (sum z^2 w)/2  (+inf in the padding -> covariance 0)
  DevBuf K;      // Npad x Npad: K(X,X)+noise*I as assembled (kept for the jitter retries)
  DevBuf L;      // Npad x Npad: lower Cholesky factor (upper triangle zero)
  DevBuf Linv;   // Npad x Npad: explicit inverse of L (upper triangle zero)
  DevBuf W;      // Npad x Npad: scratch of the triangular inversion
  DevBuf dinv;   // (Npad/64) x 64 x 64: inverses of L's diagonal blocks
  DevBuf alpha;  // Npad x yld (0 in the padding)
  DevBuf resid;  // Npad x ycols: Y - mean, then L^-1 (Y - mean)
  DevBuf atmp;   // launch_alpha's intermediates: t = Linv resid (Npad x ycols) + slice partials (nslices x ycols x Npad)
  DevBuf info;   // int[4]: first failing pivot (1-based), 0 if none
  DevBuf ybuf;   // N x ycols raw

  // ---- predict / score state over the resident grid
  bool predicted = false;
  int64_t Mpred = 0;
  DevBuf mu;     // M x ycols
  DevBuf var;    // M
  DevBuf acc;    // M score accumulator
  bool acc_valid = false;
  int spin_us = 500;         // how long a call spins on a completion word in mapped host memory before it waits for the stream (B7_SPIN_US; 0: never)
  bool npad_small = true;    // N <= 64 (and <= 64 basis features) padded to ONE 64-block (B7_NPAD_SMALL=0: to 128)
  bool potrf_small = true;   // Npad == 64: factorisation + inverse (+ alpha) in one workgroup of one launch (blr_small.hip); B7_POTRF_SMALL=0 / any explicit B7_POTRF_SCHED: off
  bool blr_small = true;     // b7_blr_eval_nominate: the head for z <= 64 features in one workgroup of one launch (blr_small.hip)
  double fmin_scalar = 0.0;  // f_min of a single response column: a kernel argument of the EI kernels (launched with fmin_dev == nullptr), no staging copy
  bool acc_fresh = false;  // the accumulator stands for zeros that were never written: the next score launch onto it starts from 0.0
                           // (acc_valid, acc_fresh and acc_kind change only through score.hip's acc_* helpers)
  int acc_kind = 0;        // what the live accumulator holds (B7_ACC_*): nothing added since the reset, a linear sum (EI, CB), or a
                           // running log-sum-exp (LogEI), whose empty value is -inf and whose score:div is a subtraction of log(divisor)
  DevBuf ks;     // K(X*,X) chunk workspace
  size_t ks_bytes = (size_t)4 << 30;
  int diag_variant = 1;  // 64x64 diagonal-block kernel: 0 = rsqrt pivot chain, 1 = square-root-free chain with the DPP-fused
                         // multiply-add, 2 = the same with mov_dpp + fma (the bit-for-bit reference of 1) (B7_DIAG_VARIANT)
  int inverse_inline = 1;  // build inv(L) inside the factorisation launches: 0 never (separate trtri passes), 1 for
                           // Npad <= 8192, 2 always (B7_INVERSE_INLINE)
  PinnedBlock *pinned = nullptr, *pinned_dev = nullptr;  // the fixed pinned block as the host / the device addresses it
  std::vector<double> net_host;  // the basis network last uploaded to netbuf (packed W, b per layer)
  PinBuf pin_blr;   // b7_blr_eval_nominate: staging of the observations and beta (y - mean) (not mapped)
  PinBuf pin_eval;  // b7_eval_nominate: [S][4] pivot reports + the packed hypers of all S samples (mapped)
  PinBuf pin_nll;   // b7_gp_nll_batch: hypers in, results out (mapped)
  PinBuf pin_slice; // b7_gp_slice_sample: start points, bounds and widths in, samples, values, statuses and the completion counter out (mapped)
  DevBuf slice_state;          // b7_gp_slice_sample: the chains' state blocks (slice_chain_kernel)
  DevBuf slice_trace;          // b7_gp_slice_trace_enable: the last call's trace records, [C][rpc][B7_SLICE_TRACE_WIDTH] doubles | [C] counts
  int slice_trace_rpc = 0;     // records per chain to keep (0: no trace)
  int slice_trace_C = 0, slice_trace_D = 0;  // shape of what the last traced call left (0: nothing)
  bool fmin_staged = false;  // the fmin staging slot of the pinned block holds a caller's values
  bool potrf_attrs_set = false;  // dynamic-LDS limits of the Cholesky kernels raised (once per context)
  bool linv_done = false;  // launch_potrf produced Linv for the current factor
  int potrf_sched = 3;   // 1: one panel at a time (near update fused into the panel solve, far update riding on the
                         // next diagonal-block launch) for Npad <= 4096, 2: always; 0: panel groups with separate
                         // update launches; 3: ONE persistent launch for Npad <= 4096, else as 1 (B7_POTRF_SCHED)
  int syrk_small = 1;    // whole-K single-stage kernel for trailing updates with <= 256 tiles (B7_SYRK_SMALL)
  int potrf_defer = 1;   // far part of each trailing update rides on the next diagonal-block launch (B7_POTRF_DEFER)
  int potrf_group = 2;   // panels per bulk trailing update of the Cholesky (B7_POTRF_GROUP overrides); A/B at
                         // N = 2048 (tools/potrf_ab.py): G = 1 1.068 ms, 2 1.067, 4 1.119, 8 1.274
  // ---- persistent Cholesky schedule (potrf_persist.hip)
  struct JobList { DevBuf buf; int n = 0; };
  std::map<int, JobList> pjobs_cache;  // job queues by (nb, mode)
  DevBuf pstamps;  // diagnostics (B7_PERSIST_STAMPS)
  int pjobs_nb = 0, pjobs_n = 0;   // shape of the last single persistent launch (for the stamp reader)
  // b7_gp_nll_batch: B fits of the resident data in likelihood mode
  DevBuf bhyp, bw, bzsc, bzss, bK, bL, bdinv, bflags, binfo, bresid, bterms, bLinv, balpha, bmu, bvar;
  bool persist_attr_set = false, persist_stamps = false;
  int persist_helpers = 0;   // cap on the helper workgroups (B7_PERSIST_HELPERS; 0 = one per remaining CU)
  int persist_aborts = 0;    // launches that gave up waiting and were redone with the launch schedule
  int nll_small = 1;         // b7_gp_nll_batch at Npad <= 128, d <= 32: the one-workgroup-per-evaluation kernel (B7_NLL_SMALL: 0 general
                             // path, 1 gp_small_kernel (eight waves), 2 round 3's four-wave nll_small_kernel)
  bool kpost_small = true;   // GP posterior at Npad <= 128, d <= 32, one response column: K(X*,X), mean and variance in one kernel, K*
                             // never stored (kpost_small.hip; B7_KPOST_SMALL=0: ksx_kernel + post_kernel)
  bool fit_small = true;     // b7_eval_nominate / b7_gp_fit_hyp at Npad <= 128, d <= 32, one response column: the whole fit of a hyper
                             // vector in one workgroup of one launch (gp_small.hip; B7_FIT_SMALL=0: the general schedule)
  int persist_fault = -1;    // tests only (B7_PERSIST_FAULT): panel whose flag workgroup 0 withholds, to exercise the time-out
  int potrf_sched_saved = 0; // the schedule to return to after such a redo
  DevBuf part;   // argmax partials (value, index)
  // ---- max-value entropy search (mes.hip): y* of the last search, its brackets and the rounds' partial sums, laid out by mes_begin
  DevBuf ystar, mes_ticket;
  DevBuf mes_user;          // b7_mes_compute: the caller's y* (up to B7_MES_KMAX doubles), apart from the last search's
  int mes_levels = 8;       // K of the searches a score starts (b7_mes_set_levels)
  int mes_S = 0, mes_K = 0, mes_nb = 0;  // the layout of c->ystar: samples, levels, row blocks
  int64_t mes_M = 0;        // rows per sample of that layout
  int mes_slot = 0;         // the sample slot the next score_add of kind MES searches into (the nomination's per-sample loops set it)
  bool mes_valid = false;   // a search has filled the buffer since it was laid out (b7_mes_last_ystar)
  DevBuf ticket; // score_finish_slot_kernel's arrival counter (zero between launches)
  // ---- the feasibility column (score.hip: b7_feas_*): log-weights L[M] over the resident grid, allocated on demand, forgotten with
  // the accumulator whenever the grid changes (feas_valid changes only through score.hip's feas_* helpers)
  DevBuf feas;
  DevBuf feas_stage;        // b7_feas_add's host vector on its way onto the column
  bool feas_valid = false;
  DevBuf scratch; // a ScratchBlock (b7_scratch)
  DevBuf tmpgrid; // predict_at temporary grid
  DevBuf tmpmu, tmpvar;
  DevBuf fant;   // fantasize workspace (pending-point covariance pieces)
  // ---- b7_eval_nominate_batch (batch.hip): per hyper sample the posterior mean, the variance being downdated and the
  // believer columns u_1 .. u_q-1 over the grid ([S][M] each), and the small vectors of a pick
  DevBuf bel;     // mu [S][M] | var [S][M] | u [q-1][S][M]
  DevBuf belvec;  // per sample: k(X, x_j) [Npad] | w_j = inv(K) k(X, x_j) [Npad] | amp, noise + jitter | t_j, u_i(x_j) (i < j)
  PinBuf pin_bel; // amp, noise + jitter of the S samples on their way to belvec (not mapped)
  // ---- b7_ts_nominate (rff.hip): the last call's sample paths and draws (b7_ts_last_paths / _draws), one hyper sample's operands,
  // and b7_rff_compute's staging, apart from them
  DevBuf ts_paths;  // [M][q]
  DevBuf ts_draw;   // omega [min(S, q)][F][d] | phase [F] | weight [q][F] | eps [q][N]
  DevBuf ts_work, ts_user;
  TsPaths ts;  // what the last path-drawing call left (above)
  // ---- b7_ts_nominate_refine / b7_ts_path_grad_at (ts_refine.hip): the packed operands and the starts' state, the last call's
  // trace, b7_ts_path_grad_at's staging, and the last call's result on the host
  DevBuf ts_ref_ws, ts_ref_trace, ts_ref_user;
  bool ts_ref_trace_on = false;
  TsRefLast ts_ref_last;
  // ---- b7_ts_hvi_nominate / b7_ts_hvi3_nominate / b7_hvi_compute (ts_hvi.hip): the staged front or boxes, the picks, the arg-max
  // partials (ts_hvi), the [q][M] copies of the objectives' paths (ts_hvi_t) and b7_hvi_compute's staging, apart from the kept paths
  DevBuf ts_hvi, ts_hvi_t, ts_hvi_user;
  int ts_hvi_layout = 1;  // 1: a pick reads a contiguous column of a [q][M] copy made once per call; 0: column j of [M][q] at stride q
  // ---- b7_ts_feas_nominate / b7_ts_feas_compute (ts_feas.hip): the arg-min partials, the paths' bests, the exclusion list and the
  // picks' values (ts_feas), and b7_ts_feas_compute's staging, apart from the kept paths
  DevBuf ts_feas, ts_feas_user;
  int ts_feas_onepass = 0;  // 0: path by path, q chained passes (default: the faster arm on real paths); 1: all q paths scored in one pass, exclusions resolved on the host
  // ---- b7_eval_nominate_refine / b7_gp_grad_at (refine.hip): the workspace of 64 query columns, the last call's trace and result
  DevBuf refine_ws, refine_trace;
  DevBuf refine_user;       // b7_score_grad_compute's staging, apart from them
  bool refine_trace_on = false, refine_valid = false;
  int refine_P = 0, refine_d = 0, refine_iters = 0, refine_trace_P = 0, refine_trace_iters = 0;  // shapes of what the last call left (trace_P 0: no trace)
  RefState refine_last;     // the last call's final state
  // ---- b7_kg_nominate (kg.hip): what the last call left for b7_kg_last, and b7_kg_compute's staging, apart from it
  DevBuf kg;         // mu [S][M] | var [S][M] | v [S][M]: every sample's posterior and its knowledge gradient over the grid
  DevBuf kgvec;      // the small arrays of a call (kg.hip: KgState)
  DevBuf kg_slopes;  // [S][M][n + 1], written only while b7_kg_trace_enable is on
  DevBuf kg_user;
  PinBuf pin_kg;     // amp, noise + jitter of the S samples on their way to kgvec (not mapped)
  bool kg_trace_on = false, kg_valid = false, kg_traced = false;
  int kg_S = 0, kg_n = 0;  // the shapes of what the last successful call left
  int64_t kg_M = 0;
  size_t kg_al_off = 0;    // where that call's alpha [S][16] sits in kgvec (doubles); the rows of A follow it
  // ---- b7_eval_posterior / b7_ehvi_* (ehvi.hip): the kept posterior of the last b7_eval_posterior, forgotten with the accumulator
  // whenever the grid changes and whenever the data does (post_forget); the front's staging; b7_ehvi_compute's staging, apart
  DevBuf post;       // mu [S][M] | var [S][M]
  bool post_valid = false;
  int post_S = 0;
  int64_t post_M = 0;
  DevBuf ehvi_front; // a_1 .. a_P, r1 | r2, b_1 .. b_P: 2 (P + 1) doubles as the kernel reads them
  DevBuf ehvi_user;
  // ---- b7_ehvi3_* (ehvi3.hip): three objectives over the same kept posteriors
  DevBuf ehvi3_front;  // the cuts of the three objectives (3 (PMAX + 1) doubles), then the boxes as five table rows each (ints)
  DevBuf ehvi3_table;  // T [rows][C] of one chunk of C candidates, then the row-class flags [3][C] (ints)
  DevBuf ehvi3_user;   // b7_ehvi3_compute's staging, apart from the kept posterior
  // ---- the probit classifier (laplace.hip): per fit of the last call nll | iterations | info | psi ([B][4] doubles), then the mode
  // f | a | W ([3][Npad]) of the last b7_clf_fit_hyp; b7_probit_compute's staging, apart from them
  DevBuf clf, clf_mode, clf_user;
  uint64_t clf_lab_epoch = ~(uint64_t)0;  // the epoch at which the resident labels were last checked to be 0 / 1, their count then, and
  int clf_lab_N = 0, clf_lab_bad = 0;     // the first offender (1-based; 0: none)
  bool clf_mode_valid = false;  // b7_clf_fit_hyp has left a mode since the data, the kernel or the fit slot last changed
  uint64_t clf_epoch = 0;       // the context's epoch when it did
  int clf_N = 0;
  DevBuf feat;   // DNGO basis features of the resident grid: Mfeat x Npad (zero-padded columns)
  size_t feat_zeroed_bytes = 0;  // how much of `feat` was zeroed when it was laid out for feat_z columns
  int feat_z = -1;
  int64_t Mfeat = 0;
  int zdim = 0;
  uint64_t feat_version = 0, grid_version = 0;
  uint64_t epoch = 0;  // counts the changes of the grid, the data or the covariance kernel (post_forget): what was kept under an earlier one is stale
  DevBuf netbuf; // MLP weights/biases of the basis network
  // ---- likelihood gradients and the bounded fit (nll_grad.hip)
  DevBuf gradpart;           // [tiles][d + 2] partial sums of the last gradient, then its d + 3 components
  PinBuf pin_grad;           // those components on their way to the host (not mapped)
  bool grad_hook = false;    // fit_hyp_core enqueues the gradient behind the fit's tail (set around the call by b7_gp_fit_hyp_grad)
  bool gfit = false;         // the context's fit slot holds what fit_hyp_core left (b7_gp_nll_grad asks: fit_front and b7_gp_append
  double gfit_jitter = 0.0;  // withdraw it; a change of the grid does not), with its jitter and the N it was made at
  int gfit_N = 0;
  bool map_trace_on = false; // b7_gp_fit_map_trace_enable
  std::vector<double> map_trace;  // the last traced b7_gp_fit_map's records, map_trace_n of map_trace_w doubles
  int map_trace_n = 0, map_trace_w = 0;

  // ---- the arg-max exchange (comm.hip): RCCL communicator of this rank, one per context = per GPU = per process
  void *comm = nullptr;  // ncclComm_t
  int comm_rank = 0, comm_world = 1;
  DevBuf slots;  // [world, B7_TAB_W] x u64 exchange table (also the staging of b7_comm_allreduce_f64)
  uint64_t *tab_host = nullptr;  // pinned, device-mapped host copy of the table: B7_MAX_WORLD records, a staging record, the completion word
  uint64_t *tab_host_dev = nullptr;  // its device address
  struct b7_group *group = nullptr;  // set while the context is a member of a single-process group (group.hip)
  bool group_busy = false;           // ... and this while the group itself is calling the member's grid mutators
  // the last exchange as every rank saw it: the winner (index, owning rank, grid row) and the row count of every shard.
  // b7_nominate_commit takes the row from here, so that a model-based trial needs no second collective.
  bool win_valid = false;
  int64_t win_idx1 = 0;
  int win_rank = -1, win_d = 0;
  double win_row[B7_MAX_D];
  int64_t shard_rows[B7_MAX_WORLD];
  int shard_world = 0;

  // ---- measurement
  hipEvent_t tev[B7_MAX_TIMERS][2];
  bool tev_init = false;
  bool profile = false;
  std::map<std::string, PhaseStat> phases;
  // phase profiling without host synchronisation: event pairs are recorded into `pending` and turned into times
  // when somebody asks (b7_profile_get / _reset), after one stream synchronisation; events are recycled
  struct PendingPhase { const char *name; hipEvent_t e0, e1; };
  std::vector<PendingPhase> pending;
  std::vector<hipEvent_t> free_events;
  hipEvent_t phase_e0 = nullptr;  // start event of the phase being recorded
};

// ---- error helpers ---------------------------------------------------------------------------------
int b7_fail(b7_ctx *c, int code, const char *fmt, ...);
// (the message names the call site, not the expression: the library's strings hold no internal constant names)
#define B7_HIP(c, expr)                                                                          \
  do {                                                                                           \
    hipError_t e__ = (expr);                                                                     \
    if (e__ != hipSuccess)                                                                       \
      return b7_fail((c), e__ == hipErrorOutOfMemory ? B7_ERR_NOMEM : B7_ERR_HIP, "%s:%d: %s", \
                     __FILE_NAME__, __LINE__, hipGetErrorString(e__));                           \
  } while (0)
#define B7_TRY(expr)          \
  do {                        \
    int rc__ = (expr);        \
    if (rc__ != B7_OK) return rc__; \
  } while (0)

int b7_ensure(b7_ctx *c, DevBuf &b, size_t bytes);
void b7_release(DevBuf &b);
// at least `bytes` of pinned host memory in b; growing waits for the stream (nothing in flight may use the old block) and allocates twice the need
int b7_pin_ensure(b7_ctx *c, PinBuf &b, size_t bytes, bool mapped);
static inline ScratchBlock *b7_scratch(const b7_ctx *c) { return static_cast<ScratchBlock *>(c->scratch.p); }

// Phase timing (no-ops unless profiling is on).
struct PhaseScope {
  b7_ctx *c;
  const char *name;
  PhaseScope(b7_ctx *c, const char *name);
  ~PhaseScope();
};

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
// The padded size of a system of n observations (or basis features): one 64-block up to n = 64 -- the first 64 trials of every
// run at the reference's defaults, and the 50 features of models/dngo.lua's head: a quarter of the posterior's work and
// half the K* bytes of the 128 padding --, multiples of 128 (the posterior kernels' n-tile) above.  B7_NPAD_SMALL=0 (read in
// b7_create, like every switch): 128 always.
int npad_of(const b7_ctx *c, int64_t n);

// ---- where fits live ----------------------------------------------------------------------------------------
// A read-only view of S >= 1 fits of the resident data, side by side on the device: what every posterior launcher is told instead
// of reading the context's fit fields.  Sample s sits at base + s * stride; THE STRIDES ARE WRITTEN HERE AND NOWHERE ELSE on the
// host.  The fit scalars come in one of two forms: on the host (amp_dev == nullptr; one fit), or as device arrays of S entries
// (the HypPack of c->bhyp).  It owns nothing.  Built by ctx_fit / batch_fits / fit_at alone.
struct FitSet {
  const double *w = nullptr, *zsc = nullptr, *zss = nullptr, *Linv = nullptr, *alpha = nullptr;
  int S = 1, Npad = 0, dpad = 0;  // the padded shape of the data the fits are of (the context's, when the view was made)
  double amp = 0.0, noise = 0.0, mean = 0.0;
  const double *amp_dev = nullptr, *noise_dev = nullptr, *mean_dev = nullptr;
  static int64_t s_w(int, int dpad) { return dpad; }
  static int64_t s_zsc(int Npad, int dpad) { return (int64_t)Npad * dpad; }
  static int64_t s_zss(int Npad, int) { return Npad; }
  static int64_t s_Linv(int Npad, int) { return (int64_t)Npad * Npad; }
  static int64_t s_alpha(int Npad, int) { return Npad; }
};
// the context's own slot: what the fit producers (fit_front, launch_potrf*, launch_alpha, launch_fit_small) leave
static inline FitSet ctx_fit(const b7_ctx *c) {
  FitSet f;
  f.w = (const double *)c->w.p, f.zsc = (const double *)c->zsc.p, f.zss = (const double *)c->zss.p;
  f.Linv = (const double *)c->Linv.p, f.alpha = (const double *)c->alpha.p;
  f.Npad = c->Npad, f.dpad = c->dpad;
  f.amp = c->amp, f.noise = c->noise, f.mean = c->mean;
  return f;
}

// ---- kernel launchers (each enqueues on c->stream and returns a B7 code) ----------------------------
// sobol.hip
int launch_sobol(b7_ctx *c, double *out, int64_t size, int dims, int64_t skip, const double *mins,
                 const double *maxes);
int launch_random_grid(b7_ctx *c, double *out, int64_t size, int dims, uint64_t seed, int64_t row_offset,
                       const double *mins, const double *maxes);
int launch_remove_row(b7_ctx *c, const double *src, double *dst, int64_t M, int d, int64_t idx0);
int launch_remove_rows(b7_ctx *c, const double *src, double *dst, int64_t M, int d, const int64_t *cuts_dev, int ncut);
int launch_colrange(b7_ctx *c, const double *grid, int64_t M, int d, double *out_dev);
int launch_col_affine(b7_ctx *c, double *grid, int64_t M, int d, const double *v_dev, bool mul);
int launch_gather_rows(b7_ctx *c, const double *src, double *out, const int64_t *idx0_dev, int64_t n, int d);
// trust_region.hip: the map of b7_grid_trust_region over M x d base points in place; vec_dev = center | lo | span | shift | hi (d each)
int launch_trust_region(b7_ctx *c, double *grid, int64_t M, int d, const double *vec_dev, bool rotate, double prob, uint64_t seed,
                        int64_t row_offset);

// covar.hip
struct KBatchDesc {   // a batch of fits over the same observations: strides (doubles) per fit, per-fit amplitudes
  int64_t s_w = 0, s_zsc = 0, s_zsh = 0, s_out = 0;
  const double *amp = nullptr;
  // the posterior mean of every fit alongside (K(X*,X) of a batch of fits over the same candidates): per-fit alpha stride,
  // constant means, output stride
  int64_t s_alpha = 0, s_mu = 0;
  const double *mean = nullptr;
};
struct ObsSet {
  const double *zsc;  // npad x dpad scaled observations
  const double *zsh;  // npad half norms (+inf in the padding)
  int npad;
  const double *w = nullptr;  // inverse squared lengthscales (dpad); null = the context's current ones
  KBatchDesc batch;
};
int launch_prep_obs_aux(b7_ctx *c, const double *xobs, const double *ls_dev, int N, int npad, double *zsc,
                        double *zsh);
int launch_k_generic(b7_ctx *c, const double *xq, int64_t rows, int64_t Mtotal, const ObsSet &o, double *out);
int launch_prep_obs(b7_ctx *c, const double *xobs, const double *lenscale_sq_dev, int N, int d);
int launch_kxx(b7_ctx *c, double diag_add);
// K(X*,X) and the mean of f's S fits (device scalars) over the same rows in one launch: K*_s = ks + s s_out, mu_s = mu + s s_mu
int launch_ksx_batch(b7_ctx *c, const FitSet &f, const double *xq, int64_t rows, int64_t Mtotal, double *ks, int64_t s_out,
                     double *mu, int64_t s_mu);
int launch_kxx_batch(b7_ctx *c, int B, const double *ls_dev, const double *amp_dev, const double *noise_dev, double *w,
                     double *zsc, double *zss, double *K);
int launch_ksx(b7_ctx *c, const FitSet &f, const double *xq, int64_t row0, int64_t rows, int64_t Mtotal, int d, double *ks,
               double *mu, int ycols);

// potrf.hip
// What a factorisation hands to the launch_alpha that follows it (the one-block kernel does more than factor): passed by the
// caller from one to the other, not kept in the context -- a caller that changes the residual or the response columns in
// between simply does not pass it on.
struct FactorNote {
  bool alpha_done = false;        // alpha (one response column) is already in c->alpha
  int *report_written = nullptr;  // where the pivot report was mirrored (mapped host memory), or null
};
// K + extra*I -> L, dinv, info (+ Linv, using W).  report_hint: where a one-block factorisation should mirror its pivot report
// itself (mapped host memory), or null; note (nullable): see FactorNote
int launch_potrf(b7_ctx *c, double extra, bool with_inverse, int *report_hint = nullptr, FactorNote *note = nullptr);
int launch_trtri(b7_ctx *c);           // L, dinv -> Linv (no-op when launch_potrf already built it)
int launch_potrf_persist(b7_ctx *c, double extra, bool with_inverse);  // the same in one persistent launch (Npad <= 4096)
int launch_nll_batch(b7_ctx *c, int B, const double *K, double *L, double *dinv, unsigned *flags, int *info,
                     const double *resid, double *terms);
int launch_nll_one(b7_ctx *c, const double *K, double *L, double *dinv, unsigned *flags, int *info, const double *resid,
                   double *terms, double extra);
size_t persist_flag_words_host(int nb);
// blr_small.hip, nll_small.hip
int launch_potrf_small(b7_ctx *c, int B, const double *K, double *L, double *Linv, double *dinv, const double *resid, double *alpha,
                       double extra, int *info, int *report_dev, int64_t sK, int64_t sL, int64_t sdinv, int64_t svec, int sinfo);
int launch_blr_head_small(b7_ctx *c, const double *Z, int N, int z, int ldz, const double *yv, double alpha_prec, double beta,
                          int *report_dev);
int launch_blr_heads_small(b7_ctx *c, int S, const double *Z, int N, int z, int ldz, const double *yraw_dev, const double *hyp3_dev,
                           double *L, double *Linv, double *m, double *b, int *info, int *report_dev, double *terms);
int launch_post_heads(b7_ctx *c, int S, const double *Linv, const double *feat, int64_t rows, int64_t Mtotal, double *var, int64_t svar,
                      const double *zero_dev, const double *invbeta_dev);
int launch_gemv_rows_batch(b7_ctx *c, int S, const double *A, int lda, const double *x, int64_t sx, int n, const double *base_dev,
                           int64_t rows, double *y, int64_t sy);
int launch_nll_small(b7_ctx *c, int B, const double *hyp_dev, const double *hyp_host, double *terms_dev, int *info_dev,
                     unsigned *done_dev);
// laplace.hip: B Laplace fits of the probit classifier, one workgroup each, the whole Newton iteration inside the launch.  K: the
// fits' covariance matrices K(X,X) without a diagonal term, Npad x Npad each at stride sK (the lower triangle is read; the kernel mirrors
// it into the upper one); mean_dev: B constant means on the device, or null with the one fit's mean in mean0; out [B][4] (nll,
// iterations, info bit 0 = not converged within the cap, psi); Linv / alpha (both null: the evidence only): L^-1 W^1/2 and a in the
// batch-slot layout of FitSet; mode (nullable): f | a | W, [3][Npad] per fit
int launch_laplace_small(b7_ctx *c, int B, double *K, int64_t sK, const double *mean_dev, double mean0, double *out, double *Linv,
                         double *alpha, double *mode);
// kpost_small.hip
bool kpost_small_applies(const b7_ctx *c);
int launch_kpost_small(b7_ctx *c, const FitSet &f, const double *xq, int64_t M, double *mu, double *var, int64_t sout);
// gp_small.hip
bool gp_small_applies(const b7_ctx *c);
// ... and the whole fit of a hyper vector runs as one workgroup of one launch (launch_fit_small)
static inline bool fit_small_applies(const b7_ctx *c) {
  return c->fit_small && c->potrf_sched == 3 && c->inverse_inline && gp_small_applies(c);
}
int launch_nll_small8(b7_ctx *c, int B, const double *hyp_dev, const double *hyp_host, double *terms_dev, int *info_dev,
                      unsigned *done_dev);
int launch_fit_small(b7_ctx *c, int B, const double *hyp_dev, const double *hyp_host, double *hyp_out, double *w, double *zsc,
                     double *zss, double *L, double *Linv, double *dinv, double *alpha, double *resid, int *info_dev,
                     int *report_dev);
// report_dev (nullable): device address of mapped host memory that receives the first report_words ints of the pivot report
// resid, Linv -> alpha; report_dev (nullable): the pivot report's mirror; note: what the factorisation just before already did
int launch_alpha(b7_ctx *c, int *report_dev = nullptr, int report_words = 0, const FactorNote &note = FactorNote());
int launch_alpha_batch(b7_ctx *c, int B, const double *Linv, const double *resid, double *alpha, const int *report_src = nullptr,
                       int *report_dev = nullptr, int report_words = 0);  // B single-column fits
int launch_fit_batch(b7_ctx *c, int B, const double *K, double *L, double *Linv, double *dinv, unsigned *flags, int *info);
int launch_nll_terms(b7_ctx *c, double *out_dev);  // out[0] = sum log L_ii, out[1 + k] = r_k' alpha_k
int launch_fro_norm_sq(b7_ctx *c, const double *A, int n, int ld, double *out_dev);  // sum of squares of A[0:n, 0:n]
int launch_set_identity(b7_ctx *c);    // L = I (Npad x Npad), dinv = identity blocks: the chol(I) fallback

// posterior.hip
// the variance of one fit (host scalars; c->model_kind == 1: f.Linv and f.noise are a Bayesian linear head's, ks its features)
int launch_post(b7_ctx *c, const FitSet &f, const double *ks, int64_t row0, int64_t rows, int64_t Mtotal, double *var);
int launch_post_batch(b7_ctx *c, const FitSet &f, const double *ks, int64_t sks, int64_t rows, int64_t Mtotal, double *var,
                      int64_t svar);

// extras.hip
int launch_mean_multi(b7_ctx *c, const FitSet &f, const double *ks, int64_t row0, int64_t rows, int64_t Mtotal, double *mu);
int launch_gemm_nt(b7_ctx *c, const double *A, int lda, const double *B, int ldb, double *C, int ldc, int m, int n,
                   int k);
int launch_fantasy_cov(b7_ctx *c, const double *kpp, const double *g, double *S, int P, double diag_add);
int launch_fantasy_factor(b7_ctx *c, double *S, double *dinv_tmp, int *info_dev);
int launch_fantasy_sample(b7_ctx *c, const double *Lp, const double *mu, int P, int n, uint64_t seed, double *out);
int launch_add_diag(b7_ctx *c, double *S, int ld, int n, double v);

int launch_append_finalize(b7_ctx *c, const double *krow, const double *lvec, const double *uvec, const double *evec,
                           int *status_dev);
int launch_append_vectors(b7_ctx *c, const double *krow, double *lvec, double *uvec, double *part, double *evec);
int launch_mlp_forward(b7_ctx *c, const double *X, int64_t M, int d, const double *net_dev, const int *dims,
                       int n_layers, int activation, double *out, int ld_out);
int launch_mlp_forward_mean(b7_ctx *c, const double *X, int64_t M, int d, const double *net_dev, const int *dims,
                            int n_layers, int activation, double *out, int ld_out, const double *mvec, double mean0,
                            double *mu, bool *mean_done);
int launch_gemv_rows(b7_ctx *c, const double *A, int lda, const double *x, int n, double base, int64_t row0,
                     int64_t rows, int64_t Mtotal, double *y);
int launch_transpose_pad(b7_ctx *c, const double *Z, int n, int ldz, int z, double *Zt, int zpad, int nk);
int launch_blr_assemble(b7_ctx *c, const double *G, double *K, int z, int zpad, double alpha_prec, double beta);

// score.hip
// one hyper sample's score of mu (M x ycols) / var (M) written to out or added onto it; p's S samples added onto acc in order
int launch_score(b7_ctx *c, ScoreParams p, const double *mu, const double *var, int64_t M, int ycols, double *out, bool accumulate);
int launch_score_batch(b7_ctx *c, const ScoreParams &p, double *acc, int64_t M);
// logacc: acc is a log accumulator -- score:div is acc - log(divisor)
int launch_finish(b7_ctx *c, double *acc, int64_t M, double divisor, double *best_val, int64_t *best_idx1, bool logacc = false);
int launch_fill(b7_ctx *c, double *p, int64_t n, double v);
// feas (nullable): the feasibility column; every row becomes w(acc / divisor, feas[j]) before the arg-max (score.hip's header)
int launch_finish_slot(b7_ctx *c, double *acc, int64_t M, double divisor, uint64_t *tab_dev, int rank, int world,
                       int64_t offset, const double *grid, int d, bool all_slots, uint64_t *host_rec = nullptr,
                       unsigned *host_done = nullptr, bool logacc = false, const double *feas = nullptr);

// excl (nullable): rows that take no part in the arg-max (their score is still written to acc)
// feas (nullable, not together with excl): the feasibility column, applied between score:div and the arg-max
struct ExclRows {
  int n = 0;
  long long row[B7_BATCH_MAX];  // 0-based
};
int launch_score_finish_slot(b7_ctx *c, const ScoreParams &p, double *acc, int64_t M, double divisor, uint64_t *tab_dev,
                             int rank, int world, int64_t offset, const double *grid, int d, bool all_slots, uint64_t *host_rec = nullptr,
                             unsigned *host_done = nullptr, const ExclRows *excl = nullptr, const double *feas = nullptr);
// the accumulator's state: zeros declared (bots/bayesopt.lua:69 without a launch of its own: the first score launch onto it
// starts from 0.0; score_kind: the B7_SCORE_* it will add), zeros written now, no accumulator (the grid changed), declared zeros
// written before anybody reads them
void acc_declare_zeros(b7_ctx *c, int score_kind);
int acc_write_zeros(b7_ctx *c);
// the caller writes every row of c->acc with a finished log score on c's stream (ehvi_nominate): a log accumulator, valid, not fresh
void acc_declare_log_written(b7_ctx *c);
void acc_forget(b7_ctx *c);
int acc_materialize(b7_ctx *c);
void feas_forget(b7_ctx *c);  // the grid changed: there is no feasibility column until the next b7_feas_reset
// the grid or the data changed: there is no kept posterior until the next b7_eval_posterior (ehvi.hip)
static inline void post_forget(b7_ctx *c) { c->post_valid = false, ++c->epoch; }
// The kept paths of a context, for every caller that wants them: none, the DNGO head's (whatever their age), a GP's of an earlier
// grid, data or covariance kernel, or a GP's of this one.  Every site that changes M, N, dfit or the kernel goes through post_forget,
// so the epoch alone decides; the shapes are compared as well, which costs nothing.  The callers word their own refusals.
enum { TS_STATE_NONE = 0, TS_STATE_BLR, TS_STATE_STALE, TS_STATE_FRESH };
static inline int ts_state(const b7_ctx *c) {
  const TsPaths &t = c->ts;
  if (t.who == TS_NONE) return TS_STATE_NONE;
  if (t.who == TS_BLR) return TS_STATE_BLR;
  return (t.epoch != c->epoch || t.M != c->M || t.N != c->N || t.d != c->dfit) ? TS_STATE_STALE : TS_STATE_FRESH;
}
int feas_write_zeros(b7_ctx *c);                      // L := 0.0 over the resident grid (allocates on demand)
int launch_feas_add(b7_ctx *c, const double *src);    // L[j] += src[j], src: c->M doubles on the device
int launch_feas_best(b7_ctx *c, double *best_val, int64_t *best_idx1);  // score:max(1) of L alone (waits)
int launch_keep_record(b7_ctx *c, uint64_t *tab_dev, int rank, int world);
// the refinement's score pieces (grad<K> beside value<K>).  launch_score_grad: S samples' mean / var [S][M1] and gradients [S][M1][d]
// on the device -> the marginal value [M1] and gradient [M1][d].  launch_refine_step: the same over the 64 query columns, then the
// ladder decision per start, the next 64 query rows, the state and the trace record (refine_step_kernel)
int launch_score_grad(b7_ctx *c, const ScoreParams &p, const double *mu, const double *var, const double *dmu, const double *dvar,
                      int64_t M1, int d, double *value, double *grad);
struct RefStep {
  const double *mu, *var, *dmu, *dvar;  // [S][64], [S][64][d]
  const double *xq;                     // the 64 query rows just evaluated (column = 4 start + rung)
  double *xq_next;                      // the next ones
  RefState *st;
  double *trace;                        // [P][iters + 1][B7_REFINE_TRACE_WIDTH], or null
  const double *lo, *hi;                // the box, d entries each
  int d, P, iter, iters;
  double eta0;
};
int launch_refine_step(b7_ctx *c, const ScoreParams &p, const RefStep &r);
int launch_row_slot(b7_ctx *c, uint64_t *tab_dev, int rank, int world, int64_t idx1_global, int64_t local0, const double *grid,
                    int d);

// comm.hip: the pieces of a sharded nomination that the eval + nominate entry points (nominate_run below),
// b7_score_finish_global and the single-process group (group.hip) are assembled from
int exch_table_ensure(b7_ctx *c, int world);
// enqueue: score:div, local arg-max, this rank's record; pend (nullable): the nomination's batched score, run fused with them
// excl (nullable, with pend): rows kept out of the arg-max (b7_eval_nominate_batch: the rows already picked)
// feas (nullable): the feasibility column weighted in ahead of the arg-max (b7_eval_nominate_feasible), with or without pend
int exch_local(b7_ctx *c, double divisor, int64_t offset, int rank, int world, bool all_slots, bool mirror = false,
               const ScoreParams *pend = nullptr, const ExclRows *excl = nullptr, const double *feas = nullptr);
int exch_wait_mirror(b7_ctx *c);  // after exch_local(..., mirror = true): spin on the completion word, then (or instead, when it takes long) the stream
int exch_fail_record(b7_ctx *c, int rank, int world, int code);  // enqueue: this rank's record says "could not score"
int exch_allreduce(b7_ctx *c);                                   // enqueue: the collective (no-op without a communicator)
// a communicator's end of a nomination after exch_local: failure record if rc says so, all-reduce, fetch, wait, conclude (or
// return rc with this rank's own message)
int exch_collective(b7_ctx *c, int rc, int rank, int world, double *best_val, int64_t *best_idx1);
int exch_rewrite_record(b7_ctx *c, int rank, int world);         // enqueue: zero every record but this rank's (before a repeated all-reduce)
int exch_fetch(b7_ctx *c, int first_rank, int nranks);           // enqueue: records [first, first + n) -> pinned host copy
bool exch_pick(const uint64_t *tab, int world, int stride, double *val, int64_t *idx1, int *rank);
int exch_conclude(b7_ctx *c, const uint64_t *tab, int world, double *best_val, int64_t *best_idx1);  // statuses, winner, cache
void exch_forget(b7_ctx *c);

// gp_api.hip: the pieces of a fit that the nomination and the Bayesian linear head share with the GP entry points
void persist_gave_up(b7_ctx *c);  // a persistent factorisation timed out on a hand-off: the launch schedule from here on
// utils/math.lua:159-218 on c->K: plain attempt, then the growing-jitter retries; leaves L and dinv (+ Linv) on the device
int chol_with_jitter(b7_ctx *c, double *jitter_out, int *info_first_out, bool with_inverse, FactorNote *note = nullptr);
int check_hyp(b7_ctx *c, const b7_hyp *hyp, int d);
void launch_resid_batch(b7_ctx *c, int B, const double *mean_dev);  // c->bresid[b] = Y - mean[b] (padding rows zero), B fits
int fit_front(b7_ctx *c, const b7_hyp *hyp, const double *ls_dev);  // residual, observation scaling and K(X,X) of one hyper sample
int fit_hyp_core(b7_ctx *c, const b7_hyp *hyp, double *nll_out, double *jitter_used, int *info_out, bool then_predict);
// nll_grad.hip: the gradient of the context's fit and its copy to pinned memory, enqueued (fit_hyp_core's hook, c->grad_hook)
int nll_grad_enqueue(b7_ctx *c);
int64_t predict_chunk(const b7_ctx *c, int64_t M);  // candidate rows per pass of predict_into: what c->ks has to hold
int predict_into(b7_ctx *c, const FitSet &fit, const double *xq, int64_t M, double *mu, double *var);  // one fit, host scalars
// mean (M x cols) / variance (M) to the caller (either may be null), then one synchronisation if either was asked for, or `wait`
int copy_out_mu_var(b7_ctx *c, const void *mu, const void *var, int64_t M, int cols, double *mean_host, double *var_host,
                    bool wait = false);

// The packed hyper block of B fits over d dimensions: [B x d lengthscales | B amp | B noise | B mean]
struct HypPack { double *ls, *amp, *noise, *mean; };
static inline HypPack hyp_pack(void *base, int B, int d) {
  double *amp = static_cast<double *>(base) + (size_t)B * d;
  return {static_cast<double *>(base), amp, amp + B, amp + 2 * (size_t)B};
}
// The batch slots (c->bw ... c->bresid) sized for B fits of the resident data, the groups named by `groups`, in this order
constexpr int B7_SLOTS_OPERANDS = 1;  // bw, bzsc, bzss
constexpr int B7_SLOTS_LINV = 2;      // bLinv
constexpr int B7_SLOTS_ALPHA = 4;     // balpha
constexpr int B7_SLOTS_FACTOR = 8;    // bK, bL, bdinv, bresid: what a factorisation outside the one-launch fit works in
int batch_slots_ensure(b7_ctx *c, int B, int groups);
// the S fits in the batch slots, their scalars in the packed hypers of c->bhyp
static inline FitSet batch_fits(const b7_ctx *c, int S) {
  const HypPack hd = hyp_pack(c->bhyp.p, S, c->dfit);
  FitSet f;
  f.w = (const double *)c->bw.p, f.zsc = (const double *)c->bzsc.p, f.zss = (const double *)c->bzss.p;
  f.Linv = (const double *)c->bLinv.p, f.alpha = (const double *)c->balpha.p;
  f.S = S, f.Npad = c->Npad, f.dpad = c->dpad;
  f.amp_dev = hd.amp, f.noise_dev = hd.noise, f.mean_dev = hd.mean;
  return f;
}
// sample s of a set on its own, its scalars taken from the host's copy of that sample's hypers
static inline FitSet fit_at(const FitSet &set, int s, const b7_hyp &hyp) {
  const int Npad = set.Npad, dpad = set.dpad;
  FitSet f;
  f.Npad = Npad, f.dpad = dpad;
  f.w = set.w + s * FitSet::s_w(Npad, dpad), f.zsc = set.zsc + s * FitSet::s_zsc(Npad, dpad), f.zss = set.zss + s * FitSet::s_zss(Npad, dpad);
  f.Linv = set.Linv + s * FitSet::s_Linv(Npad, dpad), f.alpha = set.alpha + s * FitSet::s_alpha(Npad, dpad);
  f.amp = hyp.amp, f.noise = hyp.noise, f.mean = hyp.mean;
  return f;
}

// nominate.hip: bayesopt:eval as stream work without a host wait (its batched score left in *pend), the pivot reports' check and
// the per-sample redo
int nominate_args(b7_ctx *c, const char *who, const b7_score_spec *spec, int64_t offset);
int stage_fmin(b7_ctx *c, const double *fmin, double **fd_out);
static inline bool score_needs_fmin(int kind) { return kind == B7_SCORE_EI || kind == B7_SCORE_LOGEI || kind == B7_SCORE_LOGPI; }
// what a score of this kind leaves in an accumulator: a linear sum (EI, CB, MES) or a log-sum-exp (LogEI, LogPI)
constexpr int score_acc_kind(int kind) { return (kind == B7_SCORE_LOGEI || kind == B7_SCORE_LOGPI) ? B7_ACC_LOG : B7_ACC_LINEAR; }
static inline const char *score_kind_name(int kind) {  // for the messages
  return kind == B7_SCORE_EI ? "ei" : kind == B7_SCORE_LOGEI ? "logei" : kind == B7_SCORE_LOGPI ? "logpi" : kind == B7_SCORE_MES ? "mes" : "cb";
}
// ehvi.hip: the nomination of n = 2 or 3 objectives, linear or in log space, over the kept posteriors of o[0 .. n - 1] (o[0] takes
// the accumulator and the messages, which name the call as `who`); the four b7_[log]ehvi[3]_nominate entries are this.
int ehvi_nominate(b7_ctx *const *o, int n, bool log, const char *who, const double *front, int P, const double *ref, double *best_val,
                  int64_t *best_idx1);
// ehvi3.hip: what that driver needs of three objectives.  Staged3: what the three-objective kernels read of a front, on the host: the
// cuts of the three objectives one after the other and the boxes as table rows.  launch_ehvi3: the score of M rows onto out (device),
// on c's stream; `st` must outlive its copies.
int front3_refuse(b7_ctx *c, const char *who, const double *front, int P, const double *ref);
int samples3_refuse(b7_ctx *c, const char *who, const int *S);
struct Staged3 {
  std::vector<double> cuts;
  std::vector<int> box;
  int ncut[3], rows, B;
};
void stage3_host(const double *front, int P, const double *ref, Staged3 *st);
int launch_ehvi3(b7_ctx *c, bool log, const double *const *mu, const double *const *var, const int *S, const Staged3 &st, int64_t M, double *out);
// ehvi.hip: what ts_hvi.hip shares with the two-objective nomination: the front's check (messages named `who`)
int front_refuse(b7_ctx *c, const char *who, const double *front, int P, const double *ref);
// context.hip: the streams of a call's contexts o[0 .. n - 1] ordered around the work o[0]'s stream does on the others' buffers
int streams_order(b7_ctx *const *o, int n, bool before);
// mes.hip: c->ystar laid out for S samples of M rows at K levels; y* of nS samples (sample s at mu / var + s * stride) searched into
// slots [slot0, slot0 + nS) of that layout, R + 1 launches; the device address of a slot's K values
int mes_begin(b7_ctx *c, int S, int64_t M, int K);
int launch_mes_search(b7_ctx *c, const double *mu, const double *var, int64_t stride, int nS, int slot0);
const double *mes_ystar_dev(const b7_ctx *c, int slot);
// what MES does not do yet, each answered B7_ERR_UNSUPPORTED with the case named: a sharded grid (y* over shards needs R more
// all-reduces) and fantasies (more than one response column)
int mes_refuse(b7_ctx *c, const char *who, const b7_score_spec *spec);
// a score's parameters from its spec; fd: f_min staged on the device (stage_fmin), or null with the one column's f_min in c->fmin_scalar
ScoreParams score_params(const b7_ctx *c, const b7_score_spec *spec, const double *fd);
// the acquisition of c->mu / c->var over the resident candidates into c->acc: added (score:add) or, for a single model, written
int score_add(b7_ctx *c, const b7_score_spec *sp, const double *fd, bool accumulate = true);
// (kind MES: the y* search of the S samples is enqueued here, ahead of the score that reads it)
int pending_score(b7_ctx *c, int S, const b7_score_spec *spec, const double *fd, ScoreParams *out);
int eval_validate(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, int64_t offset);
// eval_enqueue picks one of four routes.  Where the fits of all S samples can run side by side (the one-launch small fit, or S > 1
// single-column fits within the persistent schedule's size) they are produced straight into the batch slots, batch_fits(c, S), and
// the posterior follows as the one-kernel small posterior, as K* / variance / score of all samples in one launch each when K* fits
// the workspace S times over, or else sample by sample through predict_into(c, fit_at(batch_fits(c, S), s, hyps[s]), ...).
// Otherwise every sample is fitted in the context's own slot, one after the other, and predicted from ctx_fit(c).
// keep (nullable; b7_eval_nominate_batch, b7_eval_nominate_refine): where every sample's posterior mean and variance over the
// grid are left, and a view of the S fits, for what follows the first pick.  The enqueued work is the same with and without it,
// copies aside: a route that fits in the context's own slot copies each fit to its batch slot (S == 1: it stays, fits = ctx_fit(c)).
struct BelKeep {
  double *mu = nullptr, *var = nullptr;  // [S][M]; mu == nullptr: not kept (b7_eval_nominate_refine reads the fits alone)
  FitSet fits;                           // out: the S fits afterwards (only the pointers are meant: the scalars travel with the caller's hypers)
  bool want_alpha = false;               // copy alpha into its batch slot where a fit does not live there yet (the believer does not read it)
};
int eval_enqueue(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, ScoreParams *pend, BelKeep *keep = nullptr);
bool reports_clean(b7_ctx *c, const int *reports, int S, bool persist);
int eval_redo(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, double *jitter_out, int *info_out,
              BelKeep *keep = nullptr);
// batch.hip: the believer pass of sample s = blockIdx.z over rows x of xq (rows of them).  column: out kcol[s][Npad] = k(X, x_j)
// (xq = the raw observations) and the believed row's scalars; else the downdate of var[s] and the store of u_j[s] (see batch.hip)
struct BelPass {
  const double *xq; int64_t rows;      // candidate rows (or the N observations)
  const double *xj;                    // the believed point: one raw row of d entries
  const double *w, *zsc, *zss;         // the S fits (strides dpad, Npad dpad, Npad)
  const double *wj;                    // [S][Npad] inv(K_s) k_s(X, x_j); unused by the column pass
  const double *par;                   // [S][2] amp, noise + jitter
  double *scal;                        // [S][1 + B7_BATCH_MAX] t_j, u_i(x_j)
  double *kcol;                        // column pass: [S][Npad] out
  double *var, *u; int64_t sgrid;      // downdate: var[s][M] in/out, u[i][s][M] (i < j read, i = j written); sgrid = M
  int64_t idx; int j;                  // the believed row (0-based), the number of earlier believer columns
};
int launch_believer(b7_ctx *c, int S, const BelPass &p, bool column);
// rff.hip: path j = 0 .. q - 1 in order, each its first minimum over the rows of paths (M x q) that no earlier path took, a NaN never
// winning, into pmin[j] / taken[j] (0-based) on the device; part: 16 nblk bytes of workspace, nblk <= 1024 blocks per pass
int launch_ts_argmins(b7_ctx *c, const double *paths, int64_t M, int q, double *pmin, long long *taken, ArgBest *part, int nblk);
// what the last successful GP b7_ts_nominate / b7_ts_paths left on the device for the paths' refinement (ts_refine.hip): the draws
// (omega [ns][F][d], phase [F], weight [q][F]), sample s's alpha columns at alpha + s alpha_stride ([Npad][yld], yld = 1 or the
// sample's columns rounded up to 64; column p is v_j of path j = s + S p).  B7_ERR_STATE if
// the buffers are not the ones that call left
struct TsKept {
  const double *omega, *phase, *weight, *alpha;
  int64_t alpha_stride;
  int ns;
};
int ts_kept(const b7_ctx *c, TsKept *k);
// ... and path j's alone, over the rows not in taken[0 .. j) (ts_hvi.hip's fallback pick)
int launch_ts_argmin(b7_ctx *c, const double *paths, int64_t M, int q, int j, double *pmin, long long *taken, ArgBest *part, int nblk);
// blr_api.hip: what b7_blr_ts_nominate (blr_ts.hip) shares with the DNGO entry points
int blr_upload_net(b7_ctx *c, const b7_mlp *net, int *z_out);
int blr_feat_alloc(b7_ctx *c, int64_t M, int z);
int blr_heads_fast_enqueue(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap,
                           const double *bt, const double *mn, int z, bool want_terms, double **hdev_out);
// grid_api.hip
int grid_drop_row(b7_ctx *c, int64_t local_idx1, double *row_out_sync);  // stable deletion, enqueued; row_out != NULL synchronises

// The protocol of the three eval + nominate entry points, once.  rc: their argument checks.  enqueue(&pend): the local
// bayesopt:eval as stream work, its batched score possibly left pending; clean(): after the stream has drained, did every fit
// factor at the first attempt; redo(): the same nomination again, synchronously, through the jitter schedule.  The redo starts
// from nothing pending: what the failed fits left is dropped with them.  feas (nullable; one rank only): the feasibility column
// that b7_eval_nominate_feasible weights in ahead of the arg-max, on the first pass and on the redo alike.
template <class Enqueue, class Clean, class Redo>
static inline int nominate_run(b7_ctx *c, const char *who, int rc, int64_t offset, double divisor, Enqueue enqueue, Clean clean,
                        Redo redo, double *best_val, int64_t *best_idx1, const double *feas = nullptr) {
  const int world = c->comm ? c->comm_world : 1, rank = c->comm ? c->comm_rank : 0;
  ScoreParams pend;
  if (!(c->comm && c->comm_world > 1)) {
    // the arg-max and the copy of its record are enqueued before the host has seen any report: one synchronisation
    B7_TRY(rc);
    B7_TRY(enqueue(&pend));
    B7_TRY(exch_local(c, divisor, offset, rank, world, true, true, &pend, nullptr, feas));  // record mirrored into mapped host memory
    B7_TRY(exch_wait_mirror(c));
    if (!clean()) {
      B7_TRY(redo());
      B7_TRY(exch_local(c, divisor, offset, rank, world, true, true, nullptr, nullptr, feas));
      B7_TRY(exch_wait_mirror(c));
    }
    return exch_conclude(c, c->tab_host, world, best_val, best_idx1);
  }
  // with a communicator the collective comes after the report check (a rank that redoes its nomination must not
  // issue one collective too many), and a rank that fails locally still reaches it, with a failure record
  if (rc == B7_OK && c->M > 0) {
    rc = enqueue(&pend);
    if (rc == B7_OK) rc = hipStreamSynchronize(c->stream) == hipSuccess ? B7_OK : b7_fail(c, B7_ERR_HIP, "%s: stream failed", who);
    if (rc == B7_OK && !clean()) {
      pend = ScoreParams();
      rc = redo();
    }
  }
  if (rc == B7_OK) rc = exch_local(c, divisor, offset, rank, world, true, false, &pend);
  return exch_collective(c, rc, rank, world, best_val, best_idx1);
}
