/*
 * bot7hip.h -- C ABI of libbot7hip.so: the MI355X (gfx950) implementation of bot7's GP-posterior +
 * acquisition-scoring hot path.
 *
 * The reference (montyhall/bot7, Lua/Torch7) has no FFI on this path: the "interface" a replacement
 * must honour is the Lua class protocol of bot7.grids / bot7.models / bot7.scores.  Each entry point
 * below names the reference method(s) whose arithmetic it replaces (paths relative to the reference
 * root).  The LuaJIT `ffi.cdef` of exactly these declarations and the three shim classes that call
 * them are in lua/ and INTEGRATION.md; tests and bench drive the same symbols through ctypes.
 *
 * Conventions
 *   - every function returns int: B7_OK (0) or a negative B7_ERR_*; nothing throws or aborts across the
 *     boundary; b7_last_error(ctx) gives the message of the last failure on that context;
 *   - all pointers are HOST pointers to contiguous row-major binary64 (int64_t for indices), owned by the
 *     caller and only touched during the call; "nullable" outputs may be NULL;
 *   - device memory is owned by the opaque context; one context = one GPU = one host thread at a time
 *     (the multi-GPU layout is one process per GPU, each with its own context);
 *   - calls are synchronous unless stated; row/candidate indices that cross the boundary are 1-BASED
 *     (Torch convention, bots/bayesopt.lua:96).
 */
#ifndef BOT7HIP_H
#define BOT7HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B7_ABI_VERSION 1

#define B7_OK 0
#define B7_ERR_INVALID (-1)     /* bad argument (shape, range, NULL) */
#define B7_ERR_HIP (-2)         /* HIP runtime failure; message holds hipGetErrorString */
#define B7_ERR_NOMEM (-3)       /* device allocation failed */
#define B7_ERR_STATE (-4)       /* call order: e.g. predict before fit, score before predict */
#define B7_ERR_UNSUPPORTED (-5) /* valid in the reference, not built yet (see DESIGN.md "out of scope") */
#define B7_ERR_RANGE (-6)       /* Sobol: dims >= 40 or index beyond 2^30-2 (grids/sobol.lua:36,317-324) */
#define B7_ERR_COMM (-7)        /* RCCL: library not loadable, or a communicator call failed */

typedef struct b7_ctx b7_ctx;

/* ---- context ---------------------------------------------------------------------------------- */
int b7_abi_version(void);
int b7_create(b7_ctx **out, int device_id);
void b7_destroy(b7_ctx *ctx);
const char *b7_last_error(const b7_ctx *ctx);
/* name_out: >= 64 bytes, nullable. */
int b7_device_info(b7_ctx *ctx, char *name_out, int *compute_units, int64_t *hbm_bytes);
int b7_sync(b7_ctx *ctx);

/* Bytes of the K(X*,X) chunk workspace (default 4 GiB); candidates are processed in chunks of
 * workspace / (8 * Npad) rows.  Must be set before the first predict. */
int b7_set_workspace(b7_ctx *ctx, int64_t bytes);

/* ---- grids: bot7.grids.sobol / bot7.grids.random ---------------------------------------------- */

/* grids/sobol.lua:58-90 generate + :216-335 i4_sobol.  Row j (1-based) is Sobol point number
 * j + skip - 1 (Gray-code order, 30 bits), then x*(maxes-mins)+mins as two rounded ops (:79-81);
 * mins/maxes both NULL = no affine map; mins only: x + (mins + column minimum) (:82-83, as the reference writes it);
 * maxes only: x * (maxes / column maximum) (:84-85) -- the column extremes are those of the WHOLE grid: a context with a
 * communicator combines them across ranks (one all-reduce of d doubles; collective).  The grid stays resident on the
 * device as THE candidate set; out_host (nullable, size x dims) receives a copy.  dims must be < 40 (:36).  A rank that
 * owns rows [lo, hi) of a global grid calls this with size = hi-lo and skip = global_skip + lo. */
int b7_grid_sobol(b7_ctx *ctx, int64_t size, int dims, int64_t skip, const double *mins, const double *maxes,
                  double *out_host);

/* Host-only: the scaled direction numbers V[i][b] = m_(b+1) * 2^(29-b) (i < dims <= 39, b < 30) that
 * grids/sobol.lua:243-289 builds in self.bank; out has dims*30 entries.  Needs no context and no GPU. */
int b7_sobol_direction_numbers(int dims, uint32_t *out);

/* grids/random.lua:23-35 with torch.rand replaced by a counter-based generator (Torch's MT19937 stream
 * is not part of the reference tree): u(row, col) = top 53 bits of splitmix64(seed, row_offset+row, col)
 * scaled by 2^-53, then the same affine map.  Any dims. */
int b7_grid_random(b7_ctx *ctx, int64_t size, int dims, uint64_t seed, int64_t row_offset, const double *mins,
                   const double *maxes, double *out_host);

/* grids/random.lua:23-35 with torch.rand's OWN stream, for replaying a reference run point for point: Torch7's CPU generator
 * is MT19937 seeded by torch.manualSeed(seed) (TH/THRandom.c; not part of the reference tree, restated from its published
 * algorithm: parity unpinned).  resolution 32: a double is random() * 2^-32 (Torch7 of bot7's era); 53: the later
 * (random64() & (2^53 - 1)) * 2^-53.  The stream is sequential, so the uniforms are made on the host and uploaded; the
 * affine map (both / one / none of mins, maxes) runs on the device as for b7_grid_random.  No row_offset: a rank that owns
 * rows [lo, hi) of a grid made this way generates the whole stream and uploads its slice (b7_torch_rand + b7_grid_upload). */
int b7_grid_random_torch(b7_ctx *ctx, int64_t size, int dims, uint64_t seed, int resolution, const double *mins,
                         const double *maxes, double *out_host);
/* Host-only: n doubles of that stream (what torch.manualSeed(seed); torch.rand(n) returns). */
int b7_torch_rand(uint64_t seed, int64_t n, int resolution, double *out);

/* The pieces of the one-sided maps, for callers that combine shards themselves: grid:min(1) / grid:max(1) of the resident
 * grid (both nullable, d entries), and the map itself given the extremes of the whole grid (exactly one of mins / maxes). */
int b7_grid_colrange(b7_ctx *ctx, double *col_min, double *col_max);
int b7_grid_apply_onesided(b7_ctx *ctx, const double *mins, const double *maxes, const double *col_ext);

/* The trust-region map (TuRBO: Eriksson et al., NeurIPS 2019; no counterpart in the reference): maps the resident grid IN PLACE.
 * Its entries are taken as base points u in [0, 1), as b7_grid_sobol / b7_grid_random / b7_grid_random_torch leave them without
 * mins / maxes; the result is a candidate set inside the box [lo, hi] around `center`.  Per element (row i, column k), with
 * g = row_offset + i, in this order:
 *   rotation (Cranley-Patterson; only with `shift`, 0 <= shift[k] < 1):  t = u + shift[k]; if (t >= 1.0) t -= 1.0;
 *   mask:   perturbed iff counter_uniform(counter_key(seed, 0), g d + k) < prob, or k == f(g),
 *           f(g) = min(d - 1, (int)(counter_uniform(counter_key(seed, 1), g) * d))        (the generator of csrc/counter_rng.h)
 *   value:  perturbed: x = t * (hi[k] + (-lo[k])); x = x + lo[k]  (two rounded operations), clamped into [lo[k], hi[k]];
 *           otherwise x = center[k], bit for bit.
 * Column f(g) of EVERY row is perturbed.  Eriksson et al. force a column only when the draw perturbed none of the row; here an
 * element is a pure function of (seed, g, k), so nothing is reduced across a row and nothing depends on M or on how rows are split
 * between calls: a shard passes its first row's global number as row_offset, as for b7_grid_random.
 * Synchronous; drops predictions, accumulator, feasibility column and kept posterior as every grid change does.  A local call: a
 * communicator of any size is no obstacle and nothing is exchanged.  B7_ERR_STATE: no grid; a member of a group.  B7_ERR_INVALID: a
 * NULL center / lo / hi, a non-finite entry, lo[k] > hi[k], a center outside [lo, hi], prob outside [0, 1], a shift outside
 * [0, 1), a negative row_offset.  Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_grid_trust_region(b7_ctx *ctx, const double *center /*d*/, const double *lo /*d*/, const double *hi /*d*/, double prob,
                         const double *shift /*d, nullable*/, uint64_t seed, int64_t row_offset);

/* A caller-made grid (cache.candidates, bots/abstract.lua:30). */
int b7_grid_upload(b7_ctx *ctx, const double *X_hid, int64_t M, int d);
int b7_grid_download(b7_ctx *ctx, int64_t row0 /*0-based*/, int64_t rows, double *out_host);
int b7_grid_shape(b7_ctx *ctx, int64_t *M, int *d);

/* utils/tensor.lua:158-170 remove, as used by steal (:175-193) from bots/abstract.lua:118: stable
 * deletion of candidate row idx1 (1-based); later rows shift up by one.  row_out (nullable, d) gets the
 * removed row (what steal appends to `pending`). */
int b7_grid_remove(b7_ctx *ctx, int64_t idx1, double *row_out);
/* The same for an index list, as utils.tensor.remove / steal accept (utils/tensor.lua:158-193: `idx` is a
 * LongTensor): the rows named by idx1[0..n) (1-based, against the grid BEFORE the call; duplicates count once,
 * keep:indexFill is idempotent) are deleted in one stable pass.  rows_out (nullable, n x d) = src:index(1, idx),
 * in the order given. */
int b7_grid_remove_rows(b7_ctx *ctx, const int64_t *idx1, int64_t n, double *rows_out);

/* ---- model: gp_regressor + ardse | ardmatern52 + GaussianNoise_iso + constant mean (bots/bayesopt.lua:40-43) - */

/* Replaces the table model:parse_hypers returns (bots/bayesopt.lua:75).  lenscale_sq[k] is what
 * utils.math.pdist receives as `lenscale` (it divides squared differences, utils/math.lua:72). */
typedef struct {
  const double *lenscale_sq; /* d entries, > 0 */
  double amp;                /* signal variance sigma_f^2 */
  double noise;              /* sigma_n^2 added to diag K(X,X) */
  double mean;               /* constant mean m */
} b7_hyp;

/* Choices the reference leaves to the absent `gp` package, made explicit (defaults in brackets). */
typedef struct {
  double jitter_eps;    /* [1e-8]  utils/math.lua:175 */
  double jitter_growth; /* [1.1]   utils/math.lua:176 */
  int var_with_noise;   /* [0] add `noise` to the predictive variance */
  int var_clamp;        /* [0] clamp variance below at var_min (TH clamp: NaN passes) */
  double var_min;       /* [0.0] */
} b7_gp_opts;
int b7_gp_default_opts(b7_gp_opts *out);
/* The options of the calls that FOLLOW.  What earlier calls left stays as they made it: the predictions of b7_gp_predict, the score
 * accumulator and a kept posterior (b7_eval_posterior) hold the variance under the options in force when they were computed, and
 * are served as such (a caller that changes var_with_noise / var_clamp between b7_eval_posterior and b7_ehvi_nominate scores the
 * earlier variance). */
int b7_gp_set_opts(b7_ctx *ctx, const b7_gp_opts *opts);

/* The covariance kernel (bots/bayesopt.lua:41 config.model.kernel; the kernels themselves live in the absent `gp` package).
 * With D = sum_k (x_k - z_k)^2 / lenscale_sq_k, the same distance for both, and the same b7_hyp layout:
 *   B7_KERNEL_ARDSE      K = amp * exp(-D/2)                                 (the default)
 *   B7_KERNEL_MATERN52   K = amp * (1 + s + s^2/3) * exp(-s),  s = sqrt(5 D)  (ARD Matern-5/2, Snoek et al. 2012)
 * Every entry point below that forms a covariance uses the context's kernel; k(x, x) = amp under both.  Context state, not a
 * field of the hyper or option structs above (hosts allocate those): a context that never calls this stays on ARD-SE.  Setting a DIFFERENT
 * kernel drops the fit and the predictions made from it (predict, fantasize, append and download answer B7_ERR_STATE until the
 * next fit) and a kept posterior (b7_eval_posterior: b7_posterior_get and the EHVI nominations answer B7_ERR_STATE until the
 * next one); the resident data and grid stay, and so does the score accumulator (the last call's result).  Setting the current
 * one again does nothing.  Unknown values: B7_ERR_INVALID.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_KERNEL_ARDSE 0
#define B7_KERNEL_MATERN52 1
int b7_gp_set_kernel(b7_ctx *ctx, int kernel);

/* The arithmetic of model:predict's first half (call sites scores/expected_improvement.lua:63,
 * scores/confidence_bound.lua:63): K = amp*exp(-pdist(X,X,lenscale_sq)/2) + noise*I with the distance of
 * utils/math.lua:65-111 (the ARD-SE form: K is the context's kernel, b7_gp_set_kernel above); L = chol(K) with the jitter schedule of utils/math.lua:159-218 (eps <- eps*growth
 * added to the ORIGINAL diagonal until success, or chol(I) once eps > ||K||_F); alpha = K^-1 (Y - mean).
 * X_obs N x d (d <= 96), Y_obs N x ycols (ycols <= 256: fantasy columns share K, L and differ only in alpha).
 * Outputs (all nullable): nll_out[ycols] negative log marginal likelihood,
 * jitter_used (0 = none, -1 = fell back to chol(I)), info = 1-based first failing pivot (not > 0, NaN, or below
 * the smallest normal double) of the FIRST
 * attempt (0 = positive definite). */
int b7_gp_fit(b7_ctx *ctx, const double *X_obs, const double *Y_obs, int N, int d, int ycols, const b7_hyp *hyp,
              double *nll_out, double *jitter_used, int *info);

/* The same in two steps, for the regime Bayesian optimisation lives in: model:sample_hypers (bots/bayesopt.lua:68,
 * 73-75) drives samplers/slice.lua:92-168, whose every density evaluation refits the SAME (X_obs, Y_obs) under new
 * hypers.  b7_gp_set_data puts the data on the device once; b7_gp_fit_hyp then uploads d + 3 numbers per fit (the
 * residual Y - mean is formed on the device).  b7_gp_fit == b7_gp_set_data + b7_gp_fit_hyp, bit for bit. */
int b7_gp_set_data(b7_ctx *ctx, const double *X_obs, const double *Y_obs, int N, int d, int ycols);
int b7_gp_fit_hyp(b7_ctx *ctx, const b7_hyp *hyp, double *nll_out, double *jitter_used, int *info);

/* model:predict(X_obs, Y_obs, X_hid, hyp, {mean, var}) in ONE call for resident data and a resident grid
 * (scores/expected_improvement.lua:63 fits and predicts in one breath): b7_gp_fit_hyp + b7_gp_predict with the posterior
 * enqueued right behind the fit, so the host waits for the pivot report only and never idles the GPU between the two
 * (a failed plain attempt redoes the prediction after the jitter schedule).  Results as b7_gp_fit_hyp / b7_gp_predict;
 * every output is nullable. */
int b7_gp_predict_hyp(b7_ctx *ctx, const b7_hyp *hyp, double *mean_host, double *var_host, double *nll_out,
                      double *jitter_used, int *info);

/* B likelihood evaluations of the resident data at once: the slice sampler's step-out / step-in probes
 * (samplers/slice.lua:118-164) and multi-chain samplers ask for the density at several hyper vectors per update.
 * lenscale_sq is B x d row-major; amp / noise / mean have B entries; nll_out[B] as b7_gp_fit_hyp's (same jitter schedule
 * per fit: jitter_out[B] / info_out[B], nullable).  N <= 128 observations with d <= 32 -- the reference's own regime
 * (budget 100, bots/abstract.lua:64), where a trial is hundreds of sequential density evaluations against one nomination --
 * take ONE workgroup of ONE launch per evaluation (observations in, two numbers out through device-mapped pinned memory: no
 * copy calls; B = 1 carries its hypers in the kernel arguments and waits on a completion word instead of the stream:
 * 24 us per call up to N = 64, 43 us up to 128; a batch of up to 256 costs ~7 us more).  Larger problems: the B
 * factorisations run concurrently in ONE persistent launch (each a chain of workgroups; 28 fit on the chip at N <= 256, 7 at
 * N <= 512, larger ones go one after the other), with L z = r solved alongside: no inverse, no alpha.  The context's current fit (and its predictions) is left untouched -- except
 * when a fit's hand-offs time out twice (the GPU is shared with another persistent kernel): that likelihood is then
 * evaluated through the launch schedule in the context's fit slot, and the next predict asks for a new fit (B7_ERR_STATE).
 * One response column, N <= 4096. */
int b7_gp_nll_batch(b7_ctx *ctx, int B, const double *lenscale_sq, const double *amp, const double *noise,
                    const double *mean, double *nll_out, double *jitter_out, int *info_out);

/* THE SLICE SAMPLER'S HYPER CHAIN ON THE DEVICE: C chains of U updates each in ONE launch, one workgroup per chain -- the
 * control flow of samplers/slice.lua:51-168 and the likelihood evaluation loop inside the kernel, so a trial's 46-74 sequential
 * density evaluations cost one launch and one host wait instead of one each.  No counterpart in the reference's call
 * structure; the same decisions: the default mode -- random direction (:78-86), log space, step-out, per-dimension widths,
 * max_step -- over the density  -NLL(exp(theta_1..d+2), theta_d+3)  with a flat prior inside [lo, hi]:
 *   theta = [log lenscale_sq_1..d, log amp, log noise, mean], d + 3 components; theta0 is C x (d + 3), the chains' start points.
 *   A theta with a component outside [lo, hi] or not finite has density -inf and is not evaluated.  An update after the first
 *   of a call starts from the value of the point the last one ended on without evaluating it again.
 *   Every evaluation is b7_gp_nll_batch's, bit for bit: the value is -(0.5 t0 + t1 + c0) of the same two terms.
 * Runs over the resident data (b7_gp_set_data) under the context's covariance kernel (b7_gp_set_kernel), N <= 128, d <= 32, one
 * response column.  The context's current fit, its predictions, the grid and the score accumulator are untouched.
 * Draws: the library's counter generator.  Chain c of a call draws from the stream key(seed, c); update number g = update0 + u
 * owns the counters 4096 g .. 4096 g + 4095:  4096 g + k (k < d + 3) the direction's normal z_k;  4096 g + 64 the uniform u_Y of
 * the slice level Y = f(x0) + log(u_Y);  4096 g + 128 + k the uniforms of `right`;  4096 g + 256 + i the uniform of shrink step i.
 * A draw depends on (seed, chain, g) alone: U updates in one call are U calls of one update chained through theta_out and
 * update0, and chain c's samples do not depend on C.
 * Every loop is bounded: step-outs by max_step, the density requests of one update (the start point's included, evaluated or
 * not) by max_evals.  status_out, per (chain, update), is a bit mask:
 *   1   a NaN density was met: as the reference does (:138-141), the update stops shrinking and takes the point
 *   2   the slice shrank to zero (:146-149): the reference's behaviour, the point is taken
 *   4   max_evals was reached: the update returns the point it started from
 *   8   a likelihood's plain factorisation reported a failed pivot: the chain stops -- this update and all later ones return
 *       the chain's last good theta.  The kernel never runs the jitter schedule; the call still returns B7_OK and the caller
 *       decides (the models finish such a chain through the host sampler, whose evaluations carry the schedule)
 *   16  the update was not run (it follows one with bit 8)
 * theta_out C x U x (d + 3), value_out C x U (the density at theta_out; NaN where none is known), nevals_out[C] the likelihood
 * evaluations the chain ran.
 * B7_ERR_STATE: no resident data.  B7_ERR_UNSUPPORTED, the case named: N > 128, d > 32, more than one response column (Gibbs
 * updates and linear space are not built: the bindings answer those by name).  B7_ERR_INVALID: NULL arguments, C outside
 * 1..B7_SLICE_MAX_CHAINS, U < 1, max_evals outside 1..B7_SLICE_MAX_EVALS, U * max_evals > B7_SLICE_MAX_WORK, max_step < 0,
 * d + 3 > 64, a width <= 0, lo > hi.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_SLICE_MAX_CHAINS 256
#define B7_SLICE_MAX_EVALS 3840
#define B7_SLICE_MAX_WORK 65536
int b7_gp_slice_sample(b7_ctx *ctx, int C, int U, const double *theta0 /*C x (d+3)*/, const double *lo, const double *hi,
                       const double *widths /*d+3 each*/, int max_step, int max_evals, uint64_t seed, uint64_t update0,
                       double *theta_out /*C x U x (d+3)*/, double *value_out /*C x U*/, int *status_out /*C x U*/,
                       int *nevals_out /*C*/);
/* Inspection (tests, cost tools): with records_per_chain > 0 every later b7_gp_slice_sample keeps, per chain, its first
 * records_per_chain records of B7_SLICE_TRACE_WIDTH doubles each, in the order the kernel made them; 0 (default) turns it off.
 * A full buffer stops recording and leaves the chain unaffected.  rec[0] is the record's type:
 *   0  an update:   rec[1] g, rec[2] u_Y, rec[3] log u_Y, rec[8 + k] z_k, rec[72 + k] the uniform of right_k      (k < d + 3)
 *   1  a density request:  rec[1] kind (0 start, 1 step-out right, 2 step-out left, 3 shrink), rec[2] the shrink uniform (else
 *      0), rec[3] 1 inside the bounds, rec[4] 1 reused (the known value of the start point), rec[5] the value, rec[6] the
 *      evaluation's length in ticks of the 100 MHz wall clock (0 when nothing was evaluated), rec[7] reserved, rec[8 + k]
 *      theta_k, rec[72 + k] the hyper pack the likelihood body was given (lenscale_sq_1..d, amp, noise, mean; 0 when not evaluated)
 * b7_gp_slice_trace copies chain `chain`'s records of the last traced call (records: room for records_per_chain records,
 * nullable) and their number.  B7_ERR_STATE without one. */
#define B7_SLICE_TRACE_WIDTH 136
int b7_gp_slice_trace_enable(b7_ctx *ctx, int records_per_chain);
int b7_gp_slice_trace(b7_ctx *ctx, int chain, double *records, int *n_records);

/* utils.math.chol(src, 'L') (utils/math.lua:159-218) on a caller-provided symmetric n x n matrix: lower factor
 * with the same jitter schedule as b7_gp_fit.  res_host n x n (upper triangle zero).  Replaces the current fit
 * on this context.  jitter_used / info as in b7_gp_fit (nullable). */
int b7_chol(b7_ctx *ctx, const double *src_host, int n, double *res_host, double *jitter_used, int *info);

/* Second half of model:predict over the resident candidate grid: mean = m + K(X*,X) alpha (M x ycols),
 * var = amp - colsumsq(L^-1 K(X*,X)') (M).  Results stay on the device for the score calls; host copies
 * are optional. */
int b7_gp_predict(b7_ctx *ctx, double *mean_host, double *var_host);

/* model:predict for arbitrary X1 (M1 x d) that is not the resident grid; does not disturb the grid or the
 * score accumulator. */
int b7_gp_predict_at(b7_ctx *ctx, const double *X1, int64_t M1, double *mean_host, double *var_host);

/* model:fantasize(nFantasies, X_obs, Y_obs, X_pend, hyp) (scores/expected_improvement.lua:57; the class is in the
 * absent `gp` package): nFantasies joint draws from the posterior of the CURRENT fit at the P pending points,
 * y = mu_P + chol(Sigma_P) z with Sigma_P = K(Xp,Xp) - K(Xp,X) K^-1 K(X,Xp) (+ noise when var_with_noise) factored
 * with the utils.math.chol jitter schedule.  torch.randn is replaced by a counter-based generator:
 * z(k, s) = Box-Muller of splitmix64(seed, 2(k n + s) + 1 | + 2).  Y_out P x nFantasies; mean_out[P] and
 * cov_out[P x P] (nullable) expose mu_P and Sigma_P.  P <= 64; the fit must have ycols == 1. */
int b7_gp_fantasize(b7_ctx *ctx, const double *X_pend, int P, int nFantasies, uint64_t seed, double *Y_out,
                    double *mean_out, double *cov_out);

/* Incremental refit (bots/abstract.lua:137-144 appends one observation per trial): extends the CURRENT fit by one
 * observation (x_new[d], y_new[ycols]) under the same hypers in O(N^2): l = L^-1 k, lambda^2 = kappa - l'l, new rows
 * of L and L^-1, alpha recomputed.  Returns B7_ERR_STATE when the padded factor is full (N = 64, or a multiple of 128 above) or
 * lambda^2 does not stand clear of the rounding-error bound of its own evaluation,
 * lambda^2 <= (N+2) u (2 |l|'(|L^-1||k|) + l'l), u = 2^-53 (this includes lambda^2 <= 0) -- refit with b7_gp_fit then
 * (which also applies the jitter schedule). */
int b7_gp_append(b7_ctx *ctx, const double *x_new, const double *y_new);

/* Inspection (tests): lower Cholesky factor N x N, alpha N x ycols, explicit inverse factor N x N. */
int b7_gp_download(b7_ctx *ctx, double *L_host, double *alpha_host, double *Linv_host);

/* ---- model: bot7.models.dngo -- basis network + Bayesian linear head (models/dngo.lua:108-175) -------------- */

/* The trained feature extractor as plain arrays: layer l is nn.Linear(dims[l], dims[l+1]) with W[l] row-major
 * dims[l+1] x dims[l] (nn.Linear's weight layout) and bias b[l], each followed by the same activation
 * (0 identity, 1 Tanh, 2 ReLU, 3 Sigmoid); the output of the last listed layer is the basis (self.basis.output,
 * models/dngo.lua:101-105).  1..4 layers, widths <= 256.  Training the network (nnTools.trainer) is out of scope. */
typedef struct {
  int n_layers;
  const int *dims;          /* n_layers + 1 entries */
  const double *const *W;
  const double *const *b;
  int activation;
} b7_mlp;

/* models/dngo.lua:155-171: features by a forward pass.  X == NULL: the resident candidate grid, features stay on
 * the device for b7_blr_predict (Z_host nullable, M ignored).  X != NULL: M x dims[0] host rows, Z_host M x z. */
int b7_blr_basis(b7_ctx *ctx, const b7_mlp *net, const double *X, int64_t M, double *Z_host);
/* Caller-made features for the candidates (M x z) instead of a grid + network. */
int b7_blr_features(b7_ctx *ctx, const double *Z1, int64_t M, int z);
/* gp.models.bayes_linear (absent `gp` package) restated as standard Bayesian linear regression (Bishop 3.3;
 * Snoek et al. 2015): prior precision alpha_prec, noise precision beta, constant mean:
 *   K = beta Z0'Z0 + alpha_prec I,  m = beta K^-1 Z0'(Y0 - mean).  Replaces the GP fit on this context.
 * nll_out (nullable): negative log evidence, for sampling (alpha_prec, beta) on the host ('marginalize'). */
int b7_blr_fit(b7_ctx *ctx, const double *Z0, const double *Y0, int N, int z, double alpha_prec, double beta,
               double mean, double *nll_out);
/* The same with Z0 = basis(X0) computed and kept on the device (models/dngo.lua:155-162 + :174 in one call). */
int b7_blr_fit_x(b7_ctx *ctx, const b7_mlp *net, const double *X0, const double *Y0, int N, double alpha_prec,
                 double beta, double mean, double *nll_out);
/* mean = m0 + Z1 m, var = 1/beta + z' K^-1 z over the resident features; results stay on the device for the
 * b7_score_* calls (same accumulator and arg-max as the GP path). */
int b7_blr_predict(b7_ctx *ctx, double *mean_host, double *var_host);

/* ---- scores: bot7.scores.expected_improvement / confidence_bound + bayesopt marginalisation ---- */

/* bots/bayesopt.lua:69: score = zeros(M). */
int b7_score_reset(b7_ctx *ctx);
/* scores/expected_improvement.lua:69-88 on the last predict, added into the accumulator
 * (bots/bayesopt.lua:76 score:add).  fmin[ycols] = Y_obs:min(1) (:64); tradeoff = xi (:30). */
int b7_score_ei(b7_ctx *ctx, const double *fmin, double tradeoff);
/* scores/confidence_bound.lua:70-106; upper != 0 selects UCB (:96-100) else LCB (:102-106); the result is
 * val if sign > 0 else -val (:89-93); added into the accumulator. */
int b7_score_cb(b7_ctx *ctx, double tradeoff, int upper, double sign);
/* Log-space expected improvement of the last predict -- NO counterpart in scores/ of the reference (Ament et al.,
 * "Unexpected Improvements to Expected Improvement", NeurIPS 2023): with sigma, imprv and z as b7_score_ei forms them and
 * h(z) = phi(z) + z Phi(z),  log EI = log(sigma) + log h(z),  log h = log(phi(z) + z erfc(-z/sqrt2)/2) for z > -1 and
 * -z^2/2 - log(2 pi)/2 + log1p(-t sqrt(pi/2) erfcx(t/sqrt2)), t = -z, below (from t = 1e5 on the log1p term is its own
 * expansion, -2 log t + log1p(-3/t^2): the product rounds to 1 or past it out there): finite and ordered where EI has long
 * underflowed to 0, down to z ~ -1.3e154, and never NaN for finite inputs with var >= 0.  var == 0: log(imprv) for imprv > 0, else -inf; var < 0, NaN: NaN.  The accumulator becomes a running
 * log-sum-exp (empty at -inf): each call folds a <- logaddexp(a, log EI) -- the marginal is log((1/S) sum_s EI_s), not the
 * mean of the logs; ycols > 1 (fantasies): the log of the row mean of EI.  The first add after b7_score_reset decides
 * whether the accumulator is linear (b7_score_ei / _cb) or logarithmic; adding the other kind onto it is B7_ERR_STATE. */
int b7_score_logei(b7_ctx *ctx, const double *fmin, double tradeoff);
/* Log probability of improvement of the last predict -- NO counterpart in scores/ of the reference.  With sigma, imprv and z as
 * b7_score_ei forms them the value is log Phi(z), evaluated so that it neither underflows nor loses the upper tail:
 * log1p(-erfc(z/sqrt2)/2) for z >= 0, log(erfc(-z/sqrt2)/2) for -1 < z < 0, (-z^2/2 - log 2) + log(erfcx(-z/sqrt2)) for z <= -1;
 * finite and ordered down to z ~ -1.3e154 (z^2/2 overflows: -inf), never NaN for finite inputs with var >= 0.  var == 0: 0.0 for
 * imprv >= 0, else -inf; z = +inf: 0.0; z = -inf: -inf; var < 0, var NaN or mean NaN: NaN.  Relative accuracy is not promised where
 * |log Phi| < 1e-300 (z beyond ~37).  As an acquisition it is log-PI; on the GP of a constraint c_k, with fmin = the threshold t_k
 * and tradeoff = 0, it is the log probability of feasibility log Pr[c_k(x) <= t_k] (Gelbart et al. 2014, Gardner et al. 2014; the
 * log-space form of Ament et al. 2023).  The accumulator is a log one, exactly as b7_score_logei's: the marginal is
 * log((1/S) sum_s Phi(z_s)); ycols > 1: the log of the row mean.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_score_logpi(b7_ctx *ctx, const double *fmin, double tradeoff);
/* Max-value entropy search of the last predict -- NO counterpart in scores/ of the reference (Wang & Jegelka, "Max-value
 * Entropy Search for Efficient Bayesian Optimization", ICML 2017): the expected reduction of the entropy of the optimum's VALUE.
 * The library minimises, so the paper's maximum is the minimum y*, and its distribution is that of the minimum over the
 * resident candidates themselves (independent candidates, as in the paper): no sampler, no joint posterior, no random numbers,
 * and no clamp to the incumbent.  Rows of the last predict (mu_j, var_j):
 *   bad    mu or var NaN, or var < 0    score NaN (the first NaN wins the arg-max, as everywhere)
 *   exact  var == 0                     score exactly 0.0
 *   live   the rest, sigma_j = sqrt(var_j); only these take part in the search
 * Search: L(y) = sum_live log Phi((mu_j - y)/sigma_j); y*_k (k = 1..K) is the root of L(y) = log1p(-(k - 1/2)/K), bracketed by
 * lo0 = min_j(mu_j - 10 sigma_j), hi0 = min_j(mu_j + 10 sigma_j) -- s = sqrt(var); t = s * 10; mu - t; mu + t, one rounded operation
 * each, then the minimum, so lo0 / hi0 do not depend on the decomposition -- and narrowed by 10 rounds of 15 interior probes
 * y_p = lo + (hi - lo) p/16 to 16^-10 of the bracket; y*_k is the last bracket's midpoint.  11 launches, no host round trip,
 * bit-reproducible.  No live row: every y*_k is NaN.
 * Score: with g_k = (mu_j - y*_k)/sigma_j and h(g) = g phi(g)/(2 Phi(g)) - log Phi(g),  score_j = (1/K) sum_k h(g_k), added into
 * the (linear) accumulator like b7_score_ei; the marginal over hyper samples is the mean, each sample with its own y*.
 * One response column only (fantasies: B7_ERR_UNSUPPORTED), and no communicator of more than one rank (y* over a sharded grid
 * needs an all-reduce per round: B7_ERR_UNSUPPORTED).  After b7_blr_predict it scores the DNGO head's posterior.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_MES_KMAX 64
int b7_score_mes(b7_ctx *ctx);
/* K of the searches that b7_score_mes and a B7_SCORE_MES nomination start: default 8; outside 1..B7_MES_KMAX: B7_ERR_INVALID. */
int b7_mes_set_levels(b7_ctx *ctx, int K);
/* y* of the last search on this context (b7_score_mes: S = 1; a B7_SCORE_MES nomination: its S samples in order):
 * ystar S x K (nullable), bracket S x 2 = lo0, hi0 per sample (nullable).  B7_ERR_STATE when no search has run. */
int b7_mes_last_ystar(b7_ctx *ctx, int *S, int *K, double *ystar, double *bracket);
/* The search alone on caller-provided host vectors (M mean, M var): ystar[K], bracket[2] = lo0, hi0 (nullable).  It IS a search
 * on this context: afterwards b7_mes_last_ystar reports this one (S = 1, this K), not an earlier nomination's. */
int b7_mes_ystar(b7_ctx *ctx, const double *mean, const double *var, int64_t M, int K, double *ystar, double *bracket);
/* The score alone, with the caller's y*[K]: out[j] = (1/K) sum_k h((mean_j - ystar_k)/sigma_j), row classes as above.  Domain:
 * within 1e-13 max(1, |h|) of exact arithmetic for g >= -8 (a searched y* keeps g >= -2.5); below that the same form -- phi/Phi
 * through erfcx -- stays finite but is not held to that bar.  The caller's y* is kept apart from the context's own: the
 * last search's values (b7_mes_last_ystar) are untouched. */
int b7_mes_compute(b7_ctx *ctx, const double *mean, const double *var, const double *ystar, int K, int64_t M, double *out);
/* bots/bayesopt.lua:79 score:div(nSamples) then :96 score:max(1): best_val and the 1-based index of the
 * first maximum (first NaN wins, as TH's max).  divisor = 1 skips nothing: x/1 is exact.
 * scores_host nullable (M).  On a log accumulator (b7_score_logei) score:div is a - log(divisor), and best_val /
 * scores_host are log EI; the same holds for b7_score_finish_global. */
int b7_score_finish(b7_ctx *ctx, double divisor, double *best_val, int64_t *best_idx1, double *scores_host);

/* ---- multi-GPU: the one exchange of a candidate-sharded nomination (RCCL over xGMI) ------------ *
 * Layout: one process per GPU, each with its own context; rank r owns candidate rows
 * [offset_r, offset_r + M_r) of the global grid (it generates them itself: b7_grid_sobol with skip + offset_r),
 * refits the GP redundantly, accumulates scores locally.  bots/bayesopt.lua:95-96's score:max(1) over ALL
 * candidates is then ONE ncclAllReduce inside b7_score_finish_global / b7_eval_nominate, over a table with one
 * fixed-width record of 64-bit words per rank: (value bits, global 1-based index, failure flag, rows of the shard,
 * the winner's grid row) -- so the same exchange also delivers what bots/abstract.lua:118-121 needs next, the
 * nominee's coordinates, to every rank (b7_nominate_commit), and a rank that could not score its shard makes every
 * rank return an error instead of leaving the others inside the collective.  800 B per rank, latency-bound.
 * librccl is dlopen'ed at the first b7_comm_* call; a context without a communicator is a world of one.
 * (One process driving several GPUs: the b7_group_* calls further down.) */
#define B7_COMM_ID_BYTES 128
/* ncclGetUniqueId: rank 0 makes the id (no context needed) and hands the 128 bytes to the other ranks by whatever
 * channel the host has (a file, an environment variable, a socket). */
int b7_comm_unique_id(void *id_out);
/* ncclCommInitRank on this context's device; collective over all `world` ranks; the exchange runs on the context's
 * stream.  One communicator per context. */
int b7_comm_init(b7_ctx *ctx, int rank, int world, const void *id);
int b7_comm_info(b7_ctx *ctx, int *rank, int *world);
int b7_comm_destroy(b7_ctx *ctx); /* also done by b7_destroy */
/* Control-plane reduction of a few host doubles (n <= 128) over the communicator, in place; also a barrier
 * (every rank returns only after all have entered and the context's stream has drained). */
#define B7_COMM_SUM 0
#define B7_COMM_MAX 1
#define B7_COMM_MIN 2
int b7_comm_allreduce_f64(b7_ctx *ctx, double *inout, int n, int op);
/* Host-only, needs no context and no GPU: the rule every rank applies to the gathered records, here as a [world, 2]
 * table of 64-bit words (value bits, global 1-based index; index 0 = that rank's shard was empty) -- TH's max over the union of the shards:
 * the first NaN wins, else the largest value, ties to the lowest global index.  B7_ERR_STATE when every shard is empty.
 * Exposed so that the rule can be checked for any world size without that many GPUs. */
int b7_comm_pick_winner(const uint64_t *table, int world, double *best_val, int64_t *best_idx1);
/* b7_score_finish across ranks: score:div(divisor) on this rank's shard, local first-maximum on the device, the
 * (value, global 1-based index = global_row_offset + local index) pairs of all ranks exchanged by one all-reduce,
 * and on every rank the same winner by TH's rule (first NaN, else max, ties to the lowest global index): exactly
 * what score:max(1) returns on the unsharded vector.  A rank whose shard is empty (no grid rows) still calls it. */
int b7_score_finish_global(b7_ctx *ctx, double divisor, int64_t global_row_offset, double *best_val,
                           int64_t *best_idx1);

/* bots/abstract.lua:118 `pending, candidates = steal(pending, candidates, idx)` on a candidate set sharded across
 * ranks: idx1_global is the nominee's 1-based index in the union of the shards (what b7_eval_nominate /
 * b7_score_finish_global returned, or the random initial pick of bots/bayesopt.lua:90-91 drawn against the GLOBAL row
 * count from a seed all ranks share).  *global_row_offset is this rank's offset (rows before its shard), in and out.
 * Every rank calls it with the same idx1_global:
 *   - the rank whose shard holds the row deletes it on the device, stably (utils/tensor.lua:158-170: later rows move up);
 *   - ranks behind the owner get *global_row_offset - 1 back: the union has shrunk in front of them;
 *   - row_out (nullable, d) receives the nominee's coordinates on EVERY rank: from the record of the last exchange when
 *     idx1_global is its winner (no communication at all), otherwise by one more all-reduce in which the owner
 *     contributes the row (the random initial trials).
 * The removal is enqueued, not waited for: the next nomination runs behind it on the context's stream.
 * B7_ERR_INVALID when the index lies in no shard, or the offsets overlap. */
int b7_nominate_commit(b7_ctx *ctx, int64_t idx1_global, int64_t *global_row_offset, double *row_out);
/* Host-only, needs no context and no GPU: the bookkeeping rule b7_nominate_commit applies, for a shard that holds global
 * rows (offset, offset + M_local] (1-based): local_idx1 = the row to delete in this shard (0: another shard's),
 * new_offset = offset - 1 when the deleted row lies before this shard, else offset. */
int b7_shard_commit_rule(int64_t idx1_global, int64_t offset, int64_t M_local, int64_t *local_idx1, int64_t *new_offset);
/* What the last exchange told this rank (all outputs nullable): world size, candidate rows held by every rank
 * (world entries: their sum is the global row count, their prefix sums the offsets of contiguous shards), the winner's
 * global index, owning rank and grid row (d entries).  B7_ERR_STATE when the grid has changed since. */
int b7_exchange_info(b7_ctx *ctx, int *world, int64_t *rows_per_rank, int64_t *winner_idx1, int *winner_rank,
                     double *winner_row);

/* ---- bayesopt:eval + nominate as ONE call (bots/bayesopt.lua:56-99) --------------------------- *
 * score = (1/S) sum_s acq(model, hyp_s, X_obs, Y_obs, X_hid) over the resident data (b7_gp_set_data) and the
 * resident grid, then score:max(1) -- across ranks when the context has a communicator, exactly as
 * b7_score_finish_global.  Same results as the loop  { b7_gp_predict_hyp(hyp_s); b7_score_ei|cb } x S  +
 * b7_score_finish_global(S, offset), bit for bit, but all S fits, posteriors and score:adds are enqueued back to
 * back and the host waits once (without a communicator: on a word the arg-max kernel raises behind its record in mapped
 * host memory, so the call may return a moment before the stream is formally idle -- later calls queue behind it as always,
 * b7_sync waits for the stream): each fit's pivot report is checked afterwards, and a failed pivot (or a
 * hand-off time-out) redoes the nomination through the per-sample path with utils/math.lua:159-218's jitter
 * schedule.  With S > 1 and one response column the S fits run SIDE BY SIDE in one persistent launch (one critical
 * workgroup each): a fit's dependent chain leaves most of the chip idle, so ten fits cost little more than one;
 * and when K(X*,X) of all S samples fits the workspace, K*, posterior and score:add of all samples are one launch each.
 * jitter_out / info_out: nullable, S entries (as b7_gp_fit's).  The accumulator holds score / S afterwards
 * (b7_score_finish with divisor 1 downloads it); the context's own fit slot and mean / variance vectors hold none of
 * the S samples (fit again before b7_gp_predict / b7_score_*). */
#define B7_SCORE_EI 1 /* scores/expected_improvement.lua: needs fmin[ycols]; tradeoff = xi */
#define B7_SCORE_CB 2 /* scores/confidence_bound.lua: tradeoff = kappa, upper, sign as b7_score_cb */
/* Log-space EI, as b7_score_logei: no counterpart in scores/ of the reference (Ament et al., NeurIPS 2023).
 * log EI = log(sigma) + log(phi(z) + z Phi(z)); fmin and tradeoff as for B7_SCORE_EI, upper and sign ignored; the
 * marginal over the S samples is log((1/S) sum_s EI_s), best_val and the accumulator are log EI.  Accepted by every
 * eval + nominate entry point (b7_eval_nominate, b7_group_eval_nominate, b7_blr_eval_nominate, b7_blr_eval_nominate_marg).
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_SCORE_LOGEI 3
/* Max-value entropy search, as b7_score_mes: no counterpart in scores/ of the reference (Wang & Jegelka, ICML 2017).  fmin,
 * tradeoff, upper and sign are ignored.  Accepted by b7_eval_nominate on one rank and one response column: every sample's y*
 * search runs on the device ahead of its score, on every route of the call, the jitter redo included, and equals the loop
 * { b7_gp_predict_hyp; b7_score_mes } x S + b7_score_finish(S) bit for bit (b7_mes_last_ystar gives the S x K values of y*).
 * B7_ERR_UNSUPPORTED, each with a message naming the case: a communicator of more than one rank and b7_group_eval_nominate
 * (y* over a sharded grid), b7_blr_eval_nominate and b7_blr_eval_nominate_marg (b7_blr_predict + b7_score_mes works),
 * b7_eval_nominate_batch, more than one response column.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_SCORE_MES 4
/* Log probability of improvement, as b7_score_logpi: log Phi(z); fmin and tradeoff as for B7_SCORE_EI, upper and sign ignored; a
 * log accumulator, as B7_SCORE_LOGEI's.  Which entry point does what with it:
 *   accepted   b7_eval_nominate (every route, the jitter redo included; equals the loop { b7_gp_predict_hyp; b7_score_logpi } x S
 *              + b7_score_finish(S) bit for bit), b7_eval_nominate_feasible, b7_eval_nominate_batch, b7_group_eval_nominate,
 *              b7_blr_eval_nominate, b7_blr_eval_nominate_marg (all templates over the kind)
 *   refused    b7_eval_nominate_refine and b7_score_grad_compute: B7_ERR_UNSUPPORTED, "no gradient piece"
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_SCORE_LOGPI 5
typedef struct {
  int kind;
  double tradeoff;
  int upper;
  double sign;
  const double *fmin;
} b7_score_spec;
int b7_eval_nominate(b7_ctx *ctx, int S, const b7_hyp *hyps, const b7_score_spec *spec, int64_t global_row_offset,
                     double *best_val, int64_t *best_idx1, double *jitter_out, int *info_out);

/* ---- constrained nomination: the feasibility column and the weighted arg-max ------------------- *
 * No counterpart in the reference.  Gelbart et al. 2014 and Gardner et al. 2014 weight the acquisition by the probability that
 * every constraint c_k(x) <= t_k holds, EIC(x) = EI(x) prod_k Pr[c_k(x) <= t_k], each constraint with a GP and hyper samples of
 * its own; in log space (Ament et al. 2023) log EI + sum_k log PoF_k, which still ranks where the product underflows.
 * A context carries a device vector L[M] of LOG-WEIGHTS over its resident grid, allocated on demand, freed with the context and
 * FORGOTTEN whenever the grid changes (upload, generation, removal, commit, a one-sided map), as the accumulator is.
 *   b7_feas_reset     L := 0.0.  B7_ERR_STATE without a grid.
 *   b7_feas_add       L[j] += logw[j] from a host vector of M entries; M must be the grid's row count (B7_ERR_INVALID).  -inf
 *                     masks a row.  The general door for known constraints, masks and penalties.
 *   b7_feas_add_acc   L[j] += src's accumulator, device to device, no host copy.  src must be on the same device
 *                     (B7_ERR_UNSUPPORTED otherwise) and hold a valid, materialised LOG accumulator (B7_ERR_STATE otherwise) of
 *                     the same M (B7_ERR_INVALID otherwise): what b7_eval_nominate(src, ..., B7_SCORE_LOGPI) leaves, the marginal
 *                     already divided.  The two streams are ordered by events, both ways.  That both contexts hold the SAME GRID
 *                     ROWS is the caller's contract: only the row count can be checked.
 *   b7_feas_get       download L (M entries).
 *   b7_feas_nominate  score:max(1) of L alone (first NaN wins, else the first maximum); L is left untouched.  The nomination
 *                     while no feasible observation exists (Gelbart et al. 2014, section 3.2).
 * All but b7_feas_reset answer B7_ERR_STATE without a valid column; all answer B7_ERR_STATE on a member of a group.
 *   b7_eval_nominate_feasible   b7_eval_nominate with global_row_offset = 0 in every respect -- the routes, the single host wait,
 *                     the jitter redo behind a failed pivot, jitter_out / info_out -- except that between score:div and
 *                     score:max(1) each row's score v becomes w(v, L[j]):
 *                       a log accumulator (B7_SCORE_LOGEI, B7_SCORE_LOGPI)   w = v + L
 *                       B7_SCORE_EI                                          w = v * exp(L)
 *                     NaN if either operand is NaN; otherwise L = -inf gives -inf / 0.0 whatever v is (+inf - inf is never
 *                     formed).  The accumulator holds the WEIGHTED score afterwards; L is read, not modified.
 *                     B7_ERR_STATE: no valid column; a member of a group.  B7_ERR_UNSUPPORTED, the case named: B7_SCORE_CB (a
 *                     signed score has no product form), B7_SCORE_MES, more than one response column, a communicator of more
 *                     than one rank.
 * Not built in this version: sharded grids and groups, feasibility-weighted believer batches, refinement, Thompson paths,
 * decoupled evaluation of objective and constraints, the BLR head.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_feas_reset(b7_ctx *ctx);
int b7_feas_add(b7_ctx *ctx, const double *logw, int64_t M);
int b7_feas_add_acc(b7_ctx *ctx, b7_ctx *src);
int b7_feas_get(b7_ctx *ctx, double *out /*M*/);
int b7_feas_nominate(b7_ctx *ctx, double *best_val, int64_t *best_idx1);
int b7_eval_nominate_feasible(b7_ctx *ctx, int S, const b7_hyp *hyps, const b7_score_spec *spec, double *best_val,
                              int64_t *best_idx1, double *jitter_out, int *info_out);

/* A greedy BATCH of q nominees from one call: b7_eval_nominate's pick, then q - 1 more by KRIGING-BELIEVER variance downdates.
 * No counterpart in the reference, whose bots nominate one point per trial (bots/abstract.lua:118).  The believer pretends that
 * the row just picked, x_j, was observed at its own posterior mean under each hyper sample s (y_j := mu_s(x_j)).  Under that
 * lie the posterior mean of every candidate is unchanged, and the latent variance takes a rank-one downdate:
 *   c_s,j(x)   = k_s(x, x_j) - K*_s(x, X) w_s,j,        w_s,j = inv(K_s) k_s(X, x_j) = inv(L)' (inv(L) k_s(X, x_j))
 *   u_s,j(x)   = (c_s,j(x) - sum_{i<j} u_s,i(x) u_s,i(x_j)) / sqrt(t_s,j),     t_s,j = var_s,j-1(x_j) + noise_s
 *   var_s,j(x) = var_s,j-1(x) - u_s,j(x)^2
 * (noise_s includes the jitter that sample's factorisation needed, if any).  No refit, no factorisation, no variance product:
 * an extra pick is one pass that forms the rows of K* without storing them, two triangular mat-vecs per sample and a rescoring.
 *   pick 1     best_val[0], best_idx1[0], jitter_out and info_out are b7_eval_nominate's with global_row_offset = 0, bit for
 *              bit, for every score kind and covariance kernel, the jitter redo included;
 *   pick 2..q  the whole grid re-scored from the unchanged per-sample means, the downdated variances and the caller's spec (fmin
 *              stays the caller's: the lie never enters it), marginalised over the S samples as b7_eval_nominate does, then
 *              score:max(1) with the rows already picked in this call left out (a NaN there does not win).
 * q in 1..B7_BATCH_MAX and q <= the grid's rows, else B7_ERR_INVALID.  B7_ERR_UNSUPPORTED: b7_gp_opts.var_with_noise or
 * var_clamp set (the downdate works on the latent variance), more than one response column, a communicator of more than one
 * rank; a member of a group answers B7_ERR_STATE as b7_eval_nominate does (sharded batches are not built).  The grid is not
 * modified: the caller commits the q rows itself (b7_grid_remove_rows).  Deterministic: the same call twice gives the same
 * bits.  Afterwards the accumulator holds the LAST pick's score / S, and the context's own fit slot holds none of the samples.
 * Device memory: S (q + 1) M doubles beside b7_eval_nominate's, allocated on demand (B7_ERR_NOMEM) and freed with the context.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_BATCH_MAX 16
int b7_eval_nominate_batch(b7_ctx *ctx, int S, const b7_hyp *hyps, const b7_score_spec *spec, int q, double *best_val /*q*/,
                           int64_t *best_idx1 /*q*/, double *jitter_out, int *info_out);

/* The nominee REFINED OFF THE GRID by gradient ascent on the marginalised acquisition.  No counterpart in this reference's bots,
 * which nominate a grid row (bots/abstract.lua:118); Spearmint, which it descends from, hands its best grid rows to a local
 * optimiser.  b7_eval_nominate runs first: best_val, best_idx1, jitter_out and info_out are its outputs with global_row_offset
 * = 0, bit for bit, the jitter redo included.  Then `starts` starts -- the nominee, then the next winners of the same accumulator
 * under score:max(1)'s rule with the earlier ones left out; nothing is rescored -- climb for `iters` iterations on the posterior's
 * analytic gradient (both covariance kernels; EI with the score's own Phi and phi, LogEI through erfcx, CB), marginalised over
 * the S samples as the grid's score is.  Per start: a point x, its value v and gradient, a step eta in box widths (from eta0):
 *   iteration 0     value and gradient at the start itself (a start is not clipped);
 *   iteration t     g~_c = grad_c (hi_c - lo_c), m = max_c |g~_c|; m zero or not finite: the start stays (FLAT).  Otherwise four
 *                   rungs k = 0..3 at x'_c = min(max(x_c + (eta 4^-k g~_c / m)(hi_c - lo_c), lo_c), hi_c) are evaluated; the best
 *                   is the highest value, the lowest k on ties, a NaN never wins.  Strictly above v: the start moves there and
 *                   eta <- min(1, 4 eta 4^-k); otherwise it stays and eta <- eta / 256.  eta < 2^-40: CONVERGED, it moves no more.
 * A start's value never decreases.  The result is the start with the highest final value (lowest start order on ties, non-finite
 * values left out): x_out (d entries), val_out, start_idx1_out = the 1-based grid row it started from.  If no start moved, x_out is
 * the nominee's grid row bit for bit, val_out the refinement's own value there and start_idx1_out = best_idx1.  A start whose grid
 * score is NaN or whose iteration-0 value is not finite is NOT RUN and cannot win.  Deterministic: every sum has one order, so the
 * same call twice gives the same bits.  Afterwards the accumulator holds score / S as after b7_eval_nominate, the grid is not
 * modified, and the context's own fit slot holds none of the samples.
 * b7_refine_opts: starts in 1..B7_REFINE_MAX_STARTS and <= the grid's rows, iters in 0..B7_REFINE_MAX_ITERS, eta0 in (0, 1],
 * lo / hi d entries each (both NULL: the unit cube), finite, lo < hi; otherwise, or with a NULL argument other than jitter_out /
 * info_out: B7_ERR_INVALID.  B7_ERR_UNSUPPORTED, the case named: B7_SCORE_MES, more than one response column,
 * b7_gp_opts.var_with_noise / var_clamp, a communicator of more than one rank.  B7_ERR_STATE: a member of a group.
 * Device memory: a few S Npad 64 doubles, allocated on demand (B7_ERR_NOMEM) and freed with the context.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_REFINE_MAX_STARTS 16
#define B7_REFINE_MAX_ITERS 256
typedef struct {
  int starts;       /* [16] */
  int iters;        /* [16] */
  double eta0;      /* [1/16] first step, in box widths */
  const double *lo; /* [NULL] d entries; NULL (with hi): the unit cube */
  const double *hi;
} b7_refine_opts;
int b7_refine_default_opts(b7_refine_opts *out);
int b7_eval_nominate_refine(b7_ctx *ctx, int S, const b7_hyp *hyps, const b7_score_spec *spec, const b7_refine_opts *opts,
                            double *best_val, int64_t *best_idx1, double *x_out /*d*/, double *val_out, int64_t *start_idx1_out,
                            double *jitter_out, int *info_out);
/* Every start of the last b7_eval_nominate_refine: their number, final points P x d, final values, 1-based grid rows and status
 * bits (all nullable).  B7_ERR_STATE before a successful call. */
#define B7_REFINE_NOT_RUN 1   /* grid score NaN or iteration-0 value not finite */
#define B7_REFINE_FLAT 2      /* the gradient was zero or not finite at some iteration */
#define B7_REFINE_CONVERGED 4 /* eta fell below 2^-40 */
#define B7_REFINE_MOVED 8     /* moved at least once */
int b7_refine_last(b7_ctx *ctx, int *P, double *x /*P x d*/, double *val /*P*/, int64_t *start_idx1 /*P*/, int *status /*P*/);
/* The shapes of what the last b7_eval_nominate_refine left, for a caller that sizes b7_refine_last's and b7_refine_trace's buffers:
 * starts, d, iters, and whether it was traced (all nullable).  B7_ERR_STATE before a successful call. */
int b7_refine_shape(b7_ctx *ctx, int *P, int *d, int *iters, int *traced);
/* Trace of the calls that follow (on != 0): one record per start and iteration 0..iters, B7_REFINE_TRACE_WIDTH doubles each:
 * x after the iteration (d) | its value | its gradient (d) | eta before the step | the four rungs' values (NaN where no ladder was
 * run) | the rung taken (-1: stayed) | status bits | zeros.  b7_refine_trace: start `start`'s records of the last call (nullable)
 * and their number, iters + 1.  B7_ERR_STATE without a traced call. */
#define B7_REFINE_TRACE_WIDTH 200
int b7_refine_trace_enable(b7_ctx *ctx, int on);
int b7_refine_trace(b7_ctx *ctx, int start, double *records, int *n_records);
/* b7_gp_predict_at with gradients, on the context's CURRENT fit (one response column): mean[M1], var[M1] (the latent variance, amp -
 * |inv(L) k*|^2), dmean and dvar M1 x d (all nullable), by the refinement's kernels in chunks of 64 rows.  It disturbs nothing.
 * B7_ERR_STATE without a GP fit; B7_ERR_UNSUPPORTED as b7_eval_nominate_refine. */
int b7_gp_grad_at(b7_ctx *ctx, const double *X1, int64_t M1, double *mean, double *var, double *dmean /*M1 x d*/,
                  double *dvar /*M1 x d*/);
/* The refinement's score piece on host arrays (the b7_ei_compute of the refinement): S samples' mean / var (S x M1) and their
 * gradients (S x M1 x d) -> the marginal value[M1] (the grid's fold / div in sample order) and its gradient M1 x d (EI, CB: the mean
 * of the per-sample gradients; LogEI: their softmax-weighted sum).  spec->fmin: one entry.  d in 1..96. */
int b7_score_grad_compute(b7_ctx *ctx, const b7_score_spec *spec, int S, const double *mean, const double *var /*S x M1*/,
                          const double *dmean, const double *dvar /*S x M1 x d*/, int64_t M1, int d, double *value /*M1*/,
                          double *grad /*M1 x d*/);

/* THOMPSON SAMPLING: q nominees from q pathwise (decoupled) posterior samples.  No counterpart in the reference; Wilson,
 * Borovitskiy, Terenin, Mostowsky, Deisenroth (ICML 2020).  A sample path of the posterior is
 *   f_j(x) = m + phi(x)' w_j + K(x, X) v_j,        v_j = inv(K) (y - m - Phi(X) w_j - eps_j)
 * phi: F random Fourier features of the prior, phi(x)[f] = sqrt(2 amp / F) cos(Omega[f] . x + phase[f]); w_j ~ N(0, I);
 * eps_j ~ N(0, noise I) with the hyper sample's own noise (not the jitter its factorisation may add).  No M x M covariance is
 * formed: the update term is the posterior mean of a fit whose response columns are the pseudo-responses, the prior term one
 * kernel over the grid that never stores Phi.  Runs over the resident data (b7_gp_set_data, one response column) and grid.
 *   hyper samples  path j is drawn under hyper sample j mod S (Thompson sampling over hypers and function at once): min(S, q)
 *                  factorisations; hyper samples beyond the q-th are unused and report jitter 0, info 0.
 *   draws          from the library's counter generator (splitmix64 -> Box-Muller, as b7_gp_fantasize).  The basis (the normals
 *                  behind Omega, Matern's chi-square, the phases) is one per seed and shared by the call's paths; weight and eps are
 *                  path j's own.  Everything depends on (seed, j) alone: the paths of a q = 3 call are the first three of a q = 5
 *                  call.  ARD-SE: Omega[f][k] = z / sqrt(lenscale_sq[k]); ARD Matern-5/2: z sqrt(5 / u_f) / sqrt(lenscale_sq[k]),
 *                  u_f a sum of five squared normals (the spectral density is a multivariate t with 5 degrees of freedom).
 *   arg-mins       paths in order j = 0 .. q-1; path j takes its first minimum over the rows NOT TAKEN BY AN EARLIER PATH of this
 *                  call (two paths often share their minimiser); a NaN does not win; path_min[j] is the path's value at the row it
 *                  took, best_idx1[j] that row, 1-based.
 * jitter_out / info_out: nullable, S entries, as b7_eval_nominate's; a failed pivot goes through utils.math.chol's jitter schedule.
 * Deterministic: the same call twice gives the same bits.  The grid is not modified (commit with b7_grid_remove_rows); the
 * context's fit slot holds none of the samples afterwards; the score accumulator is untouched.
 * B7_ERR_INVALID: q outside 1..B7_BATCH_MAX or q > the grid's rows; F outside 16..B7_TS_MAX_FEATURES or not a multiple of 16;
 * S < 1; NULL arguments.  B7_ERR_UNSUPPORTED, the case named: more than one response column, a communicator of more than one
 * rank.  B7_ERR_STATE: a member of a group (as b7_eval_nominate_batch answers), no resident data or grid.
 * Device memory beside the posterior's own buffers: M q doubles for the paths (plus the draws, min(S, q) F d + (q + 1) F + q N, and
 * one hyper sample's operands), allocated on demand (B7_ERR_NOMEM) and freed with the context.
 * Not built: sharded grids and groups, more than one response column, a one-launch variant for N <= 128.  The Bayesian-linear head
 * has an entry of its own: b7_blr_ts_nominate below.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_TS_MAX_FEATURES 4096
int b7_ts_nominate(b7_ctx *ctx, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, double *path_min /*q*/,
                   int64_t *best_idx1 /*q*/, double *jitter_out /*S*/, int *info_out /*S*/);
/* Inspection (tests): the last successful b7_ts_nominate's paths over the grid, M x q row-major, and path `path`'s draws -- omega
 * (F x d, under its hyper sample's lengthscales), phase (F), weight (F, before the sqrt(2 amp / F) scale), eps (N); each nullable.
 * B7_ERR_STATE before a successful b7_ts_nominate. */
int b7_ts_last_paths(b7_ctx *ctx, double *paths_host /* M x q */);
int b7_ts_last_draws(b7_ctx *ctx, int path, double *omega /*F x d*/, double *phase /*F*/, double *weight /*F*/, double *eps /*N*/);
/* The feature kernel alone on host arrays (the b7_ei_compute of Thompson sampling): out = cos(X omega' + phase) W, M1 x q.
 * d in 1..96, q in 1..B7_BATCH_MAX, F a multiple of 16 in 16..B7_TS_MAX_FEATURES.  Its cosine reduces the argument in two
 * fused steps: accurate to ~1e-16 absolute for |argument| up to ~1e6, which unit-cube inputs over any admissible lengthscale stay
 * far inside. */
int b7_rff_compute(b7_ctx *ctx, const double *X /*M1 x d*/, int64_t M1, int d, const double *omega /*F x d*/,
                   const double *phase /*F*/, const double *W /*F x q*/, int F, int q, double *out /*M1 x q*/);

/* THOMPSON NOMINEES REFINED OFF THE GRID by descent on their own sample paths.  A pathwise sample is an explicit differentiable
 * function of x (Wilson et al. 2020 optimise it by gradient):
 *   f_j(x)     = m_s + sum_f W_j[f] cos(omega_s[f] . x + phase[f]) + sum_i v_j[i] k_s(x, X_i)              s = j mod S
 *   df_j/dx_c  = -sum_f W_j[f] sin(omega_s[f] . x + phase[f]) omega_s[f][c] - w_c (x_c sum_i v_j[i] g_i - sum_i v_j[i] g_i X_ic)
 * W = sqrt(2 amp / F) weight, w_c = 1 / lenscale_sq_c, g = k for ARD-SE and (5/3) amp (1 + s) exp(-s) for Matern-5/2.  No inv(L), no
 * variance and no hyper-sample loop enter: one evaluation costs O((F + N) d) per point.
 * b7_ts_nominate runs first: path_min, best_idx1, jitter_out, info_out and the kept paths and draws are its outputs, bit for bit.
 * Then every path j is refined on its own: its starts are its grid nominee (rank 0), then the `starts` - 1 rows of lowest f_j among
 * the rows that are none of the q grid nominees, ascending by (value, row), a NaN never chosen -- so the paths do not depend on each
 * other.  Each start runs b7_eval_nominate_refine's ladder on -f_j: the same four rungs, point formula, decision rule (strictly
 * better, the lowest rung on ties, a NaN never wins), eta update, 2^-40 floor and B7_REFINE_* status bits; iteration 0 evaluates the
 * start itself, unclipped.  A start's path value never increases.  Path j's result is the start of lowest final value (the lowest
 * rank on ties, non-finite values left out): x_out row j, val_out[j] = f_j there, start_idx1_out[j] = the 1-based grid row it
 * started from.  If no start of the path moved, the result is its grid nominee's row bit for bit, with the refinement's own value
 * there.  The whole refinement is one launch; every sum has one order, so a start's trajectory depends on its path's operands, its
 * start row and the options alone: the same call twice gives the same bits, and start rank r is the same for every `starts` > r.
 * The rows to commit (b7_grid_remove_rows) are the grid nominees best_idx1, distinct by construction.
 * b7_refine_opts as b7_eval_nominate_refine judges them, and starts <= M - q + 1; otherwise, or with a NULL argument other than
 * jitter_out / info_out: B7_ERR_INVALID.  B7_ERR_UNSUPPORTED: a communicator of more than one rank, more than one response column.
 * B7_ERR_STATE: a member of a group.  Everything else as b7_ts_nominate answers it.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_ts_nominate_refine(b7_ctx *ctx, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, const b7_refine_opts *opts,
                          double *path_min /*q*/, int64_t *best_idx1 /*q*/, double *x_out /*q x d*/, double *val_out /*q*/,
                          int64_t *start_idx1_out /*q*/, double *jitter_out /*S*/, int *info_out /*S*/);
/* Every start of path `path` in the last b7_ts_nominate_refine, in rank order: their number, final points P x d, final path values,
 * 1-based grid rows (0: no row was left for that rank) and status bits (all nullable).  B7_ERR_STATE before a successful call. */
int b7_ts_refine_last(b7_ctx *ctx, int path, int *P, double *x /*P x d*/, double *val /*P*/, int64_t *start_idx1 /*P*/,
                      int *status /*P*/);
/* Trace of the b7_ts_nominate_refine calls that follow (on != 0): one record per path, start and iteration 0..iters,
 * B7_REFINE_TRACE_WIDTH doubles each, in b7_refine_trace's layout: x after the iteration (d) | the path's value there | the path's
 * gradient there (d) | eta before the step | the four rungs' path values (NaN where no ladder was run) | the rung taken (-1:
 * stayed) | status bits | zeros.  The ladder ran on the negated values and gradients.  b7_ts_refine_trace: the records of start
 * `start` of path `path` (nullable) and their number, iters + 1.  B7_ERR_STATE without a traced call. */
int b7_ts_refine_trace_enable(b7_ctx *ctx, int on);
int b7_ts_refine_trace(b7_ctx *ctx, int path, int start, double *records, int *n_records);
/* The kept paths of the last b7_ts_nominate / b7_ts_paths / b7_ts_nominate_refine and their gradients at the rows of X1, by the
 * refinement's kernel: val M1 x q, grad M1 x q x d (both nullable).  It disturbs nothing.  B7_ERR_STATE: no kept paths, or the grid,
 * the data or the covariance kernel changed since they were drawn; a member of a group.  B7_ERR_UNSUPPORTED: the kept paths are
 * b7_blr_ts_nominate's (the DNGO head), a communicator of more than one rank, more than one response column. */
int b7_ts_path_grad_at(b7_ctx *ctx, const double *X1 /*M1 x d*/, int64_t M1, double *val /*M1 x q*/, double *grad /*M1 x q x d*/);

/* THOMPSON SAMPLING FOR THE BAYESIAN-LINEAR HEAD (DNGO): q nominees per call.  No counterpart in the reference.  The head's posterior
 * over its z weights is a finite Gaussian, N(m_s, inv(A_s)) with A_s = alpha_s I + beta_s Z'Z = L_s L_s', so a sample path is exact:
 *   f_j(x) = mean_s + phi(x)' w_j,      w_j = m_s + L_s^-T eps_j,      eps_j ~ N(0, I_z),      s = j mod S
 * -- no random features, no pseudo-response fit, no M x M covariance.  Paths are of the latent function: the 1 / beta observation
 * noise is not added, as b7_ts_nominate's paths carry none.
 *   heads     b7_blr_eval_nominate_marg's: one basis pass over the N observations and one over the resident grid; the S heads in one
 *             launch for z <= 64, otherwise head by head through b7_blr_fit_x.  All S are fitted (nll_out reports them), path j uses
 *             head j mod S.  A failed pivot redoes the heads through b7_blr_fit_x's jitter schedule, the paths are drawn from the
 *             jittered factors and *jitter_used < 0 (0 otherwise).
 *   draws     eps_j[k] is the library's counter normal on a stream of its own, a function of (seed, j, k) alone: the paths of a
 *             q = 3 call are the first three of a q = 5 call.
 *   arg-mins  b7_ts_nominate's rule: paths in order, each its first minimum over the rows no earlier path of the call took; a NaN
 *             does not win; path_min[j] is the path's value at the row it took, best_idx1[j] that row, 1-based.
 * Deterministic; an element of a path depends on its own grid row and its own weights alone (not on M, q or the other paths).  The grid
 * is not modified, the score accumulator is untouched, b7_ts_last_paths serves this call too.  z <= 256.
 * B7_ERR_INVALID: q outside 1..B7_BATCH_MAX or q > the grid's rows; S < 1; NULL arguments; a precision <= 0.  B7_ERR_UNSUPPORTED, the
 * case named: a communicator of more than one rank.  B7_ERR_STATE: a member of a group, no resident grid.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_blr_ts_nominate(b7_ctx *ctx, const b7_mlp *net, const double *X0, const double *Y0, int N, int S,
                       const double *alpha_prec, const double *beta, const double *mean /*S each*/, int q, uint64_t seed,
                       double *path_min /*q*/, int64_t *best_idx1 /*q*/, double *nll_out /*S, nullable*/,
                       double *jitter_used /*nullable*/);
/* Inspection (tests): path `path`'s draw eps and weight vector w (z each, either nullable) of the last successful
 * b7_blr_ts_nominate; B7_ERR_STATE before one (and after a b7_ts_nominate, whose draws b7_ts_last_draws reads). */
int b7_blr_ts_last_draws(b7_ctx *ctx, int path, double *eps /*z*/, double *weight /*z*/);
/* The paths kernel alone on host arrays (the b7_rff_compute of this feature): out = mean0' + Z W, M1 x q, on the fp64 matrix
 * cores.  z in 1..256, q in 1..B7_BATCH_MAX.  The order of summation over z is fixed and mean0[j] is added once, last: an element's
 * bits depend on its own row of Z and column of W alone. */
int b7_blr_paths_compute(b7_ctx *ctx, const double *Z /*M1 x z*/, int64_t M1, int z, const double *W /*z x q*/,
                         const double *mean0 /*q*/, int q, double *out /*M1 x q*/);

/* THE KNOWLEDGE GRADIENT: a one-step look-ahead nomination.  No counterpart in the reference; Frazier, Powell & Dayanik (2009),
 * Scott, Frazier & Powell (2011).  The expected decrease of the MINIMUM OF THE POSTERIOR MEAN after one more, possibly noisy,
 * evaluation at x -- it needs no incumbent f_min and values a point for what it teaches about other points.  Under hyper sample
 * s, with a discretisation set A of n grid rows a_1 .. a_n:
 *   KG_s(x) = min_i alpha_i - E_Z[min_i (alpha_i + b_i Z)] >= 0,       Z ~ N(0, 1),
 *   alpha_i = mu_s(a_i),  b_i = c_i(x) / sqrt(t(x)),  c_i(x) = k_s(x, a_i) - K*_s(x, X) inv(K_s) k_s(X, a_i)  (the posterior covariance),
 *   t(x) = var_s(x) + noise_s (+ the jitter its factorisation may have needed);
 *   line 0 is x's own: alpha_0 = mu_s(x), b_0 = var_s(x) / sqrt(t(x)); it is left out when x is itself a row of A (by row index).
 * The expectation is exact (the lower envelope of the n + 1 lines, in Frazier's positive-term form: a small KG keeps its relative
 * accuracy).  var NaN or < 0, or mu NaN: NaN; t(x) = 0: 0.  The nominee is the arg-max of the linear mean over the S samples in
 * sample order, by b7_eval_nominate's rule (the first NaN, else the maximum, ties to the lowest index).
 *   rows1   n distinct 1-based grid rows, e.g. the minimisers b7_ts_nominate returned; NULL: the library takes the n rows of lowest
 *           (1/S) sum_s mu_s (ties to the lowest index), chosen on the device.
 * Fits, routes, the single host wait and the jitter redo are b7_eval_nominate's; jitter_out / info_out as there (nullable, S).
 * Runs over the resident data (one response column) and grid, both covariance kernels.  Deterministic: the same call twice gives the
 * same bits, and a row's value does not depend on how many rows the grid has.  The grid is not modified; the context's fit slot
 * holds none of the samples afterwards; the score accumulator holds the marginal knowledge gradient (b7_score_finish reads it).
 * B7_ERR_INVALID: n outside 1..B7_KG_MAX_POINTS or above the grid's rows; a duplicate or out-of-range row; S < 1; NULL hyps,
 * best_val or best_idx1.  B7_ERR_UNSUPPORTED, the case named: more than one response column, var_with_noise / var_clamp, a
 * communicator of more than one rank.  B7_ERR_STATE: a member of a group, no resident data or grid.
 * Device memory beside the posterior's own buffers: 3 S M doubles and 32 S Npad for the columns, allocated on demand.
 * Not built: sharded grids and groups, batches, refinement of the nominee, the Bayesian-linear head, constraints, a continuous
 * discretisation.  Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_KG_MAX_POINTS 16
int b7_kg_nominate(b7_ctx *ctx, int S, const b7_hyp *hyps, int n, const int64_t *rows1 /* n, 1-based grid rows; nullable */,
                   double *best_val, int64_t *best_idx1, double *jitter_out /*S*/, int *info_out /*S*/);
/* Inspection (tests): what the last successful b7_kg_nominate used and made -- the rows of A (1-based), alpha (S x n), the slopes
 * (S x M x (n + 1), column 0 the own line: NaN where the row is in A and has none), the per-sample values (S x M) and the own
 * lines' intercepts mu_s(x) (S x M); each nullable.  The slopes are kept only by calls made while b7_kg_trace_enable is on (the
 * nomination stores nothing extra otherwise).  B7_ERR_STATE before a successful call, or for slopes the call did not keep. */
int b7_kg_trace_enable(b7_ctx *ctx, int on);
int b7_kg_last(b7_ctx *ctx, int64_t *rows1 /*n*/, double *alpha /*S x n*/, double *slopes /*S x M x (n+1), column 0 = own line*/,
               double *values /*S x M*/, double *own_alpha /*S x M*/);
/* The envelope expectation alone on host arrays (the b7_ei_compute of the knowledge gradient), by the nomination's own code:
 * out[j] = min_i alpha[j][i] - E[min_i (alpha[j][i] + b[j][i] Z)] over L lines, L in 1..B7_KG_MAX_POINTS + 1.  Column 0 is the own
 * line; a NaN slope there means the row has none (b7_kg_last's convention).  Finite input gives a finite result >= 0. */
int b7_kg_compute(b7_ctx *ctx, int64_t M1, int L, const double *alpha /*M1 x L*/, const double *b /*M1 x L*/, double *out);

/* TWO OBJECTIVES: the exact expected hypervolume improvement (EHVI).  No counterpart in the reference; the two-objective case of
 * Emmerich, Yang & Deutz (2016).  Both objectives are MINIMISED.  ref = (r1, r2) is the reference point; a CANONICAL FRONT is P
 * points (a_k, b_k), k = 1..P, finite, strictly inside the reference box (a_k < r1, b_k < r2), a strictly ascending and b strictly
 * descending (so mutually non-dominated), stored P x 2 row-major.  With a_0 = -inf, a_P+1 = r1, b_0 = r2 and independent posteriors
 * y1 ~ N(mu1, var1), y2 ~ N(mu2, var2):
 *   EHVI = sum_{k=0..P} [Psi(a_k+1; mu1, sigma1) - Psi(a_k; mu1, sigma1)] Psi(b_k; mu2, sigma2),
 *   Psi(a; mu, sigma) = E[(a - y)+] = (a - mu) Phi(z) + sigma phi(z),  z = (a - mu) / sigma,  Psi(-inf) = 0.
 * The marginal over S1 hyper samples of objective 1 and S2 of objective 2 (independent chains) factorises strip by strip:
 *   score = sum_{k=0..P} A_k B_k,  A_k = (1/S1) sum_s max(Psi(a_k+1; s) - Psi(a_k; s), 0),  B_k = (1/S2) sum_t Psi(b_k; t),
 * which is (1/(S1 S2)) sum_s sum_t EHVI_st exactly, at O((S1 + S2) P) per candidate.  Fixed order: k ascending, s / t ascending within
 * it, each sum divided once by its sample count, one rounded operation per operator, every Psi(a_k; s) evaluated once.
 * Psi in the positive-term form: with d = a - mu, t = |d| / sigma and f = max(phi(t) - t erfc(t / sqrt2) / 2, 0) (ocml's erfc and exp),
 * Psi = sigma f for d <= 0 and d + sigma f for d > 0; sigma == 0: max(d, 0) exactly; t > 37.5 (phi(t) below the smallest normal
 * double): f = 0.
 * Row classes: any mu or var NaN, or any var < 0, in either objective: NaN (the first NaN wins the arg-max, as everywhere);
 * otherwise the score is finite and >= 0 (as long as no a - mu overflows), P = 0 included: Psi1(r1) Psi2(r2).
 * Limits: P <= B7_EHVI_PMAX; S1, S2 in 1..B7_EHVI_SMAX.  The first B7_EHVI_SREG samples of each objective are held in registers
 * across the strips, the rest in LDS.
 * Not built, each refused by name where it can be asked for: more than two objectives by these entry points (three only through
 * b7_ehvi3_* below, four and more nowhere), correlated objectives / multi-task GPs, a log-space EHVI by these entry points
 * (b7_logehvi_* below), batches, refinement, constraints combined with objectives, sharded grids and groups, the Bayesian-linear head,
 * ParEGO-style scalarisation.  Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_EHVI_PMAX 256
#define B7_EHVI_SMAX 32
#define B7_EHVI_SREG 10
/* The posterior half of b7_eval_nominate, KEPT: fits and posteriors of all S hyper samples over the resident data (one response
 * column) and grid by b7_eval_nominate's routes (the one-launch route for N <= 128, side-by-side fits with batched K*, per-sample
 * posteriors when the workspace does not hold K*, the jitter redo), mean and variance of every sample left as [S][M] in a buffer
 * the context owns.  No arg-max is taken; the routes that score inline score a confidence bound whose values are dropped, and the
 * context holds NO accumulator afterwards.  var_with_noise and var_clamp of b7_gp_opts apply as in b7_gp_predict_hyp; jitter_out /
 * info_out (nullable, S entries) as b7_eval_nominate's.  The kept posterior is forgotten when the grid or the data changes.
 * B7_ERR_UNSUPPORTED, the case named: more than one response column, a communicator of more than one rank.  B7_ERR_STATE: a member
 * of a group, no resident data or grid.  Device memory: 2 S M doubles, allocated on demand.  No counterpart in the reference. */
int b7_eval_posterior(b7_ctx *ctx, int S, const b7_hyp *hyps, double *jitter_out /*S*/, int *info_out /*S*/);
/* Sample s (0-based) of the kept posterior: mean and var, M entries each (either nullable).  B7_ERR_STATE without a kept posterior,
 * B7_ERR_INVALID for s outside it.  No counterpart in the reference. */
int b7_posterior_get(b7_ctx *ctx, int s, double *mean /*M*/, double *var /*M*/);
/* Host-only (no context, no GPU): the canonical front of n rows of two responses, Y n x 2.  Rows with a non-finite entry and rows
 * not strictly inside the reference box are dropped, dominated rows are dropped, of equal rows the lowest stays; the rest sorted.
 * front_out: room for min(n, B7_EHVI_PMAX) points (P x 2); rows1_out (nullable, same count): each point's 1-based source row.
 * B7_ERR_INVALID: a NULL argument, n < 0, a non-finite ref, or a front of more than B7_EHVI_PMAX points (nothing is written but
 * *P_out, the count).  No counterpart in the reference. */
int b7_pareto_front2(const double *Y /*n x 2*/, int64_t n, const double *ref /*2*/, double *front_out, int64_t *rows1_out, int *P_out);
/* Host-only: the area dominated by a canonical front inside the reference box, sum_k (a_k+1 - a_k)(r2 - b_k), k ascending; P = 0: 0.
 * B7_ERR_INVALID for a front that is not canonical (any P >= 0 is taken).  No counterpart in the reference. */
int b7_hypervolume2(const double *front /*P x 2*/, int P, const double *ref /*2*/, double *hv_out);
/* The score alone on host arrays (the b7_ei_compute of EHVI), by the nomination's own kernel: mu1 / var1 S1 x M, mu2 / var2 S2 x M,
 * out M.  B7_ERR_INVALID: a front that is not canonical or longer than B7_EHVI_PMAX, a non-finite ref, S1 or S2 outside
 * 1..B7_EHVI_SMAX, NULL arguments.  No counterpart in the reference. */
int b7_ehvi_compute(b7_ctx *ctx, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                    const double *front /*P x 2*/, int P, const double *ref /*2*/, int64_t M, double *out /*M*/);
/* The nomination: ctx holds objective 1's kept posterior (b7_eval_posterior), other objective 2's; other == ctx is allowed (one
 * posterior for both).  Both on the same device with the same number of grid rows -- that the rows are the same is the caller's
 * contract, as for b7_feas_add_acc; the two streams are ordered by events both ways.  The marginal score is written to ctx's
 * accumulator (a linear one, already divided: b7_score_finish(1) downloads it), the nominee is its score:max(1) by
 * b7_eval_nominate's rule (the first NaN, else the maximum, ties to the lowest index).  Neither grid is modified.  Deterministic:
 * the same call twice gives the same bits, and a row's value does not depend on how many rows the grid has.
 * B7_ERR_INVALID: a front that is not canonical or longer than B7_EHVI_PMAX, a non-finite ref, a kept posterior of more than
 * B7_EHVI_SMAX samples, different row counts, NULL arguments.  B7_ERR_STATE: no kept posterior on either side, a member of a
 * group.  B7_ERR_UNSUPPORTED: contexts on different devices.  No counterpart in the reference. */
int b7_ehvi_nominate(b7_ctx *ctx, b7_ctx *other, const double *front /*P x 2*/, int P, const double *ref /*2*/, double *best_val,
                     int64_t *best_idx1);

/* THREE OBJECTIVES: the exact EHVI over a box decomposition.  No counterpart in the reference.  All objectives are MINIMISED;
 * ref = (r1, r2, r3).  A CANONICAL FRONT here is P points, finite, strictly inside the reference box, mutually non-dominated, sorted
 * strictly ascending by (third, first, second) objective, stored P x 3 row-major.  Two non-dominated points may share a coordinate in
 * ONE objective.  The region that no front point dominates, inside (-inf, r], is cut into disjoint boxes [l_b, u_b], every l_b3 = -inf
 * (b7_nondominated_boxes3).  With independent posteriors and Psi as above,
 *   EHVI = sum_b prod_m [Psi_m(u_bm) - Psi_m(l_bm)],   Psi(-inf) = 0,
 * and the marginal over S1 x S2 x S3 hyper samples (independent chains) factorises box by box and objective by objective:
 *   T_m(c) = (1/S_m) sum_s Psi(c; mu_ms, sigma_ms),  T_m(-inf) = 0,
 *   score  = sum_b max(T_1(u_b1) - T_1(l_b1), 0) max(T_2(u_b2) - T_2(l_b2), 0) T_3(u_b3),
 * exact, no random numbers, every term non-negative; the dominated volume is never subtracted from the box's.  Fixed order: s ascending
 * within a T, each T divided once by its sample count; the boxes in the decomposition's order, ((d1 d2) T_3) added to the running sum;
 * one rounded operation per operator, Psi's arithmetic as above.  T_m is evaluated once per distinct cut (the front's coordinates and
 * r_m, at most P + 1 per objective) into a table of sum_m (cuts_m + 1) doubles per candidate, which a second kernel walks box by box;
 * the candidates are cut into chunks so that the table stays within min(b7_set_workspace's bytes, 256 MiB), and a row's bits do not depend
 * on the chunking.
 * Row classes: any mu or var NaN, or any var < 0, in any objective: NaN; otherwise the score is finite and >= 0, P = 0 included:
 * T_1(r1) T_2(r2) T_3(r3).  Limits: P <= B7_EHVI3_PMAX; S1, S2, S3 in 1..B7_EHVI_SMAX.
 * Not built, each refused by name where it can be asked for: four or more objectives, correlated objectives / multi-task GPs, a
 * log-space EHVI by these entry points (b7_logehvi3_* below), batches, refinement, constraints combined with objectives, sharded grids and groups, the Bayesian-linear head,
 * trust regions.  Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_EHVI3_PMAX 256
/* Host-only (no context, no GPU): the canonical front of n rows of three responses, Y n x 3.  Rows with a non-finite entry and rows
 * not strictly inside the reference box are dropped, dominated rows are dropped, of equal rows the lowest stays; the rest sorted by
 * (third, first, second) objective.  front_out: room for min(n, B7_EHVI3_PMAX) points (P x 3); rows1_out (nullable, same count): each
 * point's 1-based source row.  B7_ERR_INVALID: a NULL argument, n < 0, a non-finite ref, or a front of more than B7_EHVI3_PMAX points
 * (nothing is written but *P_out, the count).  No counterpart in the reference. */
int b7_pareto_front3(const double *Y /*n x 3*/, int64_t n, const double *ref /*3*/, double *front_out, int64_t *rows1_out, int *P_out);
/* Host-only: the non-dominated region of a canonical front inside (-inf, ref] as B disjoint boxes, each l1, u1, l2, u2, u3 (the lower
 * edge in the third objective is -inf throughout; -inf is a legal l1 / l2 too).  Deterministic: the front is swept in its order over
 * the two-dimensional staircase of the projections seen so far; a point's projection newly dominates a part of [a, r1] x [b, .], cut
 * into vertical rectangles at the staircase points it passes, each extended to (-inf, c]; the |F| + 1 strips of the final staircase
 * extended to (-inf, r3] follow.  B = 2P + 1 in general position, fewer with tied coordinates; boxes_out: room for 3P + 1 boxes is
 * always enough.  B7_ERR_INVALID: a NULL argument, P outside 0..B7_EHVI3_PMAX, a front that is not canonical.
 * No counterpart in the reference. */
int b7_nondominated_boxes3(const double *front /*P x 3*/, int P, const double *ref /*3*/, double *boxes_out /*B x 5*/, int *B_out);
/* Host-only: the volume dominated by a canonical front inside the reference box, as the sum over the slabs between consecutive
 * distinct third coordinates (the last up to r3) of the two-dimensional area dominated by the points at or below the slab, times the
 * slab's height; all terms positive; P = 0: 0.  B7_ERR_INVALID for a front that is not canonical.  No counterpart in the reference. */
int b7_hypervolume3(const double *front /*P x 3*/, int P, const double *ref /*3*/, double *hv_out);
/* The score alone on host arrays, by the nomination's own kernels: mu[m] / var[m] S[m] x M of objective m = 0, 1, 2, out M.
 * B7_ERR_INVALID: a front that is not canonical or longer than B7_EHVI3_PMAX, a non-finite ref, an S[m] outside 1..B7_EHVI_SMAX, NULL
 * arguments.  No counterpart in the reference. */
int b7_ehvi3_compute(b7_ctx *ctx, const double *const *mu /*3*/, const double *const *var /*3*/, const int *S /*3*/,
                     const double *front /*P x 3*/, int P, const double *ref /*3*/, int64_t M, double *out /*M*/);
/* The nomination: ctx holds objective 1's kept posterior (b7_eval_posterior), other2 objective 2's, other3 objective 3's; the contexts
 * may coincide.  All on the same device with the same number of grid rows -- that the rows are the same is the caller's contract; the
 * streams are ordered by events both ways, as b7_ehvi_nominate orders them.  The marginal score is written to ctx's accumulator (a
 * linear one, already divided: b7_score_finish(1) downloads it), the nominee is its score:max(1) by b7_eval_nominate's rule.  No grid
 * is modified, the other contexts' posteriors are only read.  Deterministic: the same call twice gives the same bits, and a row's value
 * does not depend on how many rows the grid has.
 * B7_ERR_INVALID: a front that is not canonical or longer than B7_EHVI3_PMAX, a non-finite ref, a kept posterior of more than
 * B7_EHVI_SMAX samples, different row counts, NULL arguments.  B7_ERR_STATE: no kept posterior on one of the three, a member of a
 * group.  B7_ERR_UNSUPPORTED: contexts on different devices.  No counterpart in the reference. */
int b7_ehvi3_nominate(b7_ctx *ctx, b7_ctx *other2, b7_ctx *other3, const double *front /*P x 3*/, int P, const double *ref /*3*/,
                      double *best_val, int64_t *best_idx1);

/* LOG-SPACE EHVI for two and three objectives: the logarithm of the two marginal scores above, evaluated so that it never underflows
 * (the multi-objective twin of b7_score_logei; Ament et al., NeurIPS 2023).  No counterpart in the reference.  The linear scores are
 * exactly 0 wherever every strip or box has a Psi with z < -37.5 -- a reference point that no observation has reached, late trials with
 * small posterior variance, most rows of a large grid -- and score:max(1) then nominates row 1; these still rank such rows.
 *   logPsi(a; mu, var) = log EI(mu, var, fmin = a, xi = 0) as b7_score_logei evaluates it (its three branches and edge cases); a = -inf: -inf
 *   ldiff(u, l) = log(e^u - e^l):  l == -inf: u exactly;  !(l < u): -inf (the linear code's clamp at 0);  otherwise, d = l - u:
 *                 u + log(-expm1(d)) if d > -ln 2, else u + log1p(-exp(d))
 *   LSE: a log-sum-exp in a fixed order in the running-max form -- (m, acc) = (-inf, 0); a term t == -inf is skipped; otherwise
 *        e = exp(-|t - m|) and (m, acc) = (t, acc e + 1) if t > m, else (m, acc + e); the value is -inf if m == -inf, else m + log(acc).
 *        An empty sum is -inf, a single term comes back exactly.
 *   two objectives:    log score = LSE_k[(LSE_s ldiff(logPsi(a_k+1; s), logPsi(a_k; s)) - log S1) + (LSE_t logPsi(b_k; t) - log S2)],
 *                      k ascending, s / t ascending within it, every logPsi(a_k; s) evaluated once
 *   three objectives:  LT_m(c) = LSE_s logPsi(c; s) - log S_m per distinct cut, LT_m(-inf) = -inf, and over b7_nondominated_boxes3's
 *                      boxes in their order  log score = LSE_b[(ldiff(LT1(u1), LT1(l1)) + ldiff(LT2(u2), LT2(l2))) + LT3(u3)]
 * log S_m is the logarithm of the sample count (S_m = 1: exactly 0); one rounded operation per operator; erfc, erfcx, exp, expm1, log and
 * log1p are ocml's.  Row classes: NaN exactly where the linear score is NaN (any mu or var NaN, or any var < 0, in any objective);
 * otherwise, for finite input, never NaN and never +inf; -inf is a legal value (every var == 0 and the point dominated).
 * Signatures, limits (B7_EHVI_PMAX / B7_EHVI3_PMAX, B7_EHVI_SMAX, B7_EHVI_SREG), the canonical-front checks, the refusals and the
 * ordering of the streams are those of the linear twins; the three-objective table is chunked the same way and a row's bits do not
 * depend on the chunking.  Not built: as listed for the linear twins, the log form aside.  Added without a change of B7_ABI_VERSION:
 * the change is additive. */
/* b7_ehvi_compute's twin: the log score alone on host arrays, by the nomination's own kernel.  No counterpart in the reference. */
int b7_logehvi_compute(b7_ctx *ctx, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                       const double *front /*P x 2*/, int P, const double *ref /*2*/, int64_t M, double *out /*M*/);
/* b7_ehvi_nominate's twin.  The marginal log score is written to ctx's accumulator as a LOG accumulator, already divided:
 * b7_score_finish(1) downloads it, and b7_feas_add_acc(any, ctx) takes it, so that constrained multi-objective nomination is
 * b7_feas_reset, b7_feas_add / b7_feas_add_acc of the constraints' log-weights, b7_feas_add_acc(ctx, ctx), b7_feas_nominate.  The
 * nominee is score:max(1) by b7_eval_nominate's rule (the first NaN, else the maximum, ties to the lowest index).  Errors as
 * b7_ehvi_nominate's.  No counterpart in the reference. */
int b7_logehvi_nominate(b7_ctx *ctx, b7_ctx *other, const double *front /*P x 2*/, int P, const double *ref /*2*/, double *best_val,
                        int64_t *best_idx1);
/* b7_ehvi3_compute's twin: the log score alone on host arrays, by the nomination's own kernels.  No counterpart in the reference. */
int b7_logehvi3_compute(b7_ctx *ctx, const double *const *mu /*3*/, const double *const *var /*3*/, const int *S /*3*/,
                        const double *front /*P x 3*/, int P, const double *ref /*3*/, int64_t M, double *out /*M*/);
/* b7_ehvi3_nominate's twin; the accumulator is a LOG one, as b7_logehvi_nominate leaves it.  Errors as b7_ehvi3_nominate's.
 * No counterpart in the reference. */
int b7_logehvi3_nominate(b7_ctx *ctx, b7_ctx *other2, b7_ctx *other3, const double *front /*P x 3*/, int P, const double *ref /*3*/,
                         double *best_val, int64_t *best_idx1);

/* MULTI-OBJECTIVE THOMPSON SAMPLING: q nominees per call for two or three objectives (TSEMO: Bradford, Schweidtmann & Lapkin 2018).
 * No counterpart in the reference.  Under a sample path the world is deterministic, so the best addition to a batch is the row whose
 * sampled values improve the hypervolume most.  All objectives are minimised; fronts are canonical (b7_pareto_front2 / 3).
 *
 * b7_ts_paths: the path half of b7_ts_nominate, as b7_eval_posterior is the posterior half of b7_eval_nominate: the same validation,
 * draws, fits and paths for the same arguments, bit for bit, without the arg-mins.  b7_ts_last_paths and b7_ts_last_draws serve it.
 * The context remembers which grid and data the kept paths belong to: after a change of either (or of the covariance kernel) the
 * nominations below answer B7_ERR_STATE, the way a kept posterior is forgotten; b7_ts_last_paths keeps serving the paths as they were
 * made.  Errors as b7_ts_nominate's (its two outputs aside). */
int b7_ts_paths(b7_ctx *ctx, int S, const b7_hyp *hyps, int q, int F, uint64_t seed, double *jitter_out /*S*/, int *info_out /*S*/);
/* The nominations.  ctx holds objective 1's kept paths (b7_ts_paths, or a b7_ts_nominate), other / other2, other3 those of the
 * later objectives, each drawn with its own seed and hyper samples over the same grid rows with the same q; contexts may coincide.
 * The score of a row under path j against a front is the hypervolume improvement of its sampled values y:
 *   two objectives    hvi(y) = sum_{k = 0 .. P} max(a_k+1 - max(a_k, y1), 0) * max(b_k - y2, 0),   a_0 = -inf, a_P+1 = r1, b_0 = r2
 *   three objectives  hvi(y) = sum_b (max(u1 - max(l1, y1), 0) * max(u2 - max(l2, y2), 0)) * max(u3 - y3, 0)
 * over the strips in ascending order, over the boxes of b7_nondominated_boxes3 in its order, a running sum from 0, one rounded
 * operation per operator: the deterministic limit of b7_ehvi_compute / b7_ehvi3_compute.  A row with a value that is not finite
 * scores NaN, and a NaN never wins.  A value depends on its own row and the front alone.
 * The rule, for path j = 0 .. q - 1 in order:
 *   1. the working front of path j is the canonical front (b7_pareto_front2 / 3's logic, the caller's points first) of the caller's
 *      front and the earlier picks' values under path j, (f_1j(r_i), f_2j(r_i)[, f_3j(r_i)]) for i < j;
 *   2. the pick r_j is the row with the largest hvi of its path-j values against that front over the rows no earlier path took, ties
 *      to the lowest row; hvi_out[j] is that value, best_idx1[j] the row (1-based), y_out row j (nullable) its path-j values;
 *   3. where no row has a positive hvi (the path's whole image is dominated or outside the box) the pick is the first minimum of
 *      objective 1 + (j mod m)'s path j over the rows not taken (b7_ts_nominate's arg-min), and hvi_out[j] = 0.
 * Deterministic; since paths depend on (seed, j) alone the picks of a q = 3 call are the first three of a q = 5 call.  No grid is
 * modified, the score accumulator and the kept posterior are untouched.  The streams of the contexts are ordered by events both
 * ways, as b7_ehvi_nominate orders them.
 * B7_ERR_STATE, the case named: an objective has no kept paths, or its paths are stale; a context is a member of a group.
 * B7_ERR_INVALID: q or M differ between the contexts; P + q - 1 exceeds B7_EHVI_PMAX / B7_EHVI3_PMAX (the working front can grow by
 * a point per pick); the front is not canonical or ref not finite (as b7_ehvi_nominate answers); a NULL argument.
 * B7_ERR_UNSUPPORTED: contexts on different devices; kept paths left by b7_blr_ts_nominate (the DNGO head is not built here).
 * Device memory: small staging, plus m q M doubles for the [q][M] copies of the paths that the picks read (q > 1).
 * Not built: sharded grids and groups, the DNGO head, four or more objectives, correlated objectives.
 * Added without a change of B7_ABI_VERSION: the change is additive. */
int b7_ts_hvi_nominate(b7_ctx *ctx, b7_ctx *other, const double *front /*P x 2*/, int P, const double *ref /*2*/,
                       double *hvi_out /*q*/, int64_t *best_idx1 /*q*/, double *y_out /*q x 2, nullable*/);
int b7_ts_hvi3_nominate(b7_ctx *ctx, b7_ctx *other2, b7_ctx *other3, const double *front /*P x 3*/, int P, const double *ref /*3*/,
                        double *hvi_out /*q*/, int64_t *best_idx1 /*q*/, double *y_out /*q x 3, nullable*/);
/* The score alone on host arrays (the b7_ei_compute of this feature), by the nomination's own kernels: out[i] = hvi(Y[i]) for m = 2
 * or 3 objectives; NaN for a row with an entry that is not finite.  The kept paths are untouched. */
int b7_hvi_compute(b7_ctx *ctx, const double *Y /*M1 x m*/, int64_t M1, int m, const double *front /*P x m*/, int P,
                   const double *ref /*m*/, double *out /*M1*/);

/* CONSTRAINED THOMPSON SAMPLING: q feasible-first nominees per call under C black-box constraints c_k(x) <= t_k -- the selection rule
 * of SCBO (Eriksson & Poloczek, AISTATS 2021).  No counterpart in the reference.  Under a joint sample path (f_j, c_1j .. c_Cj) of the
 * objective and every constraint the world is deterministic: path j takes the row of lowest f_j among the rows where every
 * c_kj <= t_k, and where the path sees no such row the row of smallest total violation.  No feasibility weight, no incumbent, no
 * special case while nothing feasible has been observed; the objective is minimised.
 *
 * ctx holds the objective's kept paths (b7_ts_paths, or a b7_ts_nominate), cons[k] those of constraint k + 1, each drawn with its
 * own seed and hyper samples over the same grid rows with the same q; contexts may coincide.  The key of (row i, path j), thresholds
 * finite, one rounded operation per operator:
 *   viol = ((0 + max(c_1j[i] - t_1, 0)) + max(c_2j[i] - t_2, 0)) + ..       k ascending, a running sum from 0
 *   class -1: any of the 1 + C values is NaN, the row never wins;  class 0 (feasible): viol == 0, key f_j[i];  class 1: key viol.
 * Class 0 comes before class 1, within a class the smaller key wins, equal keys go to the lowest row.  viol == 0 says "every
 * c_k <= t_k" exactly (a difference of two distinct doubles is never 0), and +-inf need no special case: the terms are non-negative.
 * A key depends on its own row and the thresholds alone.  C = 0 is b7_ts_nominate's rule.
 * The rule, for path j = 0 .. q - 1 in order: the pick r_j is the best row of path j over the rows no earlier path took;
 * key_out[j] is its key, class_out[j] its class, best_idx1[j] the row (1-based), y_out row j (nullable) its path-j values
 * f_j, c_1j .. c_Cj.  A path with no scoring row reports index 0, class -1, a NaN key and NaN values, and excludes nothing.
 * Two arms compute the same bits.  The library's default picks path by path: q passes chained on the device, pass j over the rows
 * no earlier pass took, one wait; *reruns_out (nullable) is then 0.  The other arm (the diagnostic build's B7_TS_FEAS_ONEPASS = 1)
 * scores all q paths in one pass that reads each of the 1 + C path buffers once and resolves the exclusions after one wait: where the
 * best row of path j over ALL rows is not taken it is the pick, otherwise path j alone is run again over the rows not taken, and
 * *reruns_out counts those second runs.  It is the faster arm only where the paths' minimisers are distinct, which paths of one
 * posterior seldom are.  The result is the plain sequential rule's in every case.
 * Deterministic: the same paths give the same picks, bit for bit.  The draws of path j depend on (seed, j) alone, but a hyper
 * sample's paths are the columns of one multi-column fit, so a path's last bits depend on how many paths share its sample: the
 * picks of a q = 3 call are the first three of a q = 5 call unless two rows tie within those last bits.  No grid is modified; the
 * score accumulator, the feasibility column and the kept posterior are untouched.  The streams of the contexts are
 * ordered by events both ways, as b7_ts_hvi_nominate orders them.
 * B7_ERR_INVALID: a NULL argument (cons may be NULL iff C == 0); C outside 0..B7_TS_FEAS_CMAX; a threshold that is not finite; q or M
 * differ between the contexts.  B7_ERR_STATE, the case named: a context has no kept paths, or its paths are stale (its grid, data or
 * covariance kernel changed since); a context is a member of a group.  B7_ERR_UNSUPPORTED: kept paths left by b7_blr_ts_nominate (the
 * DNGO head is not built here); contexts on different devices; a communicator of more than one rank.
 * Not built: sharded grids and groups, the DNGO head, correlated constraints, trust regions (SCBO's outer loop).
 * Added without a change of B7_ABI_VERSION: the change is additive. */
#define B7_TS_FEAS_CMAX 8
int b7_ts_feas_nominate(b7_ctx *ctx, b7_ctx *const *cons /*C, nullable iff C == 0*/, const double *thresholds /*C*/, int C,
                        double *key_out /*q*/, int *class_out /*q*/, int64_t *best_idx1 /*q*/,
                        double *y_out /*q x (1 + C): the pick's f_j, c_1j .. c_Cj; nullable*/, int *reruns_out /*nullable*/);
/* The same kernels and resolution on host arrays (the b7_hvi_compute of this feature): f is M1 x q, cvals C x M1 x q (nullable iff
 * C == 0), row-major; viol_out (nullable) receives viol as M1 x q, NaN for class -1.  B7_ERR_INVALID: a NULL argument, C outside
 * 0..B7_TS_FEAS_CMAX, a threshold that is not finite, q outside 1..B7_BATCH_MAX, M1 < q.  Like b7_hvi_compute it reads nothing of
 * the context but its device and stream, so a group member or a context with a communicator serves as well.  The kept paths are
 * untouched. */
int b7_ts_feas_compute(b7_ctx *ctx, const double *f /*M1 x q*/, const double *cvals /*C x M1 x q*/, const double *thresholds /*C*/,
                       int64_t M1, int q, int C, double *viol_out /*M1 x q, nullable*/, double *key_out /*q*/, int *class_out /*q*/,
                       int64_t *best_idx1 /*q*/);

/* ---- trust-region nomination (TuRBO: Eriksson, Pearce, Gardner, Turner & Poloczek, NeurIPS 2019).  No counterpart in the
 * reference.  Three host-only pieces (no context, no GPU) that both host languages share, and the device map b7_grid_trust_region
 * (with the grids, above).
 *
 * b7_tr_box: the box around `center` from S hyper samples' ARD lengthscales.  With range_k = maxes_k - mins_k,
 *   log r_k = (1/S) sum_s (1/2) log lenscale_sq[s][k] - log range_k      (geometric mean of the lengthscale relative to the range)
 *   w_k = exp(log r_k - (1/d) sum_j log r_j)                              (prod w = 1: volume length^d prod range before clipping)
 *   half_k = w_k length range_k / 2,   lo_k = max(mins_k, center_k - half_k),   hi_k = min(maxes_k, center_k + half_k).
 * B7_ERR_INVALID: a NULL argument, d outside 1..96, S < 1, lenscale_sq <= 0 or non-finite, range <= 0, length <= 0 or non-finite,
 * a center outside [mins, maxes]. */
int b7_tr_box(int d, int S, const b7_hyp *hyps, const double *center /*d*/, double length, const double *mins /*d*/,
              const double *maxes /*d*/, double *lo /*d*/, double *hi /*d*/);
/* The box's side length and the counters that resize it.  best is NaN while unset (after init and after a restart). */
typedef struct {
  double length, length_init, length_min, length_max, best;
  int succ, fail, succ_tol, fail_tol;
  int restarts;
} b7_tr_state;
/* Defaults (Eriksson et al.'s), each selected by passing <= 0: length_init 0.8, length_min 2^-7, length_max 1.6, succ_tol 3,
 * fail_tol ceil(max(4 / q, d / q)).  B7_ERR_INVALID: NULL, d < 1, q < 1, a NaN or infinite length, or not
 * length_min <= length_init <= length_max. */
int b7_tr_init(b7_tr_state *st, int d, int q, double length_init, double length_min, double length_max, int succ_tol, int fail_tol);
/* One trial's q responses (minimised).  Success iff min y < best - 1e-3 |best|; a NaN never succeeds; the first update after init
 * or a restart sets best and counts as a success.  Success: best updated, succ + 1, fail = 0; otherwise fail + 1, succ = 0.
 * succ == succ_tol: length = min(2 length, length_max), counters zeroed; fail == fail_tol: length /= 2, counters zeroed.
 * length < length_min: *restart_out = 1 (nullable; else 0), length = length_init, best unset, counters zeroed, restarts + 1. */
int b7_tr_update(b7_tr_state *st, const double *y /*q*/, int q, int *restart_out);

/* bayesopt:eval's DNGO branch + nominate as ONE call (bots/bayesopt.lua:65-66, :96 over models/dngo.lua:155-175):
 * b7_blr_fit_x(net, X0, Y0, ...) + b7_blr_basis(net, resident grid) + b7_blr_predict + the acquisition of `spec` (written,
 * not accumulated: ONE point (alpha_prec, beta, mean); b7_blr_eval_nominate_marg below marginalises over S of them) +
 * b7_score_finish_global, enqueued back to back with ONE host
 * synchronisation; the candidates' features are recomputed on every call, as the reference does.  Results as the separate
 * calls (the posterior mean comes out of the feature kernel itself: its last bits may differ from b7_blr_predict's).
 * best_idx1 / global_row_offset / communicator as b7_eval_nominate.  jitter_used (nullable): 0, or < 0 when the head's
 * Cholesky needed utils.math.chol's jitter schedule and the fit was redone through b7_blr_fit_x. */
int b7_blr_eval_nominate(b7_ctx *ctx, const b7_mlp *net, const double *X0, const double *Y0, int N, double alpha_prec,
                         double beta, double mean, const b7_score_spec *spec, int64_t global_row_offset, double *best_val,
                         int64_t *best_idx1, double *jitter_used);

/* The same with the head's hypers MARGINALISED -- models/dngo.lua:109 defaults hyp to 'marginalize' and hands it to the predictor
 * (:174).  gp.models.bayes_linear's own treatment lives in the absent `gp` package (parity unpinned); what is built is the
 * analogue of bayesopt:eval's GP loop (bots/bayesopt.lua:69-79): S samples (alpha_prec[s], beta[s], mean[s]) -- drawn by the host,
 * e.g. with bot7.samplers.slice over the evidence nll_out returns --, S heads fitted over the SAME features (one basis pass over
 * the observations, one over the candidates; for z <= 64 features the S heads are S workgroups of one launch), the acquisition
 * of every head added in sample order, score:div(S), score:max(1).  nll_out (nullable, S entries): the negative log evidence of
 * every head, as b7_blr_fit's.  jitter_used (nullable): 0, or < 0 when a head's Cholesky needed utils.math.chol's jitter schedule
 * and the nomination was redone head by head through b7_blr_fit_x.  S = 1 is b7_blr_eval_nominate. */
int b7_blr_eval_nominate_marg(b7_ctx *ctx, const b7_mlp *net, const double *X0, const double *Y0, int N, int S,
                              const double *alpha_prec, const double *beta, const double *mean, const b7_score_spec *spec,
                              int64_t global_row_offset, double *best_val, int64_t *best_idx1, double *nll_out,
                              double *jitter_used);

/* ---- one process, several GPUs: the reference's single-process trial loop over a sharded grid ----------------- *
 * The reference is ONE LuaJIT process (bots/abstract.lua:155-169); a group lets that one process drive n GPUs, so the
 * trial loop, Torch's RNG stream and the single evaluation of the user's objective per trial (bots/abstract.lua:124)
 * stay as they are.  Member r is a b7_ctx on device_ids[r] holding candidate rows (offset_r, offset_r + M_r] of the grid
 * (contiguous, near-equal shards: the first M % n members hold one row more) and a full copy of the observations.
 * b7_group_eval_nominate enqueues fit + K* + posterior + score on every member's stream without waiting in between,
 * combines the members' exchange records -- ONE grouped ncclAllReduce over xGMI when the devices are distinct
 * (ncclCommInitAll), a merge on the host when members share a device (RCCL refuses that; it is how the sharding is
 * exercised on a one-GPU machine) or B7_GROUP_EXCHANGE=host is set -- and waits once per member.  Results are those of
 * the unsharded calls, bit for bit.  A member's grid must only be changed through the group. */
typedef struct b7_group b7_group;
int b7_group_create(b7_group **out, int n, const int *device_ids);   /* device ids may repeat (virtual ranks) */
void b7_group_destroy(b7_group *g);
const char *b7_group_last_error(const b7_group *g);
int b7_group_info(b7_group *g, int *n, int *uses_rccl);
/* Member r, e.g. for model:sample_hypers' density evaluations (b7_gp_fit_hyp / b7_gp_nll_batch on member 0) or
 * b7_profile_*; owned by the group. */
b7_ctx *b7_group_ctx(b7_group *g, int rank);
int b7_group_set_workspace(b7_group *g, int64_t bytes);
int b7_group_gp_set_opts(b7_group *g, const b7_gp_opts *opts);
/* b7_gp_set_kernel on every member. */
int b7_group_gp_set_kernel(b7_group *g, int kernel);
/* b7_grid_sobol / _random / _upload for the whole grid: every member generates (receives) its shard; one-sided maps use
 * the column extremes of the union. */
int b7_group_grid_sobol(b7_group *g, int64_t size, int dims, int64_t skip, const double *mins, const double *maxes);
int b7_group_grid_random(b7_group *g, int64_t size, int dims, uint64_t seed, const double *mins, const double *maxes);
int b7_group_grid_onesided(b7_group *g, const double *mins, const double *maxes);
int b7_group_grid_upload(b7_group *g, const double *X_hid, int64_t M, int d);
/* Rows of the union, its dims, and the members' offsets (n + 1 entries: offsets[n] = M_global); all nullable. */
int b7_group_grid_shape(b7_group *g, int64_t *M_global, int *d, int64_t *offsets);
int b7_group_grid_download(b7_group *g, int64_t row0 /*0-based, in the union*/, int64_t rows, double *out_host);
/* utils.tensor.remove / steal with an index tensor on the union (indices 1-based against the union before the call). */
int b7_group_grid_remove_rows(b7_group *g, const int64_t *idx1, int64_t n, double *rows_out);
/* b7_gp_set_data on every member. */
int b7_group_gp_set_data(b7_group *g, const double *X_obs, const double *Y_obs, int N, int d, int ycols);
/* b7_eval_nominate over the union: best_idx1 is 1-based in the union. */
int b7_group_eval_nominate(b7_group *g, int S, const b7_hyp *hyps, const b7_score_spec *spec, double *best_val,
                           int64_t *best_idx1, double *jitter_out, int *info_out);
/* b7_nominate_commit over the union: the nominee's coordinates (row_out, nullable, d) and its stable deletion on the
 * member that holds it.  When idx1_global is the winner of the last b7_group_eval_nominate the row comes from the
 * exchange record and nothing is copied or waited for. */
int b7_group_nominate_commit(b7_group *g, int64_t idx1_global, double *row_out);

/* EI.compute / conf_bound.compute / max on caller-provided host vectors (M x c mean, M var). */
int b7_ei_compute(b7_ctx *ctx, const double *mean, const double *var, const double *fmin, double tradeoff,
                  int64_t M, int c, double *out);
int b7_cb_compute(b7_ctx *ctx, const double *mean, const double *var, double tradeoff, int upper, double sign,
                  int64_t M, int c, double *out);
/* b7_ei_compute's sibling in log space -- no counterpart in scores/ of the reference (Ament et al., NeurIPS 2023):
 * out[j] = log(sigma_j) + log(phi(z) + z Phi(z)), z = ((fmin - mean_j) - tradeoff) / sigma_j, evaluated as b7_score_logei
 * describes; c > 1 columns: out[j] = log((1/c) sum_k EI_jk) by log-sum-exp over the columns. */
int b7_logei_compute(b7_ctx *ctx, const double *mean, const double *var, const double *fmin, double tradeoff,
                     int64_t M, int c, double *out);
/* b7_logei_compute's sibling for the log probability of improvement: out[j] = log Phi(z), z as above, evaluated as
 * b7_score_logpi describes; c > 1 columns: out[j] = log((1/c) sum_k Phi(z_jk)) by log-sum-exp over the columns. */
int b7_logpi_compute(b7_ctx *ctx, const double *mean, const double *var, const double *fmin, double tradeoff,
                     int64_t M, int c, double *out);
int b7_argmax(b7_ctx *ctx, const double *scores, int64_t M, double *best_val, int64_t *best_idx1);

/* ---- binary constraints: a probit GP classifier by Laplace's method ---------------------------
 * No counterpart in the reference (Gelbart, Snoek & Adams 2014, section 2.3; Rasmussen & Williams 2006, algorithms 3.1 / 3.2).
 * The resident data (b7_gp_set_data) are N <= 128 rows with ONE response column of labels, each exactly 0 or 1, 1 meaning the
 * constraint is VIOLATED; Pr[label = 1 | h] = Phi(h) of a latent GP h with constant prior mean hyp.mean and the context's covariance
 * kernel (b7_gp_set_kernel).  hyp.noise is ignored (the probit link has unit variance) and must still be finite.  A fit is the mode
 * f^ of the latent's posterior by Newton's iteration, run WHOLE inside one kernel launch (csrc/laplace.hip states the rule: at most
 * 32 iterations, stop at |a+ - a|_inf <= 2^-26 max(1, |a+|_inf), step halving on psi), then
 *   Linv = L^-1 W^1/2,  alpha = a = grad log p(labels | f^),  nll = -log q(labels | hyp) (Laplace's approximate evidence)
 * in the regressor's layout, so that every posterior entry point reads it unchanged.  There is no jitter schedule: B = I +
 * W^1/2 K W^1/2 has every eigenvalue >= 1.  iters_out: Newton iterations taken; info_out: bit 0 set when the stopping rule was not met
 * within 32 (results are delivered all the same).  The same call twice gives the same bits; a fit's bits depend neither on the
 * batch, nor on its position in it, nor on the grid.
 * Every entry point below refuses, the case named: labels other than exactly 0 or 1 (B7_ERR_INVALID); N > 128 or more than one
 * response column (B7_ERR_UNSUPPORTED); a communicator of more than one rank (B7_ERR_UNSUPPORTED); a member of a group, no resident
 * data (B7_ERR_STATE).  NULL arguments, lenscale_sq or amp <= 0 or any hyper not finite: B7_ERR_INVALID.  A refusal leaves the
 * context as it was.
 *   b7_clf_nll_batch     the hyper sampler's density: nll of the resident labels under B hyper vectors, B workgroups of one
 *                        launch.  iters_out / info_out nullable.  The context's fit slot, predictions and accumulator are untouched.
 *   b7_clf_fit_hyp       one fit into the context's own fit slot.  Afterwards b7_gp_predict / b7_gp_predict_at return the LATENT
 *                        mean and variance (b7_gp_opts.var_with_noise adds nothing: the fit's noise is 0); nothing else is
 *                        special-cased, and b7_gp_append / b7_gp_fantasize / b7_gp_download's L are not meaningful on such a fit.
 *                        All outputs nullable.
 *   b7_clf_mode_get      f^, a and W of the last b7_clf_fit_hyp, N entries each (all nullable).  B7_ERR_STATE without one, or after
 *                        the data or the covariance kernel changed.
 *   b7_clf_eval_logfeas  S fits side by side, the latent posterior of every sample over the resident grid by the route the
 *                        regressor's nomination takes for that shape -- kept, as b7_eval_posterior keeps one: b7_posterior_get(s)
 *                        serves it --, then log Phi((0 - mu_s) / sqrt(var_s + 1)) per sample, folded by log-sum-exp in sample order
 *                        and divided by S: log Pr[feasible | x] marginalised over the samples.  This leaves exactly the log
 *                        accumulator that b7_eval_nominate(B7_SCORE_LOGPI, fmin = 0) leaves for a regression constraint:
 *                        b7_feas_add_acc(objective, ctx) takes it, b7_score_finish downloads it.  The + 1 is this entry point's own,
 *                        whatever b7_gp_opts.var_with_noise says.  Returns the accumulator's arg-max.  B7_ERR_STATE without a grid;
 *                        B7_ERR_INVALID when the grid's dims differ from the data's.  iters_out / info_out nullable.
 *   b7_probit_compute    the likelihood's three scalar pieces on a host vector z of n entries: log Phi(z), phi(z)/Phi(z) and
 *                        W(z) = -(log Phi)''(z), as the fit evaluates them.  It disturbs nothing. */
int b7_clf_nll_batch(b7_ctx *ctx, int B, const b7_hyp *hyps, double *nll_out /*B*/, int *iters_out /*B*/, int *info_out /*B*/);
int b7_clf_fit_hyp(b7_ctx *ctx, const b7_hyp *hyp, double *nll_out, int *iters_out, int *info_out);
int b7_clf_mode_get(b7_ctx *ctx, double *f_out /*N*/, double *a_out /*N*/, double *W_out /*N*/);
int b7_clf_eval_logfeas(b7_ctx *ctx, int S, const b7_hyp *hyps, double *best_val, int64_t *best_idx1, int *iters_out /*S*/,
                        int *info_out /*S*/);
int b7_probit_compute(b7_ctx *ctx, const double *z, int64_t n, double *logcdf_out /*n*/, double *ratio_out /*n*/, double *w_out /*n*/);

/* ---- likelihood gradients and the gradient-based point estimate of the GP regressor's hypers.  No counterpart in the reference,
 * whose only way from data to hypers is the slice sampler.  Added without a change of B7_ABI_VERSION: the change is additive.
 *
 * The gradient is taken in the sampler's coordinates (b7_gp_slice_sample's theta):
 *   theta = [log lenscale_sq_1 .. log lenscale_sq_d, log amp, log noise, mean]                      d + 3 components
 * and it is the derivative of the value b7_gp_fit_hyp returns in nll_out (one response column).  With Q = inv(K) - alpha alpha',
 * Kf = K - noise I, w = 1 / lenscale_sq and the radial factor g of the context's kernel (ARD-SE: g = k; Matern-5/2:
 * g = (5/3) amp (1 + s) exp(-s)):
 *   d/d log lenscale_sq_k = 1/4 sum_ij Q_ij g_ij (x_ik - x_jk)^2 w_k        d/d log amp = 1/2 sum_ij Q_ij Kf_ij
 *   d/d log noise = 1/2 noise (tr inv(K) - alpha'alpha)  (exactly 0 at noise == 0)     d/d mean = -sum_i alpha_i
 * A jitter the schedule added is a constant on the diagonal.  After the chol(I) fallback (jitter_used = -1) every component is NaN.
 * The same call gives the same bits; they do not depend on how many workgroups run side by side.
 *
 *   b7_gp_fit_hyp_grad   b7_gp_fit_hyp, bit for bit in nll_out, jitter_used, info and the fit it leaves, plus grad_out[d + 3]; the
 *                        gradient is enqueued behind the fit, and the host waits once (a failed plain attempt redoes it after the
 *                        jitter schedule).  nll_out, jitter_used and info are nullable.
 *   b7_gp_nll_grad       the gradient of the fit the context already holds.  B7_ERR_STATE without a GP fit of the resident data (also
 *                        after b7_clf_fit_hyp, a Bayesian-linear fit, b7_gp_append or a nomination: their fits are not b7_gp_fit_hyp's).
 *                        A change of the candidate grid leaves the fit, and this call, as they were.
 * Both: B7_ERR_UNSUPPORTED, the case named, for more than one response column or a communicator of more than one rank;
 * B7_ERR_STATE for a member of a group. */
int b7_gp_fit_hyp_grad(b7_ctx *ctx, const b7_hyp *hyp, double *nll_out, double *grad_out /*d+3*/, double *jitter_used, int *info);
int b7_gp_nll_grad(b7_ctx *ctx, double *grad_out /*d+3*/);

/* A projected limited-memory BFGS with box bounds.  Host-only (no context, no GPU), shared by both host languages.
 *   memory 8, two-loop recursion; a pair (s, y) is skipped where s'y <= 1e-10 |s| |y| (Armijo's test does not ask for positive
 *   curvature), and a skipped pair empties the memory: the next direction is the projected steepest descent
 *   iterates are projected onto [lo, hi]; a component at an active bound whose gradient points outward is held for that step, and
 *   a component with lo == hi is fixed
 *   Armijo backtracking, t = 1, 1/2, .. at most 20 halvings, c1 = 1e-4; a non-finite value or gradient is a failed trial point
 *   it stops on a projected-gradient infinity norm <= gtol (default 1e-5 max(1, |f|)), on max_iters, on max_evals, or on a line
 *   search that finds nothing
 * Deterministic; it never returns a point worse than x0.  fn(user, n, x, &f, g) fills the value and the n gradient components and
 * returns 0; a nonzero return stops the run (B7_LBFGSB_STOPPED) at the best point so far.  f_out, g_out, iters_out, evals_out and
 * status_out are nullable; opts NULL selects every default.  B7_ERR_INVALID: NULL fn, x0, lo, hi or x_out, n outside 1..99, lo > hi,
 * x0 outside the box or not finite. */
typedef int (*b7_objective_fn)(void *user, int n, const double *x, double *f_out, double *g_out /*n*/);
typedef struct {
  int max_iters; /* [50]  iterations (accepted steps); < 0 selects the default, 0 evaluates x0 and returns it */
  int max_evals; /* [0]   cap on the calls of fn; <= 0: none of its own */
  double gtol;   /* [0]   absolute tolerance on the projected gradient; <= 0 selects 1e-5 max(1, |f|) */
} b7_lbfgsb_opts;
#define B7_LBFGSB_CONVERGED 1   /* projected gradient within the tolerance */
#define B7_LBFGSB_MAX_ITERS 2   /* the iteration budget ran out */
#define B7_LBFGSB_MAX_EVALS 4   /* the evaluation budget ran out */
#define B7_LBFGSB_LINESEARCH 8  /* a line search found no acceptable point */
#define B7_LBFGSB_STOPPED 16    /* fn asked to stop */
#define B7_LBFGSB_BAD_START 32  /* f(x0) or its gradient is not finite: x0 is returned */
int b7_lbfgsb_default_opts(b7_lbfgsb_opts *out);
int b7_lbfgsb_minimize(b7_objective_fn fn, void *user, int n, const double *x0, const double *lo /*n*/, const double *hi /*n*/,
                       const b7_lbfgsb_opts *opts, double *x_out /*n*/, double *f_out, double *g_out /*n*/, int *iters_out,
                       int *evals_out, int *status_out);

/* The point estimate of the hypers: b7_lbfgsb_minimize over the resident data (b7_gp_set_data) with b7_gp_fit_hyp_grad as fn, from
 * theta0 inside [lo, hi] (d + 3 entries each, the coordinates above).  A component with lo == hi is fixed (a noiseless model fixes
 * log noise).  A trial point whose factorisation fell back to chol(I), or whose exp() leaves the hypers' domain, is a failed trial
 * point.  There is no prior term: with a box this is BOUNDED MAXIMUM LIKELIHOOD, which is the MAP estimate under the flat box prior
 * of the sampler.  On return the context's fit slot holds the fit at theta_out (b7_gp_predict follows directly), nll_out and
 * grad_out[d + 3] are that fit's, status_out holds B7_LBFGSB_* bits.  Outputs other than theta_out are nullable.  Refusals as
 * b7_gp_fit_hyp_grad's; B7_ERR_INVALID as b7_lbfgsb_minimize's.
 * b7_gp_fit_map_trace_enable(on): keep one record per accepted iterate of the calls that follow, record 0 the start:
 * theta (d + 3) | nll | the step length that led there.  b7_gp_fit_map_trace: the last call's records (records nullable: the counts
 * alone), *width = d + 5; B7_ERR_STATE when there is none. */
int b7_gp_fit_map(b7_ctx *ctx, const double *theta0, const double *lo, const double *hi, const b7_lbfgsb_opts *opts,
                  double *theta_out /*d+3*/, double *nll_out, double *grad_out /*d+3*/, int *iters_out, int *evals_out, int *status_out);
int b7_gp_fit_map_trace_enable(b7_ctx *ctx, int on);
int b7_gp_fit_map_trace(b7_ctx *ctx, double *records, int *n_records, int *width);

/* ---- measurement ------------------------------------------------------------------------------ */

/* HIP-event timers on the context's stream (the stream every kernel of this library is launched on). */
#define B7_MAX_TIMERS 16
int b7_timer_start(b7_ctx *ctx, int slot);
int b7_timer_stop(b7_ctx *ctx, int slot);
int b7_timer_ms(b7_ctx *ctx, int slot, float *ms_out);

/* Per-kernel-phase event timing inside fit/predict/score (off by default: it serialises phases).
 * Phases: "prep" "kxx" "potrf" "trtri" "alpha" "ksx" "post" "score" "argmax" "exchange" "sobol" "remove".
 * b7_profile_get returns the summed milliseconds and launch count since the last reset. */
int b7_profile_enable(b7_ctx *ctx, int on);
int b7_profile_reset(b7_ctx *ctx);
int b7_profile_get(b7_ctx *ctx, const char *phase, double *ms_total, int64_t *launches);

/* How many persistent launches of this context (the one-launch Cholesky of N > 128 observations) ran into a hand-off time-out
 * -- the GPU was shared with somebody else's persistent kernel -- and were redone by the per-panel launch schedule (same bits).
 * A host that keeps its own "the context's fit is current" flag compares the count around b7_gp_nll_batch: when it moved, the
 * fallback used the context's fit slot (see there) and the next predict needs a new fit.  -1 for a null context. */
int b7_persist_fallbacks(b7_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* BOT7HIP_H */
