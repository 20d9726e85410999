// The Gaussian-process entry points: data, hypers, the factorisation with the reference's jitter schedule, fits, batched
// likelihoods, predictions, fantasies, rank-one appends.  Host-side orchestration only: every number is produced by the kernels
// in covar / potrf / potrf_persist / gp_small / kpost_small / posterior / extras.hip.
#include <math.h>
#include <string.h>

#include <chrono>

#include "b7_internal.h"

// Y - mean on the device (padding rows zero): the sampler changes only the hypers, the data stay where they are.  The two
// kernels keep the C symbol names they have always had.
extern "C" __global__ void __launch_bounds__(256) resid_kernel(const double *__restrict__ y, double *__restrict__ r, int64_t nreal,
                                                               int64_t ntotal, double mean) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < ntotal) r[e] = e < nreal ? y[e] - mean : 0.0;
}

extern "C" __global__ void __launch_bounds__(256) resid_batch_kernel(const double *__restrict__ y, double *__restrict__ r, int N,
                                                                     int Npad, const double *__restrict__ mean) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i < Npad) r[(int64_t)b * Npad + i] = i < N ? y[i] - mean[b] : 0.0;
}

void launch_resid_batch(b7_ctx *c, int B, const double *mean_dev) {
  hipLaunchKernelGGL(resid_batch_kernel, dim3((c->Npad + 255) / 256, B), dim3(256), 0, c->stream, (const double *)c->ybuf.p,
                     (double *)c->bresid.p, c->N, c->Npad, mean_dev);
}

// A persistent factorisation timed out on a hand-off: count it and use the launch schedule from here on (three strikes
// switch this context over for good; the arithmetic is the same either way).
void persist_gave_up(b7_ctx *c) {
  c->persist_aborts += 1;
  if (c->potrf_sched == 3) c->potrf_sched_saved = 3;
  c->potrf_sched = 1;
}
static void persist_restore(b7_ctx *c) {
  if (c->potrf_sched_saved == 3 && c->persist_aborts < 3) c->potrf_sched = 3;
}

// One factorisation attempt of K + extra*I; returns dpotrf-style info through *info.
static int try_factor(b7_ctx *c, double extra, int *info, bool with_inverse, FactorNote *note) {
  int two[2] = {0, 0};
  for (int attempt = 0; attempt < 2; ++attempt) {
    B7_TRY(launch_potrf(c, extra, with_inverse, nullptr, note));  // factors (K + extra*I): eps goes on the ORIGINAL matrix, utils/math.lua:190
    B7_HIP(c, hipMemcpyAsync(two, c->info.p, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    if (two[1] == 0) break;
    if (attempt == 1) return b7_fail(c, B7_ERR_HIP, "Cholesky: hand-off time-out (code %d) outside the persistent schedule", two[1]);
    persist_gave_up(c);
  }
  persist_restore(c);
  *info = two[0];
  return B7_OK;
}

// The retries of utils/math.lua:174-202 after a failed plain attempt.
static int jitter_retries(b7_ctx *c, double *jitter_out, bool with_inverse, FactorNote *note) {
  const int N = c->N;
  int info = 1;
  double jitter = 0.0;
  {
    // max_eps = src:norm() (Frobenius) of the N x N matrix that was handed to chol (:174), reduced on the device in
    // a fixed order (it only gates the chol(I) fallback; copying K to the host cost 32 MiB of PCIe at N = 2048)
    double *fro_dev = reinterpret_cast<double *>(reinterpret_cast<char *>(c->info.p) + 16);
    B7_TRY(launch_fro_norm_sq(c, (const double *)c->K.p, N, c->Npad, fro_dev));
    double fro = 0.0;
    B7_HIP(c, hipMemcpyAsync(&fro, fro_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    const double max_eps = sqrt(fro);
    if (max_eps != max_eps)  // the reference's while-loop never ends here (eps > NaN is false); fail instead
      return b7_fail(c, B7_ERR_INVALID, "chol: the matrix contains NaN (check X_obs and the hyper-parameters)");
    double eps = c->opts.jitter_eps;
    for (;;) {
      if (eps > max_eps) {  // :184-186 chol(I)
        jitter = -1.0;
        B7_TRY(launch_set_identity(c));  // L = I, dinv = identity blocks
        c->linv_done = false;  // launch_trtri rebuilds inv(L) from this L and dinv
        if (note) *note = FactorNote();  // ... and launch_alpha computes alpha from that inverse
        break;
      }
      eps = eps * c->opts.jitter_growth;  // :188
      B7_TRY(try_factor(c, eps, &info, with_inverse, note));
      if (info == 0) {
        jitter = eps;
        break;
      }
    }
  }
  *jitter_out = jitter;
  return B7_OK;
}

// utils/math.lua:159-218 on c->K (N x N inside Npad x Npad): plain attempt, then the growing-jitter retries on
// the ORIGINAL matrix; leaves L and dinv on the device.
int chol_with_jitter(b7_ctx *c, double *jitter_out, int *info_first_out, bool with_inverse, FactorNote *note) {
  int info = 0;
  B7_TRY(try_factor(c, 0.0, &info, with_inverse, note));
  *info_first_out = info;
  *jitter_out = 0.0;
  if (info != 0) B7_TRY(jitter_retries(c, jitter_out, with_inverse, note));
  return B7_OK;
}

int64_t predict_chunk(const b7_ctx *c, int64_t M) {
  int64_t chunk = (int64_t)(c->ks_bytes / (sizeof(double) * (size_t)c->Npad)) / B7_MROWS * B7_MROWS;
  if (chunk < B7_MROWS) chunk = B7_MROWS;
  const int64_t Mpad = round_up(M, B7_MROWS);
  return chunk > Mpad ? Mpad : chunk;
}

int predict_into(b7_ctx *c, const FitSet &fit, const double *xq, int64_t M, double *mu, double *var) {
  if (M == 0) return B7_OK;
  if (c->kpost_small && c->model_kind == 0 && kpost_small_applies(c))  // small fits: one kernel, K* never stored
    return launch_kpost_small(c, fit, xq, M, mu, var, M);
  const int64_t chunk = predict_chunk(c, M), Mpad = round_up(M, B7_MROWS);
  B7_TRY(b7_ensure(c, c->ks, sizeof(double) * (size_t)chunk * c->Npad));
  for (int64_t row0 = 0; row0 < M; row0 += chunk) {
    int64_t rows = Mpad - row0 < chunk ? Mpad - row0 : chunk;
    B7_TRY(launch_ksx(c, fit, xq, row0, rows, M, c->dfit, (double *)c->ks.p, mu, c->ycols));
    if (c->ycols > 1) B7_TRY(launch_mean_multi(c, fit, (const double *)c->ks.p, row0, rows, M, mu));
    B7_TRY(launch_post(c, fit, (const double *)c->ks.p, row0, rows, M, var));
  }
  return B7_OK;
}

int batch_slots_ensure(b7_ctx *c, int B, int groups) {
  const size_t n = (size_t)c->Npad, one = sizeof(double) * (size_t)B;
  if (groups & B7_SLOTS_OPERANDS) {
    B7_TRY(b7_ensure(c, c->bw, one * FitSet::s_w(c->Npad, c->dpad)));
    B7_TRY(b7_ensure(c, c->bzsc, one * FitSet::s_zsc(c->Npad, c->dpad)));
    B7_TRY(b7_ensure(c, c->bzss, one * FitSet::s_zss(c->Npad, c->dpad)));
  }
  if (groups & B7_SLOTS_LINV) B7_TRY(b7_ensure(c, c->bLinv, one * FitSet::s_Linv(c->Npad, c->dpad)));
  if (groups & B7_SLOTS_ALPHA) B7_TRY(b7_ensure(c, c->balpha, one * FitSet::s_alpha(c->Npad, c->dpad)));
  if (groups & B7_SLOTS_FACTOR) {
    B7_TRY(b7_ensure(c, c->bK, one * n * n));
    B7_TRY(b7_ensure(c, c->bL, one * n * n));
    B7_TRY(b7_ensure(c, c->bdinv, one * n * B7_PANEL));
    B7_TRY(b7_ensure(c, c->bresid, one * n));
  }
  return B7_OK;
}

int check_hyp(b7_ctx *c, const b7_hyp *hyp, int d) {
  if (!hyp || !hyp->lenscale_sq) return b7_fail(c, B7_ERR_INVALID, "gp_fit_hyp: NULL argument");
  for (int k = 0; k < d; ++k)
    if (!(hyp->lenscale_sq[k] > 0.0)) return b7_fail(c, B7_ERR_INVALID, "gp_fit: lenscale_sq[%d] must be > 0", k);
  if (!(hyp->amp > 0.0) || !(hyp->noise >= 0.0)) return b7_fail(c, B7_ERR_INVALID, "gp_fit: amp > 0, noise >= 0");
  return B7_OK;
}

// residual, observation scaling and K(X,X) of one hyper sample whose lengthscales are (on their way) at ls_dev
int fit_front(b7_ctx *c, const b7_hyp *hyp, const double *ls_dev) {
  const int N = c->N, d = c->dfit, ycols = c->ycols;
  c->fitted = false;
  c->model_kind = 0;
  c->predicted = false;
  c->amp = hyp->amp;
  c->noise = hyp->noise;
  c->mean = hyp->mean;
  c->gfit = false;
  const int64_t ntotal = (int64_t)c->Npad * ycols;
  hipLaunchKernelGGL(resid_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, c->stream,
                     (const double *)c->ybuf.p, (double *)c->resid.p, (int64_t)N * ycols, ntotal, hyp->mean);
  B7_TRY(launch_prep_obs(c, (const double *)c->xobs.p, ls_dev, N, d));
  return launch_kxx(c, hyp->noise);
}

// then_predict: the posterior over the resident grid is enqueued right behind the fit, before the host has seen the
// pivot report, and the host only waits for the report (an event), not for the prediction.  If the report says the
// plain attempt failed (rare), the speculative prediction is thrown away and redone after the jitter schedule.
int fit_hyp_core(b7_ctx *c, const b7_hyp *hyp, double *nll_out, double *jitter_used, int *info_out,
                        bool then_predict) {
  if (!c) return B7_ERR_INVALID;
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_fit_hyp: call b7_gp_set_data first");
  const int N = c->N, d = c->dfit, ycols = c->ycols;
  B7_TRY(check_hyp(c, hyp, d));
  B7_HIP(c, hipSetDevice(c->device));

  // the only upload of a fit: d lengthscales, through the pinned block's vector slot (free again once the synchronisation
  // that ends every fit has passed); amp / noise / mean travel as kernel arguments
  double *ls_stage = c->pinned->vec, *ls_dev = b7_scratch(c)->lenscale;
  memcpy(ls_stage, hyp->lenscale_sq, sizeof(double) * d);
  // N <= 128, d <= 32, one response column: residual, observation scaling, K(X,X), factorisation, inverse and alpha are ONE
  // workgroup of ONE launch (gp_small.hip) with the d + 3 hypers in the kernel arguments; the kernel also leaves the
  // lengthscales in the scratch block (ScratchBlock::lenscale).  K itself is not kept: a failed pivot
  // (rare) assembles it through the general front end before the jitter schedule runs
  const bool small = fit_small_applies(c);
  if (small) {
    ls_stage[d] = hyp->amp, ls_stage[d + 1] = hyp->noise, ls_stage[d + 2] = hyp->mean;
    c->fitted = false;
    c->model_kind = 0;
    c->predicted = false;
    c->amp = hyp->amp;
    c->noise = hyp->noise;
    c->mean = hyp->mean;
    c->gfit = false;
  } else {
    B7_HIP(c, hipMemcpyAsync(ls_dev, ls_stage, sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
    B7_TRY(fit_front(c, hyp, ls_dev));
  }

  // First attempt with everything that follows it enqueued BEFORE the host looks at the pivot report: when the
  // inverse came out of the factorisation itself, alpha and the likelihood terms do not need the host, and one
  // small copy (info + terms) with one synchronisation ends the fit.  A failed pivot (rare) falls back to the
  // jitter schedule and redoes the tail.
  FitBlock &blk = c->pinned->fit;  // pinned: the copy needs no pageable staging
  double *terms_dev = reinterpret_cast<double *>(reinterpret_cast<char *>(c->info.p) + 16);
  const size_t blk_bytes = 16 + sizeof(double) * (nll_out ? 1 + ycols : 0);
  bool tail_done = false;
  FactorNote note;  // what the last factorisation already did for the launch_alpha behind it
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (small && attempt == 0) {
      B7_TRY(launch_fit_small(c, 1, nullptr, ls_stage, ls_dev, (double *)c->w.p, (double *)c->zsc.p, (double *)c->zss.p, (double *)c->L.p,
                              (double *)c->Linv.p, (double *)c->dinv.p, (double *)c->alpha.p, (double *)c->resid.p, (int *)c->info.p,
                              nullptr));
      c->linv_done = true;
      tail_done = true;
      if (nll_out) B7_TRY(launch_nll_terms(c, terms_dev));
    } else {
      B7_TRY(launch_potrf(c, 0.0, true, nullptr, &note));
      tail_done = c->linv_done;
      if (tail_done) {
        B7_TRY(launch_alpha(c, nullptr, 0, note));
        if (nll_out) B7_TRY(launch_nll_terms(c, terms_dev));
      }
    }
    if (tail_done && c->grad_hook) B7_TRY(nll_grad_enqueue(c));
    B7_HIP(c, hipMemcpyAsync(&blk, c->info.p, tail_done ? blk_bytes : 16, hipMemcpyDeviceToHost, c->stream));
    if (then_predict && tail_done) {
      B7_HIP(c, hipEventRecord(c->ev_fit, c->stream));
      c->fitted = true;  // for the launchers; withdrawn below if the report says otherwise
      B7_TRY(predict_into(c, ctx_fit(c), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->mu.p, (double *)c->var.p));
      B7_HIP(c, hipEventSynchronize(c->ev_fit));
    } else {
      B7_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (blk.info[1] == 0) break;
    c->fitted = false;
    // the persistent schedule gave up on a hand-off (its workgroups were not all resident, e.g. the GPU is shared
    // with another process's persistent kernel): same arithmetic through the launch schedule, which cannot stall
    if (attempt == 1) return b7_fail(c, B7_ERR_HIP, "Cholesky: hand-off time-out (code %d) outside the persistent schedule", blk.info[1]);
    persist_gave_up(c);
  }
  const int info_first = blk.info[0];
  double jitter = 0.0;
  bool predicted = then_predict && tail_done;
  if (info_first != 0) {
    c->fitted = false;
    if (small) B7_TRY(fit_front(c, hyp, ls_dev));  // K(X,X) for the retries (the one-launch fit does not keep it)
    B7_TRY(jitter_retries(c, &jitter, true, &note));
    tail_done = false;
    predicted = false;
  }
  if (!tail_done) {
    B7_TRY(launch_trtri(c));
    B7_TRY(launch_alpha(c, nullptr, 0, note));
    if (nll_out) B7_TRY(launch_nll_terms(c, terms_dev));
    if (c->grad_hook) B7_TRY(nll_grad_enqueue(c));
    B7_HIP(c, hipMemcpyAsync(&blk, c->info.p, blk_bytes, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (then_predict && !predicted) {
    c->fitted = true;
    B7_TRY(predict_into(c, ctx_fit(c), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->mu.p, (double *)c->var.p));
  }
  if (nll_out)
    for (int k = 0; k < ycols; ++k) nll_out[k] = 0.5 * blk.terms[1 + k] + blk.terms[0] + 0.5 * N * log(2.0 * M_PI);
  if (jitter_used) *jitter_used = jitter;
  if (info_out) *info_out = info_first;
  persist_restore(c);
  c->fitted = true;
  c->gfit = true, c->gfit_jitter = jitter, c->gfit_N = c->N;
  return B7_OK;
}

int copy_out_mu_var(b7_ctx *c, const void *mu, const void *var, int64_t M, int cols, double *mean_host, double *var_host, bool wait) {
  if (mean_host) B7_HIP(c, hipMemcpyAsync(mean_host, mu, sizeof(double) * (size_t)M * cols, hipMemcpyDeviceToHost, c->stream));
  if (var_host) B7_HIP(c, hipMemcpyAsync(var_host, var, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  if (mean_host || var_host || wait) B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

extern "C" {

// ---- model ---------------------------------------------------------------------------------------------
int b7_gp_default_opts(b7_gp_opts *o) {
  if (!o) return B7_ERR_INVALID;
  o->jitter_eps = 1e-8;     // utils/math.lua:175
  o->jitter_growth = 1.1;   // utils/math.lua:176
  o->var_with_noise = 0;
  o->var_clamp = 0;
  o->var_min = 0.0;
  return B7_OK;
}

int b7_gp_set_opts(b7_ctx *c, const b7_gp_opts *o) {
  if (!c || !o) return B7_ERR_INVALID;
  if (!(o->jitter_eps > 0.0) || !(o->jitter_growth > 1.0))
    return b7_fail(c, B7_ERR_INVALID, "gp opts: jitter_eps must be > 0 and jitter_growth > 1");
  c->opts = *o;
  return B7_OK;
}

int b7_gp_set_kernel(b7_ctx *c, int kernel) {
  if (!c) return B7_ERR_INVALID;
  if (kernel != B7_KERNEL_ARDSE && kernel != B7_KERNEL_MATERN52)
    return b7_fail(c, B7_ERR_INVALID, "gp_set_kernel: unknown kernel %d", kernel);
  if (kernel == c->kernel) return B7_OK;
  // what a fit under the old kernel left behind goes; the resident data and grid stay (no nomination leaves a score pending
  // in the context: ScoreParams belongs to the call that made it)
  c->kernel = kernel;
  c->fitted = false;
  c->predicted = false;
  post_forget(c);  // a kept posterior (b7_eval_posterior) is of the kernel it was made under
  return B7_OK;
}

int b7_gp_set_data(b7_ctx *c, const double *X, const double *Y, int N, int d, int ycols) {
  if (!c) return B7_ERR_INVALID;
  if (!X || !Y) return b7_fail(c, B7_ERR_INVALID, "gp_set_data: NULL argument");
  if (N < 1 || d < 1 || ycols < 1) return b7_fail(c, B7_ERR_INVALID, "gp_set_data: N %d d %d ycols %d", N, d, ycols);
  if (d > B7_MAX_D) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_set_data: d %d > %d", d, B7_MAX_D);
  if (ycols > 256) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_set_data: ycols %d > 256", ycols);
  B7_HIP(c, hipSetDevice(c->device));
  c->fitted = false;
  c->have_data = false;
  c->predicted = false;  // the score accumulator survives: marginalisation adds across fits (bots/bayesopt.lua:73-78)
  post_forget(c);        // a kept posterior (b7_eval_posterior) is of the data it was made from
  c->N = N;
  c->Npad = npad_of(c, N);
  c->dfit = d;
  c->dpad = b7_dpad_class(d);
  c->ycols = ycols;
  c->yld = (ycols == 1) ? 1 : (int)round_up(ycols, 64);
  const size_t np = (size_t)c->Npad, nn = np * np * sizeof(double);
  B7_TRY(b7_ensure(c, c->xobs, sizeof(double) * np * d));  // room for b7_gp_append up to Npad rows
  B7_TRY(b7_ensure(c, c->ybuf, sizeof(double) * np * ycols));
  B7_TRY(b7_ensure(c, c->w, sizeof(double) * c->dpad));
  B7_TRY(b7_ensure(c, c->zsc, sizeof(double) * np * c->dpad));
  B7_TRY(b7_ensure(c, c->zss, sizeof(double) * np));
  B7_TRY(b7_ensure(c, c->K, nn));
  B7_TRY(b7_ensure(c, c->L, nn));
  B7_TRY(b7_ensure(c, c->Linv, nn));
  B7_TRY(b7_ensure(c, c->W, nn));
  B7_TRY(b7_ensure(c, c->dinv, sizeof(double) * (np + B7_PANEL) * B7_PANEL));
  B7_TRY(b7_ensure(c, c->alpha, sizeof(double) * np * c->yld));
  B7_TRY(b7_ensure(c, c->resid, sizeof(double) * np * ycols));
  B7_TRY(b7_ensure(c, c->info, B7_INFO_BYTES));
  B7_HIP(c, hipMemcpyAsync(c->xobs.p, X, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(c->ybuf.p, Y, sizeof(double) * (size_t)N * ycols, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays are consumed
  c->have_data = true;
  return B7_OK;
}

int b7_gp_nll_batch(b7_ctx *c, int B, const double *lenscale_sq, const double *amp, const double *noise,
                    const double *mean, double *nll_out, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_nll_batch: call b7_gp_set_data first");
  if (B < 1 || !lenscale_sq || !amp || !noise || !mean || !nll_out) return b7_fail(c, B7_ERR_INVALID, "gp_nll_batch: bad arguments");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_nll_batch: one response column only");
  if (c->Npad > B7_PERSIST_NMAX) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_nll_batch: N > 4096 (evaluate with b7_gp_fit_hyp one by one)");
  const int N = c->N, n = c->Npad, d = c->dfit, nb = n / B7_PANEL;
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k < d; ++k)
      if (!(lenscale_sq[(size_t)b * d + k] > 0.0)) return b7_fail(c, B7_ERR_INVALID, "gp_nll_batch: lenscale_sq[%d][%d] must be > 0", b, k);
    if (!(amp[b] > 0.0) || !(noise[b] >= 0.0)) return b7_fail(c, B7_ERR_INVALID, "gp_nll_batch: amp > 0, noise >= 0 (fit %d)", b);
  }
  B7_HIP(c, hipSetDevice(c->device));
  // hypers in and results out through ONE block of pinned, device-mapped host memory, laid out
  // [B x d lengthscales | B amp | B noise | B mean][2 B terms][4 B ints of pivot reports][completion word]
  const size_t hyp_doubles = (size_t)B * (d + 3), need = sizeof(double) * (hyp_doubles + 2 * (size_t)B) + sizeof(int) * (4 * (size_t)B + 4);
  B7_TRY(b7_pin_ensure(c, c->pin_nll, need, true));
  double *pack = static_cast<double *>(c->pin_nll.host), *terms = pack + hyp_doubles;  // host side of the block
  int *info = reinterpret_cast<int *>(terms + 2 * (size_t)B);
  const HypPack hp = hyp_pack(pack, B, d);
  memcpy(hp.ls, lenscale_sq, sizeof(double) * (size_t)B * d);
  memcpy(hp.amp, amp, sizeof(double) * B);
  memcpy(hp.noise, noise, sizeof(double) * B);
  memcpy(hp.mean, mean, sizeof(double) * B);
  if (c->nll_small && gp_small_applies(c)) {
    // N <= 128, d <= 32: every evaluation is ONE workgroup of ONE launch (gp_small.hip), observations in, two numbers out.
    // A fit whose plain factorisation fails (rare) sends the whole batch through the general path below, jitter schedule
    // included.  The kernel reads the B x (d + 3) numbers and writes its 2 doubles + 4 ints per evaluation straight across
    // the bus -- no copy calls, one launch, one wait
    double *pack_dev = static_cast<double *>(c->pin_nll.dev);
    int *info_dev = reinterpret_cast<int *>(pack_dev + hyp_doubles + 2 * (size_t)B);
    // a single evaluation (every density call of the slice sampler) is waited for on a word the kernel sets after its results:
    // the host sees them as soon as they have crossed the bus instead of after the dispatch has retired and the runtime
    // has noticed.  The stream stays ordered (later launches queue behind the kernel); a kernel that has not answered after
    // 200 us is waited for the ordinary way, which also surfaces a fault.
    volatile unsigned *done = reinterpret_cast<volatile unsigned *>(info + 4 * (size_t)B);
    *done = 0u;
#ifdef B7_DIAG
    if (c->nll_small == 2)  // round 3's four-wave kernel (nll_small.hip, diagnostic build only): the bit-for-bit reference of the likelihood
      B7_TRY(launch_nll_small(c, B, pack_dev, pack, pack_dev + hyp_doubles, info_dev, reinterpret_cast<unsigned *>(info_dev + 4 * (size_t)B)));
    else
#endif
      B7_TRY(launch_nll_small8(c, B, pack_dev, pack, pack_dev + hyp_doubles, info_dev, reinterpret_cast<unsigned *>(info_dev + 4 * (size_t)B)));
    bool answered = false;
    if (B == 1) {
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned spins = 0; !answered && c->spin_us > 0; ++spins) {
        answered = __atomic_load_n(const_cast<const unsigned *>(done), __ATOMIC_ACQUIRE) != 0u;
        if (!answered && (spins & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(c->spin_us < 200 ? c->spin_us : 200)) break;
      }
    }
    if (!answered) B7_HIP(c, hipStreamSynchronize(c->stream));
    bool clean = true;
    for (int b = 0; b < B; ++b) clean = clean && info[(size_t)b * 4] == 0;
    if (clean) {
      const double c0s = 0.5 * N * log(2.0 * M_PI);
      for (int b = 0; b < B; ++b) {
        nll_out[b] = 0.5 * terms[(size_t)b * 2] + terms[(size_t)b * 2 + 1] + c0s;
        if (jitter_out) jitter_out[b] = 0.0;
        if (info_out) info_out[b] = 0;
      }
      return B7_OK;
    }
  }
  const size_t fw = persist_flag_words_host(nb), nn = (size_t)n * n;
  B7_TRY(b7_ensure(c, c->bhyp, sizeof(double) * (size_t)B * (d + 3)));
  B7_TRY(batch_slots_ensure(c, B, B7_SLOTS_OPERANDS | B7_SLOTS_FACTOR));
  // one block: [2 B doubles of likelihood terms][4 B ints of pivot reports][B x fw flag words] -- reports and flags are zeroed
  // by one memset, terms and reports come back in one copy; the jitter schedule's norm goes into bterms
  const size_t head_bytes = sizeof(double) * 2 * (size_t)B + sizeof(int) * 4 * (size_t)B;
  B7_TRY(b7_ensure(c, c->bflags, head_bytes + sizeof(unsigned) * B * fw));
  B7_TRY(b7_ensure(c, c->bterms, 64));
  // all hypers in one upload from the pinned block (no pageable staging)
  double *hyp_dev = (double *)c->bhyp.p;
  B7_HIP(c, hipMemcpyAsync(hyp_dev, pack, sizeof(double) * hyp_doubles, hipMemcpyHostToDevice, c->stream));
  const HypPack hd = hyp_pack(hyp_dev, B, d);
  launch_resid_batch(c, B, hd.mean);
  B7_TRY(launch_kxx_batch(c, B, hd.ls, hd.amp, hd.noise, (double *)c->bw.p, (double *)c->bzsc.p, (double *)c->bzss.p,
                          (double *)c->bK.p));
  // the likelihood terms and the pivot reports of all fits sit side by side on the device ([2 B doubles][4 B ints]) and come
  // back in ONE copy into the pinned block
  double *terms_dev = (double *)c->bflags.p;
  int *info_dev = reinterpret_cast<int *>(terms_dev + 2 * (size_t)B);
  unsigned *flags_dev = reinterpret_cast<unsigned *>(info_dev + 4 * (size_t)B);
  B7_TRY(launch_nll_batch(c, B, (const double *)c->bK.p, (double *)c->bL.p, (double *)c->bdinv.p, flags_dev,
                          info_dev, (const double *)c->bresid.p, terms_dev));
  B7_HIP(c, hipMemcpyAsync(terms, terms_dev, sizeof(double) * 2 * (size_t)B + sizeof(int) * 4 * (size_t)B, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  const double c0 = 0.5 * N * log(2.0 * M_PI);
  for (int b = 0; b < B; ++b) {
    double jitter = 0.0;
    const int info_first = info[(size_t)b * 4];
    int bad = info_first, aborted = info[(size_t)b * 4 + 1];
    const double *Kb = (const double *)c->bK.p + b * nn;
    double *Lb = (double *)c->bL.p + b * nn, *dib = (double *)c->bdinv.p + (size_t)b * n * B7_PANEL;
    unsigned *fb = flags_dev + b * fw;
    int *ib = info_dev + (size_t)b * 4;
    const double *rb = (const double *)c->bresid.p + (size_t)b * n;
    double *tb = terms_dev + 2 * (size_t)b;
    auto redo = [&](double extra) -> int {  // this fit alone (it has the whole chip), eps on the diagonal
      B7_TRY(launch_nll_one(c, Kb, Lb, dib, fb, ib, rb, tb, extra));
      int two[2];
      B7_HIP(c, hipMemcpyAsync(two, ib, sizeof(two), hipMemcpyDeviceToHost, c->stream));
      B7_HIP(c, hipMemcpyAsync(&terms[(size_t)b * 2], tb, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      B7_HIP(c, hipStreamSynchronize(c->stream));
      bad = two[0];
      aborted = two[1];
      return B7_OK;
    };
    if (aborted) {  // a hand-off timed out (the chip was shared): once more, alone
      c->persist_aborts += 1;
      B7_TRY(redo(0.0));
    }
    if (aborted) {
      // still no luck with the persistent schedule (the GPU is occupied by somebody else's persistent kernel): this
      // likelihood through the launch schedule, which cannot stall -- b7_gp_fit_hyp's own fallback, jitter schedule
      // included.  It runs in the context's fit slot, so the current fit is gone afterwards (the one case in which this
      // call does not leave it alone; the next predict asks for a fit with B7_ERR_STATE).
      b7_hyp h{lenscale_sq + (size_t)b * d, amp[b], noise[b], mean[b]};
      persist_gave_up(c);
      double nll1 = 0.0, jit1 = 0.0;
      int info1 = 0;
      const int rc1 = fit_hyp_core(c, &h, &nll1, &jit1, &info1, false);
      c->fitted = false;
      c->predicted = false;
      B7_TRY(rc1);
      nll_out[b] = nll1;
      if (jitter_out) jitter_out[b] = jit1;
      if (info_out) info_out[b] = info1;
      continue;
    }
    if (bad != 0) {  // the jitter schedule of utils/math.lua:174-202 for this fit
      double *fro_dev = (double *)c->bterms.p;
      B7_TRY(launch_fro_norm_sq(c, Kb, N, n, fro_dev));
      double fro = 0.0;
      B7_HIP(c, hipMemcpyAsync(&fro, fro_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
      B7_HIP(c, hipStreamSynchronize(c->stream));
      const double max_eps = sqrt(fro);
      if (max_eps != max_eps) return b7_fail(c, B7_ERR_INVALID, "gp_nll_batch: K of fit %d contains NaN", b);
      double eps = c->opts.jitter_eps;
      while (bad != 0) {
        if (eps > max_eps) return b7_fail(c, B7_ERR_INVALID, "gp_nll_batch: fit %d cannot be factored", b);
        eps = eps * c->opts.jitter_growth;
        B7_TRY(redo(eps));
        if (aborted) return b7_fail(c, B7_ERR_HIP, "gp_nll_batch: hand-off time-out (code %d) in fit %d", aborted, b);
        jitter = eps;
      }
    }
    nll_out[b] = 0.5 * terms[(size_t)b * 2] + terms[(size_t)b * 2 + 1] + c0;
    if (jitter_out) jitter_out[b] = jitter;
    if (info_out) info_out[b] = info_first;
  }
  return B7_OK;
}

int b7_gp_fit_hyp(b7_ctx *c, const b7_hyp *hyp, double *nll_out, double *jitter_used, int *info_out) {
  return fit_hyp_core(c, hyp, nll_out, jitter_used, info_out, false);
}

int b7_gp_fit(b7_ctx *c, const double *X, const double *Y, int N, int d, int ycols, const b7_hyp *hyp,
              double *nll_out, double *jitter_used, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (!hyp || !hyp->lenscale_sq) return b7_fail(c, B7_ERR_INVALID, "gp_fit: NULL argument");
  B7_TRY(b7_gp_set_data(c, X, Y, N, d, ycols));
  return b7_gp_fit_hyp(c, hyp, nll_out, jitter_used, info_out);
}

int b7_gp_predict_hyp(b7_ctx *c, const b7_hyp *hyp, double *mean_host, double *var_host, double *nll_out,
                      double *jitter_used, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "gp_predict_hyp: call b7_gp_set_data first");
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "gp_predict_hyp: no candidate grid on this context");
  if (c->d != c->dfit) return b7_fail(c, B7_ERR_INVALID, "gp_predict_hyp: grid dims %d != data dims %d", c->d, c->dfit);
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)c->M * c->ycols));
  B7_TRY(b7_ensure(c, c->var, sizeof(double) * (size_t)c->M));
  B7_TRY(fit_hyp_core(c, hyp, nll_out, jitter_used, info_out, true));
  c->predicted = true;
  c->Mpred = c->M;
  return copy_out_mu_var(c, c->mu.p, c->var.p, c->M, c->ycols, mean_host, var_host);
}

int b7_chol(b7_ctx *c, const double *src, int n, double *res, double *jitter_used, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (!src || !res || n < 1) return b7_fail(c, B7_ERR_INVALID, "chol: bad arguments");
  B7_HIP(c, hipSetDevice(c->device));
  c->fitted = false;
  c->have_data = false;
  c->predicted = false;
  post_forget(c);
  c->N = n;
  c->Npad = npad_of(c, n);
  const size_t np = (size_t)c->Npad, nn = np * np * sizeof(double);
  B7_TRY(b7_ensure(c, c->K, nn));
  B7_TRY(b7_ensure(c, c->L, nn));
  B7_TRY(b7_ensure(c, c->dinv, sizeof(double) * (np + B7_PANEL) * B7_PANEL));
  B7_TRY(b7_ensure(c, c->info, B7_INFO_BYTES));
  std::vector<double> Kp(np * np, 0.0);
  for (size_t i = 0; i < np; ++i) {
    if (i < (size_t)n)
      memcpy(&Kp[i * np], src + i * (size_t)n, sizeof(double) * n);
    else
      Kp[i * np + i] = 1.0;
  }
  B7_HIP(c, hipMemcpy(c->K.p, Kp.data(), nn, hipMemcpyHostToDevice));
  int info_first = 0;
  double jitter = 0.0;
  B7_TRY(chol_with_jitter(c, &jitter, &info_first, false));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  B7_HIP(c, hipMemcpy2D(res, sizeof(double) * n, c->L.p, sizeof(double) * np, sizeof(double) * n, n,
                        hipMemcpyDeviceToHost));
  if (jitter_used) *jitter_used = jitter;
  if (info_out) *info_out = info_first;
  return B7_OK;
}

int b7_gp_predict(b7_ctx *c, double *mean_host, double *var_host) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 0) return b7_fail(c, B7_ERR_STATE, "gp_predict: no GP fit on this context");
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "gp_predict: no candidate grid on this context");
  if (c->d != c->dfit) return b7_fail(c, B7_ERR_INVALID, "gp_predict: grid dims %d != fit dims %d", c->d, c->dfit);
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)c->M * c->ycols));
  B7_TRY(b7_ensure(c, c->var, sizeof(double) * (size_t)c->M));
  B7_TRY(predict_into(c, ctx_fit(c), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->mu.p, (double *)c->var.p));
  c->predicted = true;
  c->Mpred = c->M;
  return copy_out_mu_var(c, c->mu.p, c->var.p, c->M, c->ycols, mean_host, var_host);
}

int b7_gp_predict_at(b7_ctx *c, const double *X1, int64_t M1, double *mean_host, double *var_host) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 0) return b7_fail(c, B7_ERR_STATE, "gp_predict_at: no GP fit on this context");
  if (M1 < 0 || (!X1 && M1 > 0)) return b7_fail(c, B7_ERR_INVALID, "gp_predict_at: bad X1/M1");
  if (M1 == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)M1 * c->dfit));
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (size_t)M1 * c->ycols));
  B7_TRY(b7_ensure(c, c->tmpvar, sizeof(double) * (size_t)M1));
  B7_HIP(c, hipMemcpyAsync(c->tmpgrid.p, X1, sizeof(double) * (size_t)M1 * c->dfit, hipMemcpyHostToDevice, c->stream));
  B7_TRY(predict_into(c, ctx_fit(c), (const double *)c->tmpgrid.p, M1, (double *)c->tmpmu.p, (double *)c->tmpvar.p));
  return copy_out_mu_var(c, c->tmpmu.p, c->tmpvar.p, M1, c->ycols, mean_host, var_host, true);  // the wait also releases X1
}

int b7_gp_fantasize(b7_ctx *c, const double *X_pend, int P, int n, uint64_t seed, double *Y_out, double *mean_out,
                    double *cov_out) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 0) return b7_fail(c, B7_ERR_STATE, "gp_fantasize: no GP fit on this context");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_fantasize: the fit must have one response column");
  if (!X_pend || P < 1 || n < 1 || !Y_out) return b7_fail(c, B7_ERR_INVALID, "gp_fantasize: bad arguments");
  if (P > 64) return b7_fail(c, B7_ERR_UNSUPPORTED, "gp_fantasize: %d pending points > 64", P);
  B7_HIP(c, hipSetDevice(c->device));
  const int np = c->Npad, d = c->dfit, dp = c->dpad;
  // workspace carve-up (doubles): xp 64*d | zsc_p 64*dp | zsh_p 64 | kp 64*np | vt 64*np | g 4096 | kpp 4096 |
  // S 4096 | dinv 4096 | mu 64 | out P*n | info
  size_t need = (size_t)64 * d + (size_t)64 * dp + 64 + (size_t)2 * 64 * np + 4 * 4096 + 64 + (size_t)P * n + 16;
  B7_TRY(b7_ensure(c, c->fant, need * sizeof(double)));
  double *xp = (double *)c->fant.p, *zscp = xp + (size_t)64 * d, *zshp = zscp + (size_t)64 * dp, *kp = zshp + 64;
  double *vt = kp + (size_t)64 * np, *g = vt + (size_t)64 * np, *kpp = g + 4096, *S = kpp + 4096, *dv = S + 4096;
  double *mu = dv + 4096, *out = mu + 64;
  int *info_dev = (int *)(out + (size_t)P * n + 2);
  B7_HIP(c, hipMemcpyAsync(xp, X_pend, sizeof(double) * (size_t)P * d, hipMemcpyHostToDevice, c->stream));
  // K(Xp, X) with the fused mean, then V' = K(Xp,X) L^-T and G = V'V
  B7_TRY(launch_ksx(c, ctx_fit(c), xp, 0, 64, P, d, kp, mu, 1));
  B7_TRY(launch_gemm_nt(c, kp, np, (const double *)c->Linv.p, np, vt, np, 64, np, np));
  B7_TRY(launch_gemm_nt(c, vt, np, vt, np, g, 64, 64, 64, np));
  // K(Xp, Xp): the pending points as their own observation set, scaled with the fit's lengthscales
  double *ls_dev = b7_scratch(c)->lenscale;  // of the current fit
  B7_TRY(launch_prep_obs_aux(c, xp, ls_dev, P, 64, zscp, zshp));
  const ObsSet op{zscp, zshp, 64};
  B7_TRY(launch_k_generic(c, xp, 64, P, op, kpp));
  B7_TRY(launch_fantasy_cov(c, kpp, g, S, P, c->opts.var_with_noise ? c->noise : 0.0));
  if (cov_out) {
    B7_HIP(c, hipStreamSynchronize(c->stream));
    B7_HIP(c, hipMemcpy2D(cov_out, sizeof(double) * P, S, sizeof(double) * 64, sizeof(double) * P, P,
                          hipMemcpyDeviceToHost));
  }
  // factor with the same jitter schedule as utils.math.chol (eps on the ORIGINAL matrix: keep a copy in kpp)
  B7_HIP(c, hipMemcpyAsync(kpp, S, sizeof(double) * 4096, hipMemcpyDeviceToDevice, c->stream));
  double eps = c->opts.jitter_eps;
  int info = 0;
  for (int attempt = 0;; ++attempt) {
    B7_TRY(launch_fantasy_factor(c, S, dv, info_dev));
    B7_HIP(c, hipMemcpyAsync(&info, info_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    if (info == 0) break;
    if (attempt > 4000) return b7_fail(c, B7_ERR_INVALID, "gp_fantasize: posterior covariance cannot be factored");
    eps = eps * c->opts.jitter_growth;
    B7_HIP(c, hipMemcpyAsync(S, kpp, sizeof(double) * 4096, hipMemcpyDeviceToDevice, c->stream));
    B7_TRY(launch_add_diag(c, S, 64, P, eps));
  }
  B7_TRY(launch_fantasy_sample(c, S, mu, P, n, seed, out));
  B7_HIP(c, hipMemcpyAsync(Y_out, out, sizeof(double) * (size_t)P * n, hipMemcpyDeviceToHost, c->stream));
  if (mean_out) B7_HIP(c, hipMemcpyAsync(mean_out, mu, sizeof(double) * P, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_gp_append(b7_ctx *c, const double *x_new, const double *y_new) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 0) return b7_fail(c, B7_ERR_STATE, "gp_append: no GP fit on this context");
  if (!x_new || !y_new) return b7_fail(c, B7_ERR_INVALID, "gp_append: NULL argument");
  if (c->N + 1 > c->Npad)
    return b7_fail(c, B7_ERR_STATE, "gp_append: the padded factor is full (N = %d); refit with b7_gp_fit", c->N);
  B7_HIP(c, hipSetDevice(c->device));
  const int N = c->N, np = c->Npad, d = c->dfit, yc = c->ycols;
  c->predicted = false;
  c->gfit = false;  // an extended fit is not b7_gp_fit_hyp's: b7_gp_nll_grad asks for a new one
  post_forget(c);
  // the new observation joins the observation set (raw row, scaled row, half norm, residual row)
  B7_HIP(c, hipMemcpyAsync((double *)c->xobs.p + (size_t)N * d, x_new, sizeof(double) * d, hipMemcpyHostToDevice,
                           c->stream));
  std::vector<double> r(yc);
  for (int k = 0; k < yc; ++k) r[k] = y_new[k] - c->mean;
  B7_HIP(c, hipMemcpyAsync((double *)c->resid.p + (size_t)N * yc, r.data(), sizeof(double) * yc, hipMemcpyHostToDevice,
                           c->stream));
  if (c->have_data)  // the resident data set grows with the fit, so a later b7_gp_fit_hyp sees the new row too
    B7_HIP(c, hipMemcpyAsync((double *)c->ybuf.p + (size_t)N * yc, y_new, sizeof(double) * yc, hipMemcpyHostToDevice,
                             c->stream));
  double *ls_dev = b7_scratch(c)->lenscale;  // of the current fit
  B7_TRY(launch_prep_obs(c, (const double *)c->xobs.p, ls_dev, N + 1, d));
  // k = K(x_new, [X; x_new]) through the covariance kernel (row 0 of a 64-row launch)
  const size_t nslices = ((size_t)np + 255) / 256;  // slice partials of launch_append_vectors: nslices x np
  B7_TRY(b7_ensure(c, c->fant, sizeof(double) * ((size_t)64 * np + 4 * (size_t)np + (size_t)np * nslices + 64)));
  double *krows = (double *)c->fant.p, *lvec = krows + (size_t)64 * np, *uvec = lvec + np, *evec = uvec + np;
  double *part = evec + np;
  int *status_dev = (int *)(part + (size_t)np * nslices);
  B7_TRY(launch_ksx(c, ctx_fit(c), (const double *)c->xobs.p + (size_t)N * d, 0, 64, 1, d, krows, nullptr, 1));
  B7_TRY(launch_append_vectors(c, krows, lvec, uvec, part, evec));
  B7_TRY(launch_append_finalize(c, krows, lvec, uvec, evec, status_dev));
  int status = 0;
  B7_HIP(c, hipMemcpyAsync(&status, status_dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (status != 0) {
    // roll the observation set back; the caller refits from scratch (jitter schedule included)
    B7_TRY(launch_prep_obs(c, (const double *)c->xobs.p, ls_dev, N, d));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    return b7_fail(c, B7_ERR_STATE, "gp_append: the extended matrix is not positive definite; refit with b7_gp_fit");
  }
  c->N = N + 1;
  B7_TRY(launch_alpha(c));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_gp_download(b7_ctx *c, double *L_host, double *alpha_host, double *Linv_host) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted) return b7_fail(c, B7_ERR_STATE, "gp_download: no fit on this context");
  const size_t N = c->N, np = c->Npad;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (L_host)
    B7_HIP(c, hipMemcpy2D(L_host, sizeof(double) * N, c->L.p, sizeof(double) * np, sizeof(double) * N, N,
                          hipMemcpyDeviceToHost));
  if (Linv_host)
    B7_HIP(c, hipMemcpy2D(Linv_host, sizeof(double) * N, c->Linv.p, sizeof(double) * np, sizeof(double) * N, N,
                          hipMemcpyDeviceToHost));
  if (alpha_host)
    B7_HIP(c, hipMemcpy2D(alpha_host, sizeof(double) * c->ycols, c->alpha.p, sizeof(double) * c->yld,
                          sizeof(double) * c->ycols, N, hipMemcpyDeviceToHost));
  return B7_OK;
}

}  // extern "C"
