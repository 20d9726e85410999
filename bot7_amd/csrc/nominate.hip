// bayesopt:eval + nominate as one call, and the separate score / arg-max entry points it replaces.
#include <string.h>

#include <algorithm>

#include "b7_internal.h"

// ---- bayesopt:eval + nominate as one call ------------------------------------------------------------------
// bots/bayesopt.lua:56-99: score = (1/S) sum_s acq(model, hyp_s, X_obs, Y_obs, X_hid), then score:max(1).  The
// separate entry points (b7_gp_predict_hyp, b7_score_*, b7_score_finish*) cost one host round trip per hyper sample
// (the pivot report) plus one for the arg-max; at small N and M (cfg2: 0.2 ms of GPU work per sample) the round trips
// are a third of the wall time.  Here every sample's fit, posterior and score:add are enqueued back to back, each
// fit's 16-byte pivot report is copied into its own pinned slot in stream order, the arg-max follows, and the host
// synchronises ONCE.  Knowing all S samples up front also lets the S fits run SIDE BY SIDE: one persistent launch with
// grid.y = sample (launch_fit_batch), K assembly, residuals and alpha batched the same way; a fit is a dependent chain
// that leaves most of the chip idle, so ten cost little more than one (cfg2, S = 10: 1.55 -> 0.75 ms per nomination).  A report that says "pivot failed" or "hand-off timed out" (rare) throws the accumulated score
// away and redoes the whole nomination through the per-sample path, jitter schedule included, so the result is the
// one the separate calls give.
int stage_fmin(b7_ctx *c, const double *fmin, double **fd_out) {
  if (c->ycols == 1) {  // one response column (every path but the fantasy scores): f_min travels as a kernel argument
    c->fmin_scalar = fmin[0];
    *fd_out = nullptr;
    return B7_OK;
  }
  double *fh = c->pinned->fmin, *fd = b7_scratch(c)->fmin;
  if (!c->fmin_staged || memcmp(fh, fmin, sizeof(double) * c->ycols) != 0) {
    B7_HIP(c, hipStreamSynchronize(c->stream));
    memcpy(fh, fmin, sizeof(double) * c->ycols);
    c->fmin_staged = true;
  }
  B7_HIP(c, hipMemcpyAsync(fd, fh, sizeof(double) * c->ycols, hipMemcpyHostToDevice, c->stream));
  *fd_out = fd;
  return B7_OK;
}

ScoreParams score_params(const b7_ctx *c, const b7_score_spec *spec, const double *fd) {
  ScoreParams p;
  p.kind = spec->kind, p.upper = spec->upper;
  p.fmin = fd, p.fmin0 = c->fmin_scalar;
  p.tradeoff = spec->tradeoff, p.sign = spec->sign;
  return p;
}

// max-value entropy search: the y* search of nS samples into slots [slot0, slot0 + nS) of the layout the caller's mes_begin made,
// enqueued ahead of the score p that reads it
static int mes_search_for(b7_ctx *c, ScoreParams *p, const double *mu, const double *var, int64_t stride, int nS, int slot0) {
  B7_TRY(launch_mes_search(c, mu, var, stride, nS, slot0));
  p->ystar = mes_ystar_dev(c, slot0), p->nlev = c->mes_K;
  return B7_OK;
}

int mes_refuse(b7_ctx *c, const char *who, const b7_score_spec *spec) {
  if (spec->kind != B7_SCORE_MES) return B7_OK;
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: max-value entropy search over a communicator of %d ranks is not built (y* over a sharded grid needs an all-reduce per round)", who, c->comm_world);
  if (c->ycols != 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: max-value entropy search over %d response columns (fantasies) is not built", who, c->ycols);
  return B7_OK;
}

int score_add(b7_ctx *c, const b7_score_spec *sp, const double *fd, bool accumulate) {
  ScoreParams p = score_params(c, sp, fd);
  if (sp->kind == B7_SCORE_MES)  // y* of this sample first, into the slot the caller named (c->mes_slot)
    B7_TRY(mes_search_for(c, &p, (const double *)c->mu.p, (const double *)c->var.p, 0, 1, c->mes_slot));
  return launch_score(c, p, (const double *)c->mu.p, (const double *)c->var.p, c->M, c->ycols, (double *)c->acc.p, accumulate);
}

// The score spec and the global row offset of an eval + nominate entry point (`who` in the messages).  Only a shard of a
// larger candidate set -- a rank of a communicator, a member of a group -- may be empty: the exchange covers the others.
int nominate_args(b7_ctx *c, const char *who, const b7_score_spec *spec, int64_t offset) {
  if (spec->kind != B7_SCORE_EI && spec->kind != B7_SCORE_CB && spec->kind != B7_SCORE_LOGEI && spec->kind != B7_SCORE_MES &&
      spec->kind != B7_SCORE_LOGPI)
    return b7_fail(c, B7_ERR_INVALID, "%s: unknown score kind %d", who, spec->kind);
  if (score_needs_fmin(spec->kind) && !spec->fmin)
    return b7_fail(c, B7_ERR_INVALID, "%s: %s needs fmin", who, spec->kind == B7_SCORE_LOGPI ? "LogPI" : "EI");
  if (offset < 0) return b7_fail(c, B7_ERR_INVALID, "%s: negative row offset", who);
  if (c->M == 0 && !(c->comm && c->comm_world > 1) && !c->group)
    return b7_fail(c, B7_ERR_STATE, "%s: no candidate grid on this context", who);
  return B7_OK;
}

int eval_validate(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, int64_t offset) {
  if (S < 1 || !hyps || !spec) return b7_fail(c, B7_ERR_INVALID, "eval_nominate: S >= 1, hyps and spec required");
  B7_TRY(nominate_args(c, "eval_nominate", spec, offset));
  if (!c->have_data) return b7_fail(c, B7_ERR_STATE, "eval_nominate: call b7_gp_set_data first");
  if (c->M > 0 && c->d != c->dfit)
    return b7_fail(c, B7_ERR_INVALID, "eval_nominate: grid dims %d != data dims %d", c->d, c->dfit);
  for (int s = 0; s < S; ++s) B7_TRY(check_hyp(c, &hyps[s], c->dfit));
  return mes_refuse(c, "eval_nominate", spec);
}

// score:add x S of the batch in c->bmu / c->bvar, owed to the exchange step (exch_local), which runs it fused with score:div,
// the arg-max and the record
int pending_score(b7_ctx *c, int S, const b7_score_spec *spec, const double *fd, ScoreParams *out) {
  ScoreParams p = score_params(c, spec, fd);
  p.S = S, p.mu = (const double *)c->bmu.p, p.var = (const double *)c->bvar.p, p.stride = c->M;
  if (spec->kind == B7_SCORE_MES) B7_TRY(mes_search_for(c, &p, p.mu, p.var, p.stride, S, 0));  // all S samples: grid.y = sample
  *out = p;
  return B7_OK;
}

// ---- eval_enqueue: bots/bayesopt.lua:69-78 as stream work, and its pieces ---------------------------------------------------
// b7_eval_nominate_batch's and b7_eval_nominate_refine's hook (keep, nullable).  A sample fitted in the context's own slot is
// copied to batch slot s; these are sized for that (S == 1: the fit stays where it is)
static int keep_slots_ensure(b7_ctx *c, const BelKeep *keep, int S) {
  if (!keep || S == 1) return B7_OK;
  return batch_slots_ensure(c, S, B7_SLOTS_OPERANDS | B7_SLOTS_LINV | (keep->want_alpha ? B7_SLOTS_ALPHA : 0));
}
// Sample s of S has just been predicted into c->mu / c->var: its mean and variance go to keep's arrays.  in_slot: its fit was
// produced in batch slot s; otherwise it sits in the context's own slot and is copied there (S == 1: it stays, and is kept as that)
static int keep_sample(b7_ctx *c, BelKeep *keep, int S, int s, bool in_slot) {
  if (!keep) return B7_OK;
  const size_t mb = sizeof(double) * (size_t)c->M;
  if (keep->mu) {
    B7_HIP(c, hipMemcpyAsync(keep->mu + (size_t)s * c->M, c->mu.p, mb, hipMemcpyDeviceToDevice, c->stream));
    B7_HIP(c, hipMemcpyAsync(keep->var + (size_t)s * c->M, c->var.p, mb, hipMemcpyDeviceToDevice, c->stream));
  }
  if (S == 1 && !in_slot) {
    keep->fits = ctx_fit(c);
    return B7_OK;
  }
  keep->fits = batch_fits(c, S);
  if (in_slot) return B7_OK;
  const FitSet src = ctx_fit(c), dst = fit_at(keep->fits, s, b7_hyp{nullptr, c->amp, c->noise, c->mean});
  const int n = c->Npad, dp = c->dpad;
  auto put = [&](const double *to, const double *from, int64_t doubles) {  // the batch slots are the context's own memory
    return hipMemcpyAsync(const_cast<double *>(to), from, sizeof(double) * (size_t)doubles, hipMemcpyDeviceToDevice, c->stream);
  };
  if (keep->want_alpha) B7_HIP(c, put(dst.alpha, src.alpha, FitSet::s_alpha(n, dp)));
  B7_HIP(c, put(dst.w, src.w, FitSet::s_w(n, dp)));
  B7_HIP(c, put(dst.zsc, src.zsc, FitSet::s_zsc(n, dp)));
  B7_HIP(c, put(dst.zss, src.zss, FitSet::s_zss(n, dp)));
  B7_HIP(c, put(dst.Linv, src.Linv, FitSet::s_Linv(n, dp)));
  return B7_OK;
}
// ... or all S at once, from the batched posterior's arrays; the fits were produced in the batch slots
static int keep_batch(b7_ctx *c, BelKeep *keep, int S) {
  if (!keep) return B7_OK;
  const size_t bytes = sizeof(double) * (size_t)S * c->M;
  if (keep->mu) {
    B7_HIP(c, hipMemcpyAsync(keep->mu, c->bmu.p, bytes, hipMemcpyDeviceToDevice, c->stream));
    B7_HIP(c, hipMemcpyAsync(keep->var, c->bvar.p, bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  keep->fits = batch_fits(c, S);
  return B7_OK;
}

// The pinned staging block of a nomination: [S][4] pivot reports | the hypers of all S samples, packed ([S][d] lengthscales, then
// S amp, S noise, S mean), as the host addresses it and (the block is mapped) as the device does
struct EvalStage {
  int *reports, *reports_dev;
  double *hyp_host;
  const double *hyp_map;
  size_t hyp_bytes, rep_bytes;
};
// sizes the block and c->bhyp, packs the hypers and marks every report "not written"
static int eval_stage(b7_ctx *c, int S, const b7_hyp *hyps, EvalStage *st) {
  const int d = c->dfit;
  st->hyp_bytes = sizeof(double) * (size_t)S * (d + 3), st->rep_bytes = 16 * (size_t)S;
  B7_TRY(b7_pin_ensure(c, c->pin_eval, st->hyp_bytes + st->rep_bytes, true));
  B7_TRY(b7_ensure(c, c->bhyp, st->hyp_bytes));
  st->reports = static_cast<int *>(c->pin_eval.host), st->reports_dev = static_cast<int *>(c->pin_eval.dev);
  st->hyp_host = reinterpret_cast<double *>(static_cast<char *>(c->pin_eval.host) + st->rep_bytes);
  st->hyp_map = reinterpret_cast<const double *>(static_cast<const char *>(c->pin_eval.dev) + st->rep_bytes);
  const HypPack hp = hyp_pack(st->hyp_host, S, d);
  for (int s = 0; s < S; ++s) {
    memcpy(hp.ls + (size_t)s * d, hyps[s].lenscale_sq, sizeof(double) * d);
    hp.amp[s] = hyps[s].amp;
    hp.noise[s] = hyps[s].noise;
    hp.mean[s] = hyps[s].mean;
  }
  memset(st->reports, 0xff, st->rep_bytes);
  return B7_OK;
}

// The fits of all S samples side by side, produced in the batch slots (batch_fits(c, S) afterwards), the pivot reports on their
// way into the staging block
static int fits_side_by_side(b7_ctx *c, int S, bool small, const EvalStage &st) {
  double *bw = (double *)c->bw.p, *bzsc = (double *)c->bzsc.p, *bzss = (double *)c->bzss.p, *bLinv = (double *)c->bLinv.p;
  double *balpha = (double *)c->balpha.p;
  int *binfo = (int *)c->binfo.p;
  // N <= 128, d <= 32 (the reference's own regime): the whole fit of every hyper sample is one workgroup of ONE launch
  // (gp_small.hip), for any S -- observation scaling, K(X,X), factorisation, inverse, alpha, the pivot reports into the mapped
  // block; the kernel reads the hypers straight from that block and leaves the device copy the kernels downstream read
  if (small)
    return launch_fit_small(c, S, st.hyp_map, st.hyp_host, (double *)c->bhyp.p, bw, bzsc, bzss, nullptr, bLinv, nullptr, balpha, nullptr,
                            binfo, st.reports_dev);
  const int n = c->Npad;
  const int64_t sq = FitSet::s_Linv(n, c->dpad);  // K, L and inv(L) of a fit: Npad x Npad each
  const HypPack hd = hyp_pack(c->bhyp.p, S, c->dfit);
  const double *bK = (const double *)c->bK.p, *bresid = (const double *)c->bresid.p;
  double *bL = (double *)c->bL.p, *bdinv = (double *)c->bdinv.p;
  launch_resid_batch(c, S, hd.mean);
  B7_TRY(launch_kxx_batch(c, S, hd.ls, hd.amp, hd.noise, bw, bzsc, bzss, (double *)c->bK.p));
  // one 64-block per fit: factorisation, inverse, alpha and the pivot report (mirrored into the mapped block) of all S fits in
  // ONE launch of S workgroups
  if (n == 64 && c->potrf_small)
    return launch_potrf_small(c, S, bK, bL, bLinv, bdinv, bresid, balpha, 0.0, binfo, st.reports_dev, sq, sq, (int64_t)n * B7_PANEL,
                              FitSet::s_alpha(n, c->dpad), 4);
  // otherwise one persistent launch with grid.y = sample (one critical workgroup each)
  B7_TRY(launch_fit_batch(c, S, bK, bL, bLinv, bdinv, (unsigned *)c->bflags.p, binfo));
  if (4 * S <= 256)  // the reports ride on the last kernel of the fits into the mapped block: no copy launch
    return launch_alpha_batch(c, S, bLinv, bresid, balpha, binfo, st.reports_dev, 4 * S);
  B7_TRY(launch_alpha_batch(c, S, bLinv, bresid, balpha));
  B7_HIP(c, hipMemcpyAsync(st.reports, binfo, st.rep_bytes, hipMemcpyDeviceToHost, c->stream));
  return B7_OK;
}

// The three posteriors of fits that sit side by side in the batch slots.
// N <= 128, d <= 32: K(X*,X), mean and variance of all S samples in ONE kernel that never stores K* (kpost_small.hip); score:add
// is left to the caller's exchange step in *pend
static int post_side_by_side_small(b7_ctx *c, int S, const b7_score_spec *spec, const double *fd, ScoreParams *pend, BelKeep *keep) {
  B7_TRY(b7_ensure(c, c->bmu, sizeof(double) * (size_t)S * c->M));
  B7_TRY(b7_ensure(c, c->bvar, sizeof(double) * (size_t)S * c->M));
  B7_TRY(launch_kpost_small(c, batch_fits(c, S), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->bmu.p, (double *)c->bvar.p, c->M));
  B7_TRY(keep_batch(c, keep, S));
  B7_TRY(pending_score(c, S, spec, fd, pend));
  c->fitted = false;  // neither the context's fit slot nor its mean / variance vectors hold any of these samples
  c->predicted = false;
  return B7_OK;
}
// K* of all S samples fits the workspace at once (the reference's default sizes: 2e4 candidates, tens to hundreds of
// observations, 10 samples): K*, posterior and score:add of all samples in ONE launch each (grid.z / grid.y = sample), the score
// summed over the samples in order inside the kernel
static int post_side_by_side(b7_ctx *c, int S, const b7_score_spec *spec, const double *fd, BelKeep *keep) {
  const int64_t Mpad = round_up(c->M, B7_MROWS), sks = Mpad * c->Npad;
  const FitSet fits = batch_fits(c, S);
  B7_TRY(b7_ensure(c, c->ks, sizeof(double) * (size_t)sks * S));
  B7_TRY(b7_ensure(c, c->bmu, sizeof(double) * (size_t)S * c->M));
  B7_TRY(b7_ensure(c, c->bvar, sizeof(double) * (size_t)S * c->M));
  B7_TRY(launch_ksx_batch(c, fits, (const double *)c->grid[c->grid_cur].p, Mpad, c->M, (double *)c->ks.p, sks, (double *)c->bmu.p, c->M));
  B7_TRY(launch_post_batch(c, fits, (const double *)c->ks.p, sks, Mpad, c->M, (double *)c->bvar.p, c->M));
  B7_TRY(keep_batch(c, keep, S));
  ScoreParams all;
  B7_TRY(pending_score(c, S, spec, fd, &all));
  B7_TRY(launch_score_batch(c, all, (double *)c->acc.p, c->M));
  c->fitted = false;  // neither the context's fit slot nor its mean / variance vectors hold any of these samples
  c->predicted = false;
  return B7_OK;
}
// K* of one sample at a time: the chunked posterior of batch slot s into c->mu / c->var, then its score:add.  The context's own
// fit slot is not touched and stays declared empty; its scalars are left as the last sample's, c->mu / c->var as that sample's
// prediction (b7_score_* may follow), which is what this route has always left behind
static int post_in_turn(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, const double *fd, BelKeep *keep) {
  const FitSet fits = batch_fits(c, S);
  c->model_kind = 0;
  int rc = B7_OK;
  for (int s = 0; s < S && rc == B7_OK; ++s) {
    c->amp = hyps[s].amp, c->noise = hyps[s].noise, c->mean = hyps[s].mean;
    rc = predict_into(c, fit_at(fits, s, hyps[s]), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->mu.p, (double *)c->var.p);
    c->mes_slot = s;
    if (rc == B7_OK) rc = score_add(c, spec, fd);
    if (rc == B7_OK) rc = keep_sample(c, keep, S, s, true);
  }
  c->fitted = false;
  c->predicted = true;
  c->Mpred = c->M;
  return rc;
}

// The fits one after the other in the context's own slot (several response columns, a size or a schedule the side-by-side fits
// do not serve), each followed by its posterior and its score:add
static int fits_in_turn(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, const double *fd, BelKeep *keep) {
  B7_TRY(keep_slots_ensure(c, keep, S));
  for (int s = 0; s < S; ++s) {
    B7_TRY(fit_front(c, &hyps[s], (const double *)c->bhyp.p + (size_t)s * c->dfit));
    int *report = static_cast<int *>(c->pin_eval.dev) + 4 * s;  // a one-block factorisation mirrors its report itself
    FactorNote note;
    B7_TRY(launch_potrf(c, 0.0, true, report, &note));
    if (!c->linv_done) B7_TRY(launch_trtri(c));  // on a failed factor this inverts rubbish; the report discards it
    B7_TRY(launch_alpha(c, report, 4, note));  // + this fit's pivot report, no copy launch
    c->fitted = true;
    B7_TRY(predict_into(c, ctx_fit(c), (const double *)c->grid[c->grid_cur].p, c->M, (double *)c->mu.p, (double *)c->var.p));
    c->predicted = true;
    c->Mpred = c->M;
    c->mes_slot = s;
    B7_TRY(score_add(c, spec, fd));
    B7_TRY(keep_sample(c, keep, S, s, false));
  }
  // this fit's lengthscales sit in the batch staging block, not in ScratchBlock::lenscale: the fit slot is declared empty
  c->fitted = false;
  return B7_OK;
}

// Zero the accumulator, then fit + posterior + score:add per hyper sample, each fit's pivot report on its way to its pinned slot
// in stream order.  Returns without waiting for any of it; the small regime's score:add is left to the caller's exchange step in
// *pend.  Everything is sized before anything is in flight: a reallocation between launches would synchronise.
int eval_enqueue(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, ScoreParams *pend, BelKeep *keep) {
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)c->M * c->ycols));
  B7_TRY(b7_ensure(c, c->var, sizeof(double) * (size_t)c->M));
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)c->M));
  B7_TRY(b7_ensure(c, c->ks, sizeof(double) * (size_t)predict_chunk(c, c->M) * c->Npad));  // predict_into's workspace
  if (spec->kind == B7_SCORE_MES) B7_TRY(mes_begin(c, S, c->M, c->mes_levels));  // y*[S][K], brackets and partials
  EvalStage st;
  B7_TRY(eval_stage(c, S, hyps, &st));
  // side by side: the one-launch small fit for any S, or S > 1 single-column fits in one persistent launch when that schedule
  // serves this size
  const bool small = fit_small_applies(c);
  const bool batch = small || (S > 1 && c->ycols == 1 && c->potrf_sched == 3 && c->Npad <= B7_PERSIST_NMAX && c->inverse_inline);
  if (batch) {
    B7_TRY(batch_slots_ensure(c, S, B7_SLOTS_OPERANDS | B7_SLOTS_LINV | B7_SLOTS_ALPHA | (small ? 0 : B7_SLOTS_FACTOR)));
    B7_TRY(b7_ensure(c, c->binfo, sizeof(int) * 4 * (size_t)S));
    if (!small) B7_TRY(b7_ensure(c, c->bflags, sizeof(unsigned) * S * persist_flag_words_host(c->Npad / B7_PANEL)));
  }
  if (!small) B7_HIP(c, hipMemcpyAsync(c->bhyp.p, st.hyp_host, st.hyp_bytes, hipMemcpyHostToDevice, c->stream));
  double *fd = nullptr;
  if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
  acc_declare_zeros(c, spec->kind);
  if (!batch) return fits_in_turn(c, S, hyps, spec, fd, keep);
  B7_TRY(fits_side_by_side(c, S, small, st));
  if (c->kpost_small && kpost_small_applies(c)) return post_side_by_side_small(c, S, spec, fd, pend, keep);
  if ((size_t)round_up(c->M, B7_MROWS) * S * sizeof(double) * (size_t)c->Npad <= c->ks_bytes) return post_side_by_side(c, S, spec, fd, keep);
  return post_in_turn(c, S, hyps, spec, fd, keep);
}

// after the stream has drained: did each of S fits ([S][4] report words) factor at the first attempt, without a hand-off
// time-out?  persist: the fits may have run the persistent schedule, which a time-out switches off (persist_gave_up)
bool reports_clean(b7_ctx *c, const int *reports, int S, bool persist) {
  bool clean = true, aborted = false;
  for (int s = 0; s < S; ++s) {
    clean = clean && reports[4 * s] == 0 && reports[4 * s + 1] == 0;
    aborted = aborted || reports[4 * s + 1] != 0;
  }
  if (aborted && persist) persist_gave_up(c);
  return clean;
}

// the same nomination through the per-sample path, jitter schedule (utils/math.lua:159-218) included; synchronous
int eval_redo(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, double *jitter_out, int *info_out, BelKeep *keep) {
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(keep_slots_ensure(c, keep, S));
  B7_TRY(acc_write_zeros(c));
  if (spec->kind == B7_SCORE_MES) B7_TRY(mes_begin(c, S, c->M, c->mes_levels));
  double *fd = nullptr;
  for (int s = 0; s < S; ++s) {
    B7_TRY(fit_hyp_core(c, &hyps[s], nullptr, jitter_out ? jitter_out + s : nullptr, info_out ? info_out + s : nullptr, true));
    c->predicted = true;
    c->Mpred = c->M;
    if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
    c->mes_slot = s;
    B7_TRY(score_add(c, spec, fd));
    B7_TRY(keep_sample(c, keep, S, s, false));
  }
  return B7_OK;
}

static int score_ready(b7_ctx *c, const char *who) {
  if (!c->predicted || c->Mpred != c->M) return b7_fail(c, B7_ERR_STATE, "%s: call b7_gp_predict first", who);
  if (!c->acc_valid) return b7_fail(c, B7_ERR_STATE, "%s: call b7_score_reset first", who);
  return B7_OK;
}

static int upload_mv(b7_ctx *c, const double *mean, const double *var, int64_t M, int cc) {
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (size_t)M * cc));
  B7_TRY(b7_ensure(c, c->tmpvar, sizeof(double) * (size_t)M));
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)M));
  B7_HIP(c, hipMemcpyAsync(c->tmpmu.p, mean, sizeof(double) * (size_t)M * cc, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(c->tmpvar.p, var, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  return B7_OK;
}

// EI.compute / conf_bound.compute on the caller's host vectors (arguments checked by the entry point): upload, the cc values of
// spec.fmin (if the score takes one) to the device, the score, download, wait
static int score_compute(b7_ctx *c, const b7_score_spec &spec, const double *mean, const double *var, int64_t M, int cc, double *out) {
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(upload_mv(c, mean, var, M, cc));
  double *fd = nullptr;
  if (score_needs_fmin(spec.kind)) {
    fd = b7_scratch(c)->fmin;
    B7_HIP(c, hipMemcpyAsync(fd, spec.fmin, sizeof(double) * cc, hipMemcpyHostToDevice, c->stream));
  }
  B7_TRY(launch_score(c, score_params(c, &spec, fd), (const double *)c->tmpmu.p, (const double *)c->tmpvar.p, M, cc,
                      (double *)c->tmpgrid.p, false));
  B7_HIP(c, hipMemcpyAsync(out, c->tmpgrid.p, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

extern "C" {

int b7_eval_nominate(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, int64_t global_row_offset,
                     double *best_val, int64_t *best_idx1, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "eval_nominate: this context belongs to a group (b7_group_eval_nominate)");
  if (jitter_out && S > 0) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out && S > 0) std::fill(info_out, info_out + S, 0);
  // a property of the spec and the communicator, the same on every rank: refused before anything is enqueued and WITHOUT a
  // collective (every rank returns here, nobody is left inside one)
  if (spec && spec->kind == B7_SCORE_MES && c->comm && c->comm_world > 1) return mes_refuse(c, "eval_nominate", spec);
  return nominate_run(
      c, "eval_nominate", eval_validate(c, S, hyps, spec, global_row_offset), global_row_offset, (double)S,
      [&](ScoreParams *pend) { return eval_enqueue(c, S, hyps, spec, pend); },
      [&]() { return reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true); },
      [&]() { return eval_redo(c, S, hyps, spec, jitter_out, info_out); }, best_val, best_idx1);
}

// b7_eval_nominate with global_row_offset = 0 and the feasibility column weighted in between score:div and score:max(1)
// (score.hip's header): the same routes, the same single host wait, the same jitter redo; L is read, not modified.
int b7_eval_nominate_feasible(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, double *best_val, int64_t *best_idx1,
                              double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "eval_nominate_feasible: this context belongs to a group (constrained nomination over a sharded grid is not built)");
  if (jitter_out && S > 0) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out && S > 0) std::fill(info_out, info_out + S, 0);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_feasible: a communicator of %d ranks (constrained nomination over a sharded grid is not built)", c->comm_world);
  if (spec && spec->kind == B7_SCORE_CB)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_feasible: a confidence bound is a signed score and has no product form with a feasibility weight (EI, LogEI and LogPI are built)");
  if (spec && spec->kind == B7_SCORE_MES)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_feasible: max-value entropy search is not built with a feasibility weight (EI, LogEI and LogPI are built)");
  B7_TRY(eval_validate(c, S, hyps, spec, 0));
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_feasible: %d response columns (one is built)", c->ycols);
  if (!c->feas_valid)
    return b7_fail(c, B7_ERR_STATE, "eval_nominate_feasible: no feasibility column on this grid (call b7_feas_reset; a grid change forgets it)");
  return nominate_run(
      c, "eval_nominate_feasible", B7_OK, 0, (double)S, [&](ScoreParams *pend) { return eval_enqueue(c, S, hyps, spec, pend); },
      [&]() { return reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true); },
      [&]() { return eval_redo(c, S, hyps, spec, jitter_out, info_out); }, best_val, best_idx1, (const double *)c->feas.p);
}

// ---- the feasibility column (score.hip's header) -----------------------------------------------------------
static int feas_guard(b7_ctx *c, const char *who, bool need_column) {
  if (c->group) return b7_fail(c, B7_ERR_STATE, "%s: this context belongs to a group (a feasibility column over a sharded grid is not built)", who);
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "%s: no candidate grid", who);
  if (need_column && !c->feas_valid)
    return b7_fail(c, B7_ERR_STATE, "%s: no feasibility column on this grid (call b7_feas_reset; a grid change forgets it)", who);
  B7_HIP(c, hipSetDevice(c->device));
  return B7_OK;
}

int b7_feas_reset(b7_ctx *c) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(feas_guard(c, "feas_reset", false));
  return feas_write_zeros(c);
}

int b7_feas_add(b7_ctx *c, const double *logw, int64_t M) {
  if (!c) return B7_ERR_INVALID;
  if (!logw) return b7_fail(c, B7_ERR_INVALID, "feas_add: logw is NULL");
  B7_TRY(feas_guard(c, "feas_add", true));
  if (M != c->M) return b7_fail(c, B7_ERR_INVALID, "feas_add: %lld log-weights for a grid of %lld rows", (long long)M, (long long)c->M);
  B7_TRY(b7_ensure(c, c->feas_stage, sizeof(double) * (size_t)M));
  B7_HIP(c, hipMemcpyAsync(c->feas_stage.p, logw, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_feas_add(c, (const double *)c->feas_stage.p));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's vector need not outlive the call
  return B7_OK;
}

// L += src's accumulator, device to device.  The two streams are ordered by events both ways (streams_order): the add waits for what
// src's stream has been given (b7_eval_nominate may return before its stream is formally idle), and whatever src enqueues next waits for the add.
int b7_feas_add_acc(b7_ctx *c, b7_ctx *src) {
  if (!c) return B7_ERR_INVALID;
  if (!src) return b7_fail(c, B7_ERR_INVALID, "feas_add_acc: the source context is NULL");
  B7_TRY(feas_guard(c, "feas_add_acc", true));
  if (src->device != c->device)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "feas_add_acc: the source context is on device %d, this one on device %d (a copy across devices is not built)", src->device, c->device);
  if (!src->acc_valid) return b7_fail(c, B7_ERR_STATE, "feas_add_acc: the source context holds no accumulator (its grid changed, or nothing was scored)");
  if (src->acc_kind != B7_ACC_LOG)
    return b7_fail(c, B7_ERR_STATE, "feas_add_acc: the source's accumulator is a linear sum, not a log one (LogPI or LogEI leaves a log accumulator)");
  if (src->acc_fresh) return b7_fail(c, B7_ERR_STATE, "feas_add_acc: the source's log accumulator is declared but nothing has been added onto it");
  if (src->M != c->M)
    return b7_fail(c, B7_ERR_INVALID, "feas_add_acc: the source's grid has %lld rows, this one %lld", (long long)src->M, (long long)c->M);
  b7_ctx *const o[2] = {c, src};  // (src == c orders nothing)
  B7_TRY(streams_order(o, 2, true));
  B7_TRY(launch_feas_add(c, (const double *)src->acc.p));
  return streams_order(o, 2, false);
}

int b7_feas_get(b7_ctx *c, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (!out) return b7_fail(c, B7_ERR_INVALID, "feas_get: out is NULL");
  B7_TRY(feas_guard(c, "feas_get", true));
  B7_HIP(c, hipMemcpyAsync(out, c->feas.p, sizeof(double) * (size_t)c->M, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_feas_nominate(b7_ctx *c, double *best_val, int64_t *best_idx1) {
  if (!c) return B7_ERR_INVALID;
  B7_TRY(feas_guard(c, "feas_nominate", true));
  return launch_feas_best(c, best_val, best_idx1);
}

// ---- scores --------------------------------------------------------------------------------------------
int b7_score_reset(b7_ctx *c) {
  if (!c) return B7_ERR_INVALID;
  if (c->M <= 0) return b7_fail(c, B7_ERR_STATE, "score_reset: no candidate grid");
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)c->M));
  return acc_write_zeros(c);  // torch.zeros(X_hid:size(1)), bots/bayesopt.lua:69
}

// one score of the last predict added onto the accumulator; who: the entry point in the messages
static int score_entry(b7_ctx *c, const char *who, const b7_score_spec &spec) {
  if (!c) return B7_ERR_INVALID;
  if (score_needs_fmin(spec.kind) && !spec.fmin) return b7_fail(c, B7_ERR_INVALID, "%s: fmin is NULL", who);
  B7_TRY(score_ready(c, who));
  B7_HIP(c, hipSetDevice(c->device));
  // fmin goes pageable -> pinned staging (PinnedBlock::fmin) -> device: the caller's array need not
  // outlive this call and the copy is a true asynchronous one.  The staging slot may still be the source of an
  // earlier copy in flight, hence the wait when the values change (once per nomination: fmin is the same for every
  // hyper sample of a marginalisation loop).
  double *fd = nullptr;
  if (score_needs_fmin(spec.kind)) B7_TRY(stage_fmin(c, spec.fmin, &fd));
  return score_add(c, &spec, fd);
}

int b7_score_ei(b7_ctx *c, const double *fmin, double tradeoff) {
  return score_entry(c, "score_ei", b7_score_spec{B7_SCORE_EI, tradeoff, 0, 0.0, fmin});
}

// log-space EI of the last predict, folded into the accumulator as a running log-sum-exp (score.hip's header)
int b7_score_logei(b7_ctx *c, const double *fmin, double tradeoff) {
  return score_entry(c, "score_logei", b7_score_spec{B7_SCORE_LOGEI, tradeoff, 0, 0.0, fmin});
}

// log probability of improvement of the last predict, folded into the accumulator as a running log-sum-exp (score.hip's header)
int b7_score_logpi(b7_ctx *c, const double *fmin, double tradeoff) {
  return score_entry(c, "score_logpi", b7_score_spec{B7_SCORE_LOGPI, tradeoff, 0, 0.0, fmin});
}

// max-value entropy search of the last predict: the y* search (K = b7_mes_set_levels' value), then score:add (score.hip's header)
int b7_score_mes(b7_ctx *c) {
  if (!c) return B7_ERR_INVALID;
  const b7_score_spec spec{B7_SCORE_MES, 0.0, 0, 0.0, nullptr};
  B7_TRY(score_ready(c, "score_mes"));
  B7_TRY(mes_refuse(c, "score_mes", &spec));
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(mes_begin(c, 1, c->M, c->mes_levels));
  c->mes_slot = 0;
  return score_add(c, &spec, nullptr);
}

int b7_score_cb(b7_ctx *c, double tradeoff, int upper, double sign) {
  return score_entry(c, "score_cb", b7_score_spec{B7_SCORE_CB, tradeoff, upper, sign, nullptr});
}

int b7_score_finish(b7_ctx *c, double divisor, double *best_val, int64_t *best_idx1, double *scores_host) {
  if (!c) return B7_ERR_INVALID;
  if (!c->acc_valid) return b7_fail(c, B7_ERR_STATE, "score_finish: call b7_score_reset first");
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(acc_materialize(c));
  B7_TRY(launch_finish(c, (double *)c->acc.p, c->M, divisor, best_val, best_idx1, c->acc_kind == B7_ACC_LOG));
  if (scores_host) {
    B7_HIP(c, hipMemcpyAsync(scores_host, c->acc.p, sizeof(double) * (size_t)c->M, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
  }
  return B7_OK;
}

int b7_ei_compute(b7_ctx *c, const double *mean, const double *var, const double *fmin, double tradeoff, int64_t M,
                  int cc, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || cc < 1 || cc > 256 || (M > 0 && (!mean || !var || !fmin || !out)))
    return b7_fail(c, B7_ERR_INVALID, "ei_compute: bad arguments");
  return score_compute(c, b7_score_spec{B7_SCORE_EI, tradeoff, 0, 0.0, fmin}, mean, var, M, cc, out);
}

int b7_logei_compute(b7_ctx *c, const double *mean, const double *var, const double *fmin, double tradeoff, int64_t M,
                     int cc, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || cc < 1 || cc > 256 || (M > 0 && (!mean || !var || !fmin || !out)))
    return b7_fail(c, B7_ERR_INVALID, "logei_compute: bad arguments");
  return score_compute(c, b7_score_spec{B7_SCORE_LOGEI, tradeoff, 0, 0.0, fmin}, mean, var, M, cc, out);
}

int b7_logpi_compute(b7_ctx *c, const double *mean, const double *var, const double *fmin, double tradeoff, int64_t M,
                     int cc, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || cc < 1 || cc > 256 || (M > 0 && (!mean || !var || !fmin || !out)))
    return b7_fail(c, B7_ERR_INVALID, "logpi_compute: bad arguments");
  return score_compute(c, b7_score_spec{B7_SCORE_LOGPI, tradeoff, 0, 0.0, fmin}, mean, var, M, cc, out);
}

int b7_cb_compute(b7_ctx *c, const double *mean, const double *var, double tradeoff, int upper, double sign, int64_t M,
                  int cc, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || cc < 1 || (M > 0 && (!mean || !var || !out))) return b7_fail(c, B7_ERR_INVALID, "cb_compute: bad arguments");
  return score_compute(c, b7_score_spec{B7_SCORE_CB, tradeoff, upper, sign, nullptr}, mean, var, M, cc, out);
}

int b7_argmax(b7_ctx *c, const double *scores, int64_t M, double *best_val, int64_t *best_idx1) {
  if (!c) return B7_ERR_INVALID;
  if (M < 1 || !scores) return b7_fail(c, B7_ERR_INVALID, "argmax: empty input");
  B7_HIP(c, hipSetDevice(c->device));
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)M));
  B7_HIP(c, hipMemcpyAsync(c->tmpgrid.p, scores, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  return launch_finish(c, (double *)c->tmpgrid.p, M, 1.0, best_val, best_idx1);
}

}  // extern "C"
