// DNGO: basis features + Bayesian linear head (models/dngo.lua), as separate entry points and as one nomination call.
#include <math.h>
#include <string.h>

#include "b7_internal.h"

// ---- DNGO: basis features + Bayesian linear head --------------------------------------------------------------
int blr_upload_net(b7_ctx *c, const b7_mlp *net, int *z_out) {
  if (!net || !net->dims || !net->W || !net->b || net->n_layers < 1 || net->n_layers > 4)
    return b7_fail(c, B7_ERR_INVALID, "mlp: 1..4 layers with dims, W and b required");
  size_t total = 0;
  for (int l = 0; l < net->n_layers; ++l) total += (size_t)net->dims[l + 1] * net->dims[l] + net->dims[l + 1];
  std::vector<double> pack(total);
  size_t off = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    const size_t nw = (size_t)net->dims[l + 1] * net->dims[l];
    memcpy(&pack[off], net->W[l], nw * sizeof(double));
    off += nw;
    memcpy(&pack[off], net->b[l], (size_t)net->dims[l + 1] * sizeof(double));
    off += net->dims[l + 1];
  }
  *z_out = net->dims[net->n_layers];
  // the same network as last time (models/dngo.lua:155-171 runs it over X_obs and then over the candidates): already there
  if (c->net_host.size() == total && c->netbuf.cap >= total * sizeof(double) &&
      memcmp(c->net_host.data(), pack.data(), total * sizeof(double)) == 0)
    return B7_OK;
  B7_TRY(b7_ensure(c, c->netbuf, total * sizeof(double)));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // nobody is reading the old weights any more
  B7_HIP(c, hipMemcpy(c->netbuf.p, pack.data(), total * sizeof(double), hipMemcpyHostToDevice));
  c->net_host.swap(pack);
  return B7_OK;
}

// The feature matrix: round_up(M, 256) rows x zpad columns, of which the basis kernels write the first z of the first M
// rows.  Everything else must be zero (the variance GEMM reads whole padded rows) and is zeroed when the buffer is
// (re)allocated or its column layout changes -- not on every call: a 67 MB memset per nomination was a sixth of a cfg5 step.
int blr_feat_alloc(b7_ctx *c, int64_t M, int z) {
  const int zpad = npad_of(c, z);
  const size_t bytes = sizeof(double) * (size_t)round_up(M, B7_MROWS) * zpad;
  const bool grown = c->feat.cap < bytes;
  B7_TRY(b7_ensure(c, c->feat, bytes));
  if (grown || c->feat_z != z || c->feat_zeroed_bytes < bytes) {
    B7_HIP(c, hipMemsetAsync(c->feat.p, 0, c->feat.cap, c->stream));
    c->feat_zeroed_bytes = c->feat.cap;
    c->feat_z = z;
  }
  c->Mfeat = M;
  c->zdim = z;
  c->predicted = false;
  return B7_OK;
}

// A head of z features becomes the context's (not yet fitted) model: the fit state, and the buffers sized.  general: those of
// the general factorisation and of nk observations too (the marginalised heads live in the batch buffers and need only the report's)
static int blr_head_setup(b7_ctx *c, int z, int nk, double mean, double noise, bool general = true) {
  const size_t np = (size_t)npad_of(c, z), nn = np * np * sizeof(double);
  if (general) {
    for (DevBuf *b : {&c->K, &c->L, &c->Linv, &c->W}) B7_TRY(b7_ensure(c, *b, nn));
    B7_TRY(b7_ensure(c, c->dinv, sizeof(double) * (np + B7_PANEL) * B7_PANEL));
    B7_TRY(b7_ensure(c, c->alpha, sizeof(double) * np));
    B7_TRY(b7_ensure(c, c->resid, sizeof(double) * np));
    B7_TRY(b7_ensure(c, c->tmpvar, sizeof(double) * (size_t)nk));
  }
  B7_TRY(b7_ensure(c, c->info, B7_INFO_BYTES));
  c->have_data = false, c->fitted = false, c->predicted = false;
  post_forget(c);
  c->N = z, c->Npad = (int)np, c->ycols = 1, c->yld = 1, c->model_kind = 1;
  c->mean = mean, c->noise = noise, c->amp = 0.0;
  return B7_OK;
}

// mean and variance of the context's head over the M rows of resident features, enqueued; mean_done: c->mu holds the mean already
static int blr_predict_enqueue(b7_ctx *c, int64_t M, bool mean_done = false) {
  B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)M));
  B7_TRY(b7_ensure(c, c->var, sizeof(double) * (size_t)M));
  if (!mean_done)
    B7_TRY(launch_gemv_rows(c, (const double *)c->feat.p, c->Npad, (const double *)c->alpha.p, c->Npad, c->mean, 0, M, M,
                            (double *)c->mu.p));
  B7_TRY(launch_post(c, ctx_fit(c), (const double *)c->feat.p, 0, round_up(M, B7_MROWS), M, (double *)c->var.p));
  c->predicted = true;
  c->Mpred = M;
  return B7_OK;
}

// Shared tail of the two fit entry points: c->tmpgrid holds Z0' (zpad x nk, zero padded) on the device.
static int blr_fit_core(b7_ctx *c, const double *Y0, int N, int z, double alpha_prec, double beta, double mean,
                        double *nll_out) {
  const int zpad = npad_of(c, z), nk = (int)round_up(N, 16);
  const size_t np = (size_t)zpad;
  B7_TRY(blr_head_setup(c, z, nk, mean, 1.0 / beta));
  std::vector<double> rb((size_t)nk, 0.0);
  for (int i = 0; i < N; ++i) rb[i] = beta * (Y0[i] - mean);
  B7_HIP(c, hipMemcpyAsync(c->tmpvar.p, rb.data(), sizeof(double) * nk, hipMemcpyHostToDevice, c->stream));
  // G = Z0'Z0 (MFMA), K = beta G + alpha I, q = Z0' beta r
  B7_TRY(launch_gemm_nt(c, (const double *)c->tmpgrid.p, nk, (const double *)c->tmpgrid.p, nk, (double *)c->W.p, zpad,
                        zpad, zpad, nk));
  B7_TRY(launch_blr_assemble(c, (const double *)c->W.p, (double *)c->K.p, z, zpad, alpha_prec, beta));
  B7_TRY(launch_gemv_rows(c, (const double *)c->tmpgrid.p, nk, (const double *)c->tmpvar.p, nk, 0.0, 0, zpad, zpad,
                          (double *)c->resid.p));
  int info_first = 0;
  double jitter = 0.0;
  FactorNote note;
  B7_TRY(chol_with_jitter(c, &jitter, &info_first, true, &note));
  B7_TRY(launch_trtri(c));
  B7_TRY(launch_alpha(c, nullptr, 0, note));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (nll_out) {
    // -log p(y | alpha, beta) = -[ z/2 log alpha + N/2 log beta - E(m) - 1/2 log|K| - N/2 log 2 pi ],
    // E(m) = beta/2 |r|^2 - 1/2 (beta q)' m     (Bishop 3.82 / 3.86)
    std::vector<double> diag(z), m(z), bq(z);
    B7_HIP(c, hipMemcpy2D(diag.data(), sizeof(double), c->L.p, sizeof(double) * (np + 1), sizeof(double), z,
                          hipMemcpyDeviceToHost));
    B7_HIP(c, hipMemcpy(m.data(), c->alpha.p, sizeof(double) * z, hipMemcpyDeviceToHost));
    B7_HIP(c, hipMemcpy(bq.data(), c->resid.p, sizeof(double) * z, hipMemcpyDeviceToHost));
    double logdet = 0.0, rr = 0.0, qm = 0.0;
    for (int k = 0; k < z; ++k) {
      logdet += 2.0 * log(diag[k]);
      qm += bq[k] * m[k];
    }
    for (int i = 0; i < N; ++i) rr += (Y0[i] - mean) * (Y0[i] - mean);
    const double Em = 0.5 * beta * rr - 0.5 * qm;
    *nll_out = -(0.5 * z * log(alpha_prec) + 0.5 * N * log(beta) - Em - 0.5 * logdet - 0.5 * N * log(2.0 * M_PI));
  }
  c->fitted = true;
  return B7_OK;
}

// ---- models/dngo.lua:155-175 + bots/bayesopt.lua:65-66 + :96 as ONE call ----------------------------------------------
// The DNGO branch of bayesopt:eval scores once (no hyper marginalisation): features of the observations, the Bayesian
// linear head, features of every candidate, predictive mean / variance, the acquisition, score:max(1).  Through the
// separate entry points that is six calls and four host synchronisations around 0.2 ms of GPU work; here everything is
// enqueued back to back (the head's Cholesky reports its pivot status into pinned memory in stream order), the arg-max
// record follows, and the host waits once.  A failed pivot (rare: K = beta Z'Z + alpha I is positive definite by
// construction) redoes the fit through b7_blr_fit_x's jitter schedule and scores again.
static int blr_enqueue_fit(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int z, double alpha_prec,
                           double beta, double mean) {
  const int d = net->dims[0], zpad = npad_of(c, z), nk = (int)round_up(N, 16);
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)zpad * nk));
  B7_TRY(blr_head_setup(c, z, nk, mean, 1.0 / beta));
  // the observations and beta (y - mean) go up in ONE copy from pinned staging, laid out [X0 | beta (y - mean) | features]:
  // the caller's arrays are pageable, and an "asynchronous" copy from pageable memory makes the host wait for the stream to
  // reach it -- two of them per nomination serialised the host's enqueueing with the GPU's work
  const size_t up_doubles = (size_t)N * d + (size_t)nk;
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (up_doubles + (size_t)N * z)));
  B7_TRY(b7_pin_ensure(c, c->pin_blr, sizeof(double) * up_doubles, false));
  double *stage = static_cast<double *>(c->pin_blr.host);
  memcpy(stage, X0, sizeof(double) * (size_t)N * d);
  for (int i = 0; i < nk; ++i) stage[(size_t)N * d + i] = i < N ? beta * (Y0[i] - mean) : 0.0;
  double *xdev = (double *)c->tmpmu.p, *yvdev = xdev + (size_t)N * d, *zdev = yvdev + nk;
  B7_HIP(c, hipMemcpyAsync(xdev, stage, sizeof(double) * up_doubles, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_mlp_forward(c, xdev, N, d, (const double *)c->netbuf.p, net->dims, net->n_layers, net->activation, zdev, z));
  if (zpad == 64 && c->blr_small) {
    // z <= 64 features: Z'Z, the assembly, b, the factorisation, its inverse and the head's weights in ONE workgroup of ONE
    // launch (blr_small.hip) instead of nine dispatches; a failed pivot is reported and redone through b7_blr_fit_x
    B7_TRY(launch_blr_head_small(c, zdev, N, z, z, yvdev, alpha_prec, beta, nullptr));
    B7_HIP(c, hipMemcpyAsync(c->pinned->fit.info, c->info.p, 16, hipMemcpyDeviceToHost, c->stream));
    c->fitted = true;
    return B7_OK;
  }
  B7_TRY(launch_transpose_pad(c, zdev, N, z, z, (double *)c->tmpgrid.p, zpad, nk));
  B7_TRY(launch_gemm_nt(c, (const double *)c->tmpgrid.p, nk, (const double *)c->tmpgrid.p, nk, (double *)c->W.p, zpad, zpad,
                        zpad, nk));
  B7_TRY(launch_blr_assemble(c, (const double *)c->W.p, (double *)c->K.p, z, zpad, alpha_prec, beta));
  B7_TRY(launch_gemv_rows(c, (const double *)c->tmpgrid.p, nk, (const double *)yvdev, nk, 0.0, 0, zpad, zpad,
                          (double *)c->resid.p));
  FactorNote note;
  B7_TRY(launch_potrf(c, 0.0, true, nullptr, &note));
  if (!c->linv_done) B7_TRY(launch_trtri(c));  // on a failed factor this inverts rubbish; the report discards it
  B7_TRY(launch_alpha(c, nullptr, 0, note));
  // the pivot report of the plain attempt, into the pinned fit-report block in stream order
  B7_HIP(c, hipMemcpyAsync(c->pinned->fit.info, c->info.p, 16, hipMemcpyDeviceToHost, c->stream));
  c->fitted = true;
  return B7_OK;
}

// features of the resident grid (recomputed, as models/dngo.lua:155-171 does on every predict), mean, variance, score.
// fused_mean: the basis kernel forms the mean on its way (four fma chains per row); otherwise launch_gemv_rows does, in
// b7_blr_predict's order of summation -- the failed-pivot redo asks for that, so that it IS b7_blr_fit_x + b7_blr_basis +
// b7_blr_predict + the score, bit for bit (tests/test_gpu_blr.py holds it to that).
static int blr_enqueue_score(b7_ctx *c, const b7_mlp *net, int z, const b7_score_spec *spec, bool fused_mean = true) {
  const int zpad = npad_of(c, z);
  B7_TRY(blr_feat_alloc(c, c->M, z));
  B7_TRY(b7_ensure(c, c->mu, sizeof(double) * (size_t)c->M));
  B7_TRY(b7_ensure(c, c->var, sizeof(double) * (size_t)c->M));
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)c->M));
  bool mean_done = false;
  B7_TRY(launch_mlp_forward_mean(c, (const double *)c->grid[c->grid_cur].p, c->M, c->d, (const double *)c->netbuf.p, net->dims,
                                 net->n_layers, net->activation, (double *)c->feat.p, zpad,
                                 fused_mean ? (const double *)c->alpha.p : nullptr, c->mean, (double *)c->mu.p, &mean_done));
  B7_TRY(blr_predict_enqueue(c, c->M, mean_done));
  // bots/bayesopt.lua:65-66: the score of the one model, no accumulation over samples -> written, not added (which makes the
  // accumulator valid: score.hip, acc_mode)
  double *fd = nullptr;
  if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
  return score_add(c, spec, fd, false);
}

// ---- the same with the head's hypers marginalised (models/dngo.lua:109,174) -------------------------------------------------
// S heads over the same features.  z <= 64 features (the usual DNGO head): everything is enqueued without a host wait -- features
// of the observations, the S heads as S workgroups of ONE launch (blr_small.hip), features of the candidates, the S means (one
// batched matrix-vector launch), the S variances (one launch of the posterior kernel over the shared features), and score:add x S +
// div + arg-max + record fused in one launch.  Wider heads, or a failed pivot: head by head through b7_blr_fit_x.
static int blr_marg_slow(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap,
                         const double *bt, const double *mn, int z, const b7_score_spec *spec, double *nll_out) {
  const int zpad = npad_of(c, z);
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)c->M));
  B7_TRY(acc_write_zeros(c));
  for (int s = 0; s < S; ++s) {
    B7_TRY(b7_blr_fit_x(c, net, X0, Y0, N, ap[s], bt[s], mn[s], nll_out ? nll_out + s : nullptr));   // synchronous, jitter schedule included
    if (s == 0) {
      B7_TRY(blr_feat_alloc(c, c->M, z));
      B7_TRY(launch_mlp_forward(c, (const double *)c->grid[c->grid_cur].p, c->M, c->d, (const double *)c->netbuf.p, net->dims,
                                net->n_layers, net->activation, (double *)c->feat.p, zpad));
    }
    c->Mfeat = c->M;
    B7_TRY(blr_predict_enqueue(c, c->M));
    double *fd = nullptr;
    if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
    B7_TRY(score_add(c, spec, fd));
  }
  return B7_OK;
}

// The front of that route, which b7_blr_ts_nominate (blr_ts.hip) shares: the observations' features and the S heads, enqueued.  Leaves
// L^-1 in c->bLinv ([S][64 x 64]), the weights in c->balpha ([S][64]), the pivot reports ([S][4] ints) and, when asked for, the
// evidence's terms ([S][3] doubles behind them) on their way into c->pin_eval, and in *hdev_out the device copy of
// [S alpha | S beta | S mean | S zeros | S 1/beta].
int blr_heads_fast_enqueue(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap,
                           const double *bt, const double *mn, int z, bool want_terms, double **hdev_out) {
  const int d = net->dims[0];
  const size_t up_doubles = (size_t)N * d + (size_t)N + 5 * (size_t)S;   // [X0 | y | S alpha | S beta | S mean | S zeros | S 1/beta]
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (up_doubles + (size_t)N * z)));
  B7_TRY(b7_ensure(c, c->bL, sizeof(double) * (size_t)S * 64 * 64));
  B7_TRY(b7_ensure(c, c->bLinv, sizeof(double) * (size_t)S * 64 * 64));
  B7_TRY(b7_ensure(c, c->balpha, sizeof(double) * (size_t)S * 64));
  B7_TRY(b7_ensure(c, c->bresid, sizeof(double) * (size_t)S * 64));
  B7_TRY(b7_ensure(c, c->binfo, sizeof(int) * 4 * (size_t)S));
  B7_TRY(b7_ensure(c, c->bterms, sizeof(double) * 3 * (size_t)S + 64));
  // pinned, device-mapped block for the reports and the evidence's terms: [S][4] ints | [S][3] doubles
  const size_t rep_bytes = 16 * (size_t)S, term_bytes = sizeof(double) * 3 * (size_t)S;
  B7_TRY(b7_pin_ensure(c, c->pin_eval, rep_bytes + term_bytes, true));
  B7_TRY(b7_pin_ensure(c, c->pin_blr, sizeof(double) * up_doubles, false));
  B7_TRY(blr_head_setup(c, z, 0, c->mean, c->noise, false));  // S heads: no one mean or noise to record
  double *stage = static_cast<double *>(c->pin_blr.host);
  memcpy(stage, X0, sizeof(double) * (size_t)N * d);
  memcpy(stage + (size_t)N * d, Y0, sizeof(double) * N);
  double *hs = stage + (size_t)N * d + N;
  for (int s = 0; s < S; ++s) hs[s] = ap[s], hs[S + s] = bt[s], hs[2 * S + s] = mn[s], hs[3 * S + s] = 0.0, hs[4 * S + s] = 1.0 / bt[s];
  double *xdev = (double *)c->tmpmu.p, *ydev = xdev + (size_t)N * d, *hdev = ydev + N, *zdev = hdev + 5 * (size_t)S;
  B7_HIP(c, hipMemcpyAsync(xdev, stage, sizeof(double) * up_doubles, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_mlp_forward(c, xdev, N, d, (const double *)c->netbuf.p, net->dims, net->n_layers, net->activation, zdev, z));
  int *reports = static_cast<int *>(c->pin_eval.host);
  memset(reports, 0xff, rep_bytes);
  B7_TRY(launch_blr_heads_small(c, S, zdev, N, z, z, ydev, hdev, (double *)c->bL.p, (double *)c->bLinv.p, (double *)c->balpha.p,
                                (double *)c->bresid.p, (int *)c->binfo.p, static_cast<int *>(c->pin_eval.dev), (double *)c->bterms.p));
  if (want_terms)
    B7_HIP(c, hipMemcpyAsync(static_cast<char *>(c->pin_eval.host) + rep_bytes, c->bterms.p, term_bytes, hipMemcpyDeviceToHost, c->stream));
  *hdev_out = hdev;
  return B7_OK;
}

static int blr_marg_fast(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap,
                         const double *bt, const double *mn, int z, const b7_score_spec *spec, bool want_terms, ScoreParams *pend) {
  B7_TRY(b7_ensure(c, c->bmu, sizeof(double) * (size_t)S * c->M));
  B7_TRY(b7_ensure(c, c->bvar, sizeof(double) * (size_t)S * c->M));
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)c->M));
  double *hdev = nullptr;
  B7_TRY(blr_heads_fast_enqueue(c, net, X0, Y0, N, S, ap, bt, mn, z, want_terms, &hdev));
  B7_TRY(blr_feat_alloc(c, c->M, z));
  B7_TRY(launch_mlp_forward(c, (const double *)c->grid[c->grid_cur].p, c->M, c->d, (const double *)c->netbuf.p, net->dims,
                            net->n_layers, net->activation, (double *)c->feat.p, 64));
  B7_TRY(launch_gemv_rows_batch(c, S, (const double *)c->feat.p, 64, (const double *)c->balpha.p, 64, 64, hdev + 2 * (size_t)S, c->M,
                                (double *)c->bmu.p, c->M));
  B7_TRY(launch_post_heads(c, S, (const double *)c->bLinv.p, (const double *)c->feat.p, round_up(c->M, B7_MROWS), c->M,
                           (double *)c->bvar.p, c->M, hdev + 3 * (size_t)S, hdev + 4 * (size_t)S));
  double *fd = nullptr;
  if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
  acc_declare_zeros(c, spec->kind);
  B7_TRY(pending_score(c, S, spec, fd, pend));
  return B7_OK;
}

extern "C" {

int b7_blr_basis(b7_ctx *c, const b7_mlp *net, const double *X, int64_t M, double *Z_host) {
  if (!c) return B7_ERR_INVALID;
  B7_HIP(c, hipSetDevice(c->device));
  int z = 0;
  B7_TRY(blr_upload_net(c, net, &z));
  if (z > 256) return b7_fail(c, B7_ERR_UNSUPPORTED, "blr: basis width %d > 256", z);
  const int zpad = npad_of(c, z);
  if (!X) {  // resident grid -> resident features
    if (c->M <= 0 || c->d <= 0) return b7_fail(c, B7_ERR_STATE, "blr_basis: no candidate grid on this context");
    B7_TRY(blr_feat_alloc(c, c->M, z));
    B7_TRY(launch_mlp_forward(c, (const double *)c->grid[c->grid_cur].p, c->M, c->d, (const double *)c->netbuf.p,
                              net->dims, net->n_layers, net->activation, (double *)c->feat.p, zpad));
    if (Z_host)
      B7_HIP(c, hipMemcpy2DAsync(Z_host, sizeof(double) * z, c->feat.p, sizeof(double) * zpad, sizeof(double) * z,
                                 c->M, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    return B7_OK;
  }
  if (M < 1 || !Z_host) return b7_fail(c, B7_ERR_INVALID, "blr_basis: M >= 1 and Z_host required with X");
  const int d = net->dims[0];
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)M * d));
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * (size_t)M * z));
  B7_HIP(c, hipMemcpyAsync(c->tmpgrid.p, X, sizeof(double) * (size_t)M * d, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_mlp_forward(c, (const double *)c->tmpgrid.p, M, d, (const double *)c->netbuf.p, net->dims,
                            net->n_layers, net->activation, (double *)c->tmpmu.p, z));
  B7_HIP(c, hipMemcpyAsync(Z_host, c->tmpmu.p, sizeof(double) * (size_t)M * z, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_blr_features(b7_ctx *c, const double *Z1, int64_t M, int z) {
  if (!c) return B7_ERR_INVALID;
  if (!Z1 || M < 1 || z < 1 || z > 256) return b7_fail(c, B7_ERR_INVALID, "blr_features: bad arguments");
  B7_HIP(c, hipSetDevice(c->device));
  const int zpad = npad_of(c, z);
  B7_TRY(blr_feat_alloc(c, M, z));
  B7_HIP(c, hipMemcpy2DAsync(c->feat.p, sizeof(double) * zpad, Z1, sizeof(double) * z, sizeof(double) * z, M,
                             hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (c->M != M) {  // features stand in for a grid: the score calls size themselves by M
    c->M = M;
    c->d = 0;
    acc_forget(c);
    feas_forget(c);
    post_forget(c);
  }
  return B7_OK;
}

int b7_blr_fit(b7_ctx *c, const double *Z0, const double *Y0, int N, int z, double alpha_prec, double beta,
               double mean, double *nll_out) {
  if (!c) return B7_ERR_INVALID;
  if (!Z0 || !Y0 || N < 1 || z < 1 || z > 256) return b7_fail(c, B7_ERR_INVALID, "blr_fit: bad arguments");
  if (!(alpha_prec > 0.0) || !(beta > 0.0)) return b7_fail(c, B7_ERR_INVALID, "blr_fit: precisions must be > 0");
  B7_HIP(c, hipSetDevice(c->device));
  c->fitted = false;
  c->predicted = false;
  const int zpad = npad_of(c, z), nk = (int)round_up(N, 16);
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)zpad * nk));
  std::vector<double> zt((size_t)zpad * nk, 0.0);  // Z0' (a layout change, no arithmetic)
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < z; ++k) zt[(size_t)k * nk + i] = Z0[(size_t)i * z + k];
  B7_HIP(c, hipMemcpyAsync(c->tmpgrid.p, zt.data(), sizeof(double) * (size_t)zpad * nk, hipMemcpyHostToDevice,
                           c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return blr_fit_core(c, Y0, N, z, alpha_prec, beta, mean, nll_out);
}

int b7_blr_fit_x(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, double alpha_prec,
                 double beta, double mean, double *nll_out) {
  if (!c) return B7_ERR_INVALID;
  if (!X0 || !Y0 || N < 1) return b7_fail(c, B7_ERR_INVALID, "blr_fit_x: bad arguments");
  if (!(alpha_prec > 0.0) || !(beta > 0.0)) return b7_fail(c, B7_ERR_INVALID, "blr_fit_x: precisions must be > 0");
  B7_HIP(c, hipSetDevice(c->device));
  c->fitted = false;
  c->predicted = false;
  int z = 0;
  B7_TRY(blr_upload_net(c, net, &z));
  if (z > 256) return b7_fail(c, B7_ERR_UNSUPPORTED, "blr: basis width %d > 256", z);
  const int d = net->dims[0], zpad = npad_of(c, z), nk = (int)round_up(N, 16);
  B7_TRY(b7_ensure(c, c->tmpmu, sizeof(double) * ((size_t)N * d + (size_t)N * z)));
  B7_TRY(b7_ensure(c, c->tmpgrid, sizeof(double) * (size_t)zpad * nk));
  double *xdev = (double *)c->tmpmu.p, *zdev = xdev + (size_t)N * d;
  B7_HIP(c, hipMemcpyAsync(xdev, X0, sizeof(double) * (size_t)N * d, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_mlp_forward(c, xdev, N, d, (const double *)c->netbuf.p, net->dims, net->n_layers, net->activation,
                            zdev, z));
  B7_TRY(launch_transpose_pad(c, zdev, N, z, z, (double *)c->tmpgrid.p, zpad, nk));
  return blr_fit_core(c, Y0, N, z, alpha_prec, beta, mean, nll_out);
}

int b7_blr_predict(b7_ctx *c, double *mean_host, double *var_host) {
  if (!c) return B7_ERR_INVALID;
  if (!c->fitted || c->model_kind != 1) return b7_fail(c, B7_ERR_STATE, "blr_predict: no Bayesian-linear fit");
  if (c->Mfeat <= 0)
    return b7_fail(c, B7_ERR_STATE, "blr_predict: no current features (call b7_blr_basis / b7_blr_features after the "
                                    "last change of the candidate grid)");
  if (c->zdim != c->N) return b7_fail(c, B7_ERR_INVALID, "blr_predict: feature width %d != fit width %d", c->zdim, c->N);
  if (c->Mfeat != c->M) return b7_fail(c, B7_ERR_STATE, "blr_predict: features are stale (the grid changed)");
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->Mfeat;
  B7_TRY(blr_predict_enqueue(c, M));
  return copy_out_mu_var(c, c->mu.p, c->var.p, M, 1, mean_host, var_host);
}

int b7_blr_eval_nominate(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, double alpha_prec,
                         double beta, double mean, const b7_score_spec *spec, int64_t global_row_offset, double *best_val,
                         int64_t *best_idx1, double *jitter_used) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "blr_eval_nominate: this context belongs to a group");
  if (jitter_used) *jitter_used = 0.0;
  int rc = B7_OK, z = 0;
  if (!X0 || !Y0 || N < 1 || !spec) rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate: bad arguments");
  else if (!(alpha_prec > 0.0) || !(beta > 0.0)) rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate: precisions must be > 0");
  else rc = nominate_args(c, "blr_eval_nominate", spec, global_row_offset);
  if (rc == B7_OK && spec->kind == B7_SCORE_MES)
    rc = b7_fail(c, B7_ERR_UNSUPPORTED, "blr_eval_nominate: max-value entropy search is not built on this route (b7_blr_predict + b7_score_mes is)");
  if (rc == B7_OK) rc = hipSetDevice(c->device) == hipSuccess ? B7_OK : b7_fail(c, B7_ERR_HIP, "hipSetDevice failed");
  if (rc == B7_OK) rc = blr_upload_net(c, net, &z);
  if (rc == B7_OK && z > 256) rc = b7_fail(c, B7_ERR_UNSUPPORTED, "blr: basis width %d > 256", z);
  if (rc == B7_OK && c->M > 0 && net->dims[0] != c->d)
    rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate: network input width %d != grid dims %d", net->dims[0], c->d);
  return nominate_run(
      c, "blr_eval_nominate", rc, global_row_offset, 1.0,
      [&](ScoreParams *) {
        B7_TRY(blr_enqueue_fit(c, net, X0, Y0, N, z, alpha_prec, beta, mean));
        return blr_enqueue_score(c, net, z, spec);
      },
      [&]() { return reports_clean(c, c->pinned->fit.info, 1, true); },  // the head's report (blr_enqueue_fit)
      [&]() {  // the jitter schedule of utils/math.lua:159-218, through the synchronous fit
        B7_TRY(b7_blr_fit_x(c, net, X0, Y0, N, alpha_prec, beta, mean, nullptr));
        if (jitter_used) *jitter_used = -2.0;  // "a jitter was needed" (its size is the fit's business; see b7_blr_fit_x)
        return blr_enqueue_score(c, net, z, spec, false);
      },
      best_val, best_idx1);
}

int b7_blr_eval_nominate_marg(b7_ctx *c, const b7_mlp *net, const double *X0, const double *Y0, int N, int S, const double *ap,
                              const double *bt, const double *mn, const b7_score_spec *spec, int64_t global_row_offset,
                              double *best_val, int64_t *best_idx1, double *nll_out, double *jitter_used) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "blr_eval_nominate_marg: this context belongs to a group");
  if (jitter_used) *jitter_used = 0.0;
  int rc = B7_OK, z = 0;
  if (!X0 || !Y0 || N < 1 || S < 1 || !ap || !bt || !mn || !spec) rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate_marg: bad arguments");
  else rc = nominate_args(c, "blr_eval_nominate_marg", spec, global_row_offset);
  if (rc == B7_OK && spec->kind == B7_SCORE_MES)
    rc = b7_fail(c, B7_ERR_UNSUPPORTED, "blr_eval_nominate_marg: max-value entropy search is not built on this route (b7_blr_predict + b7_score_mes is)");
  for (int s = 0; rc == B7_OK && s < S; ++s)
    if (!(ap[s] > 0.0) || !(bt[s] > 0.0)) rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate_marg: precisions must be > 0 (sample %d)", s);
  if (rc == B7_OK) rc = hipSetDevice(c->device) == hipSuccess ? B7_OK : b7_fail(c, B7_ERR_HIP, "hipSetDevice failed");
  if (rc == B7_OK) rc = blr_upload_net(c, net, &z);
  if (rc == B7_OK && z > 256) rc = b7_fail(c, B7_ERR_UNSUPPORTED, "blr: basis width %d > 256", z);
  if (rc == B7_OK && c->M > 0 && net->dims[0] != c->d)
    rc = b7_fail(c, B7_ERR_INVALID, "blr_eval_nominate_marg: network input width %d != grid dims %d", net->dims[0], c->d);
  const bool fast = rc == B7_OK && z <= 64 && c->blr_small && c->npad_small;
  return nominate_run(
      c, "blr_eval_nominate_marg", rc, global_row_offset, (double)S,
      [&](ScoreParams *pend) {
        return fast ? blr_marg_fast(c, net, X0, Y0, N, S, ap, bt, mn, z, spec, nll_out != nullptr, pend)
                    : blr_marg_slow(c, net, X0, Y0, N, S, ap, bt, mn, z, spec, nll_out);
      },
      [&]() {  // the slow path needs no check: its fits went through the jitter schedule one by one
        if (!fast) return true;
        if (!reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, false)) return false;
        if (nll_out) {  // the evidence of every head from the kernel's three sums (Bishop 3.82 / 3.86, as blr_fit_core)
          const double *t = reinterpret_cast<const double *>(static_cast<const char *>(c->pin_eval.host) + 16 * (size_t)S);
          for (int s = 0; s < S; ++s) {
            const double Em = 0.5 * bt[s] * t[3 * s + 2] - 0.5 * t[3 * s + 1];
            nll_out[s] = -(0.5 * z * log(ap[s]) + 0.5 * N * log(bt[s]) - Em - t[3 * s] - 0.5 * N * log(2.0 * M_PI));
          }
        }
        c->fitted = false;  // the context's own fit slot holds none of the S heads
        return true;
      },
      [&]() {
        if (jitter_used) *jitter_used = -2.0;
        return blr_marg_slow(c, net, X0, Y0, N, S, ap, bt, mn, z, spec, nll_out);
      },
      best_val, best_idx1);
}

}  // extern "C"
