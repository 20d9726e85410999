// Greedy batch nomination: b7_eval_nominate's pick, then q - 1 more by kriging-believer variance downdates.
//
// No counterpart in the reference (bots/abstract.lua:118 nominates one point per trial).  The believer pretends that the row just
// picked, x_j, was observed at its own posterior mean under every hyper sample s.  The posterior mean of every candidate is then
// unchanged and the latent variance takes a rank-one downdate (include/bot7hip.h states the recurrence):
//   c_j(x)   = k(x, x_j) - K*(x, X) w_j,                  w_j = inv(K) k(X, x_j) = inv(L)' (inv(L) k(X, x_j))
//   u_j(x)   = (c_j(x) - sum_{i<j} u_i(x) u_i(x_j)) / sqrt(t_j),        t_j = var_j-1(x_j) + noise
//   var_j(x) = var_j-1(x) - u_j(x)^2
// Per extra pick and hyper sample: the column k(X, x_j) (believer_kernel's column pass over the N observations), w_j by the two
// triangular mat-vecs that make alpha (launch_alpha_batch), the downdate (believer_kernel over the grid), and one rescoring of
// all samples (score.hip's fused kernel, the rows already picked left out of its arg-max).  No factorisation, no variance product.
//
// believer_kernel is the slab walk of ksx_walk.h with w_j as the rider: the mean half of ksx_kernel (covar.hip) WITHOUT its stores
// of K*.  Prologue, slab loop and the tile (KsxWalk::cov_tile: MFMA distance product, arg = (c - xs/2) - zs/2 -> cov_nonpos4<KERN>)
// are the text ksx_kernel runs, so a downdated variance is made of the covariance entries the variance itself was made of, under
// either kernel.  k(x, x_j) comes out of one more 16x16 tile whose only live column is the
// believed point, scaled as prep_obs_kernel scales an observation.  The sum over the observations has ONE order -- per lane the
// columns lr, lr + 16, .. in slab order, then the xor-shuffle tree -- whatever the grid's size.  One text serves the general
// layout (Npad a multiple of 128) and the small regime (Npad 64 or 128): DESIGN.md section 3's padding and width classes.
#include <string.h>

#include <vector>

#include "b7_internal.h"
#include "gemm_f64.h"
#include "ksx_exp.h"
#include "ksx_walk.h"

namespace {

constexpr int BSC = 1 + B7_BATCH_MAX;   // a sample's scalars of one pick: t_j, then u_i(x_j) for i < j

// the kernel's own LDS behind the walk's: DPAD the believed point, scaled: x_j .* w | 1 + BSC zs/2 of the believed point | t_j, u_i(x_j)
constexpr int bel_extra(int dpad) { return dpad + 1 + BSC + 1; }

// The walk's rider is w_j: one word per row.
template <int DPAD, int KERN>
__global__ void __launch_bounds__(256) believer_kernel(BelPass p, int d, int Npad, int N, int column) {
  extern __shared__ __align__(16) double sm[];
  const int64_t s = blockIdx.z, S = gridDim.z;
  const double *w = p.w + s * DPAD, *zsc = p.zsc + s * (int64_t)Npad * DPAD, *zsh = p.zss + s * Npad;
  const double *wj = column ? nullptr : p.wj + s * Npad;
  const double amp = p.par[2 * s], tnoise = p.par[2 * s + 1];
  double *scal = p.scal + s * BSC;
  const int64_t Mtotal = p.rows;
  using T = KsxTile<DPAD, 1>;
  constexpr int KO = T::KO, dpad = DPAD;
  KsxWalk<DPAD, 1> wk(sm, zsc, zsh);
  const int tid = wk.tid, wave = wk.wave, lr = wk.lr, lq = wk.lq;
  const double *sh = wk.zs();
  double *sal = wk.rider();                 // 2 x KO   w_j of the slab
  double *sxj = wk.extra();                 // DPAD     the believed point, scaled: x_j .* w
  double *ssc = sxj + DPAD;                 // 1 + BSC  zs/2 of the believed point | t_j, u_i(x_j)
  const int64_t qbase = (int64_t)blockIdx.x * KSX_Q;
  const int nslab = column ? 0 : Npad / KO;

  double pre_a = 0.0;
  auto rider_load = [&](int sl) { pre_a = wj[sl * KO + tid]; };
  auto rider_store = [&](int buf) { sal[buf * KO + tid] = pre_a; };
  wk.begin(p.xq, qbase, Mtotal, d, w, amp, 0, nslab, [&] {
    // the believed point as prep_obs_kernel makes an observation: z .* w, and (sum z^2 w)/2 in ascending k
    if (tid >= 128 && tid < 128 + dpad) {
      const int k = tid - 128;
      sxj[k] = (k < d) ? p.xj[k] * w[k] : 0.0;
    }
    if (tid == 255) {
      double a = 0.0;
      for (int k = 0; k < d; ++k) {
        const double z = p.xj[k];
        a += (z * z) * w[k];
      }
      ssc[0] = 0.5 * a;
    }
    if (!column && tid >= 192 && tid < 192 + 1 + p.j) ssc[1 + (tid - 192)] = scal[tid - 192];
  }, rider_load, rider_store);

  double hq[4], macc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 4; ++r) hq[r] = wk.xs()[wave * 16 + lq + 4 * r];

  wk.run(0, nslab, rider_load, rider_store, [&](int, int cur, int t, const double (&bf)[T::KSTEPS]) {
    const d4_t c = wk.dist(bf);
    const double hk = sh[cur * KO + t * 16 + lr];
    const double al = sal[cur * KO + t * 16 + lr];
    double kv[4];
    wk.template cov<KERN>(c, hq, hk, kv);
#pragma unroll
    for (int r = 0; r < 4; ++r) macc[r] = __builtin_fma(kv[r], al, macc[r]);
  });

  // k(x, x_j): one more tile; column 0 is the believed point, the other fifteen are padding (zs/2 = 1e300 -> exactly 0)
  double kx[4];
  {
    double bf[T::KSTEPS];
#pragma unroll
    for (int k4 = 0; k4 < T::KSTEPS; ++k4) bf[k4] = (lr == 0) ? sxj[lq + 4 * k4] : 0.0;
    wk.template cov<KERN>(wk.dist(bf), hq, (lr == 0) ? ssc[0] : 1e300, kx);
  }

  if (column) {
    // the column k(X, x_j) over the observation rows (0 in the padding), and the believed row's scalars, read before the
    // downdate that follows on the stream rewrites var
    if (lr == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t g = qbase + wave * 16 + lq + 4 * r;
        if (g < Npad) p.kcol[s * Npad + g] = (g < N) ? kx[r] : 0.0;
      }
    }
    if (blockIdx.x == 0 && tid <= p.j)
      scal[tid] = (tid == 0) ? p.var[s * p.sgrid + p.idx] + tnoise : p.u[((int64_t)(tid - 1) * S + s) * p.sgrid + p.idx];
    return;
  }

  const double rs = sqrt(ssc[1]);
  double *var = p.var + s * p.sgrid, *uj = p.u + ((int64_t)p.j * S + s) * p.sgrid;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = macc[r];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    const int64_t g = qbase + wave * 16 + lq + 4 * r;
    if (lr == 0 && g < Mtotal) {
      double cc = kx[r] - v;
      for (int i = 0; i < p.j; ++i) cc = __builtin_fma(-p.u[((int64_t)i * S + s) * p.sgrid + g], ssc[2 + i], cc);
      const double u = cc / rs;
      uj[g] = u;
      var[g] = __builtin_fma(-u, u, var[g]);
    }
  }
}

int bel_launch(b7_ctx *c, int S, const BelPass &p, bool column) {
  return ksx_for_class(c, "believer kernel", [&](auto cls) {
    using C = decltype(cls);
    const size_t lds = KsxTile<C::DPAD, 1>::lds_bytes(bel_extra(C::DPAD));
    auto kern = believer_kernel<C::DPAD, C::KERN>;
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t blocks = column ? c->Npad / KSX_Q : (p.rows + KSX_Q - 1) / KSX_Q;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, 1, S), dim3(256), lds, c->stream, p, c->dfit, c->Npad, c->N, column ? 1 : 0);
    B7_HIP(c, hipGetLastError());
    return B7_OK;
  });
}

// the per-sample arrays of a call, carved out of c->bel and c->belvec
struct BelState {
  double *mu, *var, *u;                // [S][M], [S][M], [q - 1][S][M]
  double *kcol, *wj, *par, *scal;      // [S][Npad], [S][Npad], [S][2], [S][BSC]
};

int bel_state(b7_ctx *c, int S, int q, BelState *st) {
  const size_t SM = (size_t)S * c->M, n = (size_t)c->Npad;
  B7_TRY(b7_ensure(c, c->bel, sizeof(double) * SM * (size_t)(q + 1)));
  B7_TRY(b7_ensure(c, c->belvec, sizeof(double) * (size_t)S * (2 * n + 2 + BSC)));
  B7_TRY(b7_pin_ensure(c, c->pin_bel, sizeof(double) * 2 * (size_t)S, false));
  st->mu = (double *)c->bel.p, st->var = st->mu + SM, st->u = st->var + SM;
  st->kcol = (double *)c->belvec.p, st->wj = st->kcol + S * n, st->par = st->wj + S * n, st->scal = st->par + 2 * (size_t)S;
  return B7_OK;
}

}  // namespace

int launch_believer(b7_ctx *c, int S, const BelPass &p, bool column) {
  PhaseScope ps(c, "believer");
  return bel_launch(c, S, p, column);
}

extern "C" {

int b7_eval_nominate_batch(b7_ctx *c, int S, const b7_hyp *hyps, const b7_score_spec *spec, int q, double *best_val,
                           int64_t *best_idx1, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "eval_nominate_batch: this context belongs to a group (sharded batches are not built)");
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_batch: q = %d not in [1, %d]", q, B7_BATCH_MAX);
  if (!best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_batch: best_val and best_idx1 take q entries each");
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_batch: a communicator of %d ranks (sharded batches are not built)", c->comm_world);
  B7_TRY(eval_validate(c, S, hyps, spec, 0));
  if (spec->kind == B7_SCORE_MES)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_batch: max-value entropy search is not built for batches (y* would have to follow the believer downdates)");
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_batch: %d response columns (one is built)", c->ycols);
  if (c->opts.var_with_noise || c->opts.var_clamp)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_nominate_batch: the downdate works on the latent variance (var_with_noise / var_clamp are set)");
  if (q > c->M) return b7_fail(c, B7_ERR_INVALID, "eval_nominate_batch: q = %d exceeds the grid's %lld rows", q, (long long)c->M);
  if (q == 1) return b7_eval_nominate(c, S, hyps, spec, 0, best_val, best_idx1, jitter_out, info_out);

  B7_HIP(c, hipSetDevice(c->device));
  BelState st;
  B7_TRY(bel_state(c, S, q, &st));
  std::vector<double> jit(S, 0.0);
  if (jitter_out) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out) std::fill(info_out, info_out + S, 0);
  BelKeep keep;
  keep.mu = st.mu, keep.var = st.var;
  // pick 1: b7_eval_nominate's own protocol and launches; every sample's mean, variance and fit are kept on the way
  B7_TRY(nominate_run(
      c, "eval_nominate_batch", B7_OK, 0, (double)S, [&](ScoreParams *pend) { return eval_enqueue(c, S, hyps, spec, pend, &keep); },
      [&]() { return reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true); },
      [&]() { return eval_redo(c, S, hyps, spec, jit.data(), info_out, &keep); }, &best_val[0], &best_idx1[0]));
  if (jitter_out) memcpy(jitter_out, jit.data(), sizeof(double) * S);

  double *par_host = static_cast<double *>(c->pin_bel.host);
  for (int s = 0; s < S; ++s) {
    par_host[2 * s] = hyps[s].amp;
    par_host[2 * s + 1] = hyps[s].noise + (jit[s] > 0.0 ? jit[s] : 0.0);  // what went on the diagonal of the K that was factored
  }
  B7_HIP(c, hipMemcpyAsync(st.par, par_host, sizeof(double) * 2 * (size_t)S, hipMemcpyHostToDevice, c->stream));
  double *fd = nullptr;
  if (score_needs_fmin(spec->kind)) B7_TRY(stage_fmin(c, spec->fmin, &fd));
  const double *grid = (const double *)c->grid[c->grid_cur].p;
  ExclRows picked;
  picked.row[picked.n++] = best_idx1[0] - 1;
  for (int j = 1; j < q; ++j) {
    BelPass p;
    p.xj = grid + (best_idx1[j - 1] - 1) * c->d;
    p.w = keep.fits.w, p.zsc = keep.fits.zsc, p.zss = keep.fits.zss;
    p.wj = st.wj, p.par = st.par, p.scal = st.scal, p.kcol = st.kcol;
    p.var = st.var, p.u = st.u, p.sgrid = c->M;
    p.idx = best_idx1[j - 1] - 1, p.j = j - 1;
    p.xq = (const double *)c->xobs.p, p.rows = c->N;
    B7_TRY(launch_believer(c, S, p, true));
    B7_TRY(launch_alpha_batch(c, S, keep.fits.Linv, st.kcol, st.wj));
    p.xq = grid, p.rows = c->M;
    B7_TRY(launch_believer(c, S, p, false));
    // the whole grid again: the kept means, the downdated variances, the caller's spec; the picked rows stay out of the arg-max
    acc_declare_zeros(c, spec->kind);
    ScoreParams pend = score_params(c, spec, fd);
    pend.S = S, pend.mu = st.mu, pend.var = st.var, pend.stride = c->M;
    B7_TRY(exch_local(c, (double)S, 0, 0, 1, true, true, &pend, &picked));
    B7_TRY(exch_wait_mirror(c));
    B7_TRY(exch_conclude(c, c->tab_host, 1, &best_val[j], &best_idx1[j]));
    picked.row[picked.n++] = best_idx1[j] - 1;
  }
  c->fitted = false;  // the context's own fit slot holds none of the samples, as after b7_eval_nominate
  c->predicted = false;
  return B7_OK;
}

#ifdef B7_DIAG
// diagnostic build only: hyper sample s's variance over the grid as the last b7_eval_nominate_batch (q > 1) left it
int b7dbg_believer_var(b7_ctx *c, int S, int s, double *out_host) {
  if (!c || !out_host || s < 0 || s >= S || !c->bel.p || c->bel.cap < sizeof(double) * (size_t)S * c->M * 2) return B7_ERR_INVALID;
  B7_HIP(c, hipStreamSynchronize(c->stream));
  B7_HIP(c, hipMemcpy(out_host, (const double *)c->bel.p + ((size_t)S + s) * c->M, sizeof(double) * (size_t)c->M, hipMemcpyDeviceToHost));
  return B7_OK;
}
#endif

}  // extern "C"
