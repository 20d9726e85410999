// Two-objective nomination: the exact expected hypervolume improvement (the two-objective case of Emmerich, Yang & Deutz 2016),
// marginalised over the hyper samples of two independent GPs, linear (b7_ehvi_*) and in log space (b7_logehvi_*), and the kept
// posterior it reads.  No counterpart in the reference's scores/.  Both objectives are minimised.
//
// Front (a_k, b_k), k = 1..P, canonical (bot7hip.h): strictly inside the reference box, a ascending, b descending, both strictly.
// a_0 = -inf, a_P+1 = r1, b_0 = r2.  Strip k = 0..P is [a_k, a_k+1] x (-inf, b_k]:
//   score_j = sum_k A_k B_k,   A_k = (1/S1) sum_s max(Psi(a_k+1; s) - Psi(a_k; s), 0),   B_k = (1/S2) sum_t Psi(b_k; t),
// with Psi, the log-space form of every operation here and its row classes in ehvi_math.h.  Contraction off: one rounded operation per
// operator.  Order: k ascending, s / t ascending within it, each sum divided once by its sample count; Psi(a_k+1; s) is evaluated once
// and kept as strip k + 1's Psi(a_k; s).  The clamp at 0 keeps every term non-negative, so the linear score is >= 0.
// Row classes: any mu or var NaN, any var < 0, in either objective: NaN.  Otherwise finite for finite input, P = 0 included (log
// space: -inf is legal).
//
// ehvi2_kernel<Alg>, Alg = EhviLin or EhviLog: one candidate per lane, one wave per workgroup.  The front and ref arrive as two arrays
// of P + 1 doubles indexed by the strip, a wave-uniform index: scalar loads.  A sample's NV staged values (mu, sigma; log sigma too in
// log space) are made once from the coalesced [S][M] layout; the first B7_EHVI_SREG samples of each objective and their running
// Psi(a_k; s) live in registers across the strips (fully unrolled, guarded by the wave-uniform sample counts), samples beyond that in
// LDS columns of the lane's own ([value][sample][lane]: no bank conflict, no barrier -- a lane reads only what it wrote), up to
// B7_EHVI_SMAX per objective: ((NV + 1) x1 + NV x2) 512 bytes of dynamic LDS for x1 / x2 samples beyond the registers: 3 x1 + 2 x2
// columns, 56 320 bytes at most, linear; 4 x1 + 3 x2, 78 848 at most, in log space (above 64 KiB: opted in).  The summation order is
// the same on both sides of the limit.
//
// Out of scope, refused by name where it can be asked for: more than two objectives here (three through ehvi3.hip's b7_ehvi3_*, four
// and more nowhere), correlated objectives / multi-task GPs,
// batches of expected improvements (q nominees per call come from Thompson paths: ts_hvi.hip's b7_ts_hvi_nominate), refinement,
// constraints combined with objectives, sharded grids and groups, the Bayesian-linear head, ParEGO-style scalarisation.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "ehvi_math.h"

namespace {

constexpr int SR = B7_EHVI_SREG;
constexpr int EHVI_LANES = 64;

struct Ehvi2Args {
  const double *mu1, *var1, *mu2, *var2;  // [S1][M], [S2][M]
  const double *av, *bv;                  // [P + 1]: a_1 .. a_P, r1 | r2, b_1 .. b_P
  long long M;
  int S1, S2, P;
  double *out;                            // [M]
};

template <class Alg>
__global__ void __launch_bounds__(EHVI_LANES) ehvi2_kernel(Ehvi2Args g) {
  extern __shared__ double sh[];
  constexpr int NV = Alg::NV;
  const long long j = (long long)blockIdx.x * EHVI_LANES + threadIdx.x;
  if (j >= g.M) return;
  const int x1 = g.S1 > SR ? g.S1 - SR : 0, x2 = g.S2 > SR ? g.S2 - SR : 0;
  // value c of the lane's LDS sample i at [(c * x + i) * 64]: objective 1's NV values, its running Psi, objective 2's NV values
  double *l1 = sh + threadIdx.x, *lp1 = l1 + NV * x1 * EHVI_LANES, *l2 = lp1 + x1 * EHVI_LANES;
  double r1[SR][NV], p1[SR], r2[SR][NV];
  bool bad = false;
  auto take = [&](const double *mu, const double *var, int s, double *v) {  // sample s of this candidate, and its row class
    const double m = mu[(long long)s * g.M + j], vv = var[(long long)s * g.M + j];
    bad = bad || !(vv >= 0.0) || m != m;
    Alg::stage(m, vv, v);
  };
#pragma unroll
  for (int s = 0; s < SR; ++s)
    if (s < g.S1) take(g.mu1, g.var1, s, r1[s]), p1[s] = Alg::none();
  for (int s = 0; s < x1; ++s) {
    double v[NV];
    take(g.mu1, g.var1, SR + s, v);
#pragma unroll
    for (int c = 0; c < NV; ++c) l1[(c * x1 + s) * EHVI_LANES] = v[c];
    lp1[s * EHVI_LANES] = Alg::none();
  }
#pragma unroll
  for (int t = 0; t < SR; ++t)
    if (t < g.S2) take(g.mu2, g.var2, t, r2[t]);
  for (int t = 0; t < x2; ++t) {
    double v[NV];
    take(g.mu2, g.var2, SR + t, v);
#pragma unroll
    for (int c = 0; c < NV; ++c) l2[(c * x2 + t) * EHVI_LANES] = v[c];
  }
  if (bad) {
    g.out[j] = NAN;
    return;
  }
  const double n1 = Alg::count(g.S1), n2 = Alg::count(g.S2);
  typename Alg::Fold score = Alg::empty();
  for (int k = 0; k <= g.P; ++k) {
    const double a = g.av[k], b = g.bv[k];
    typename Alg::Fold A = Alg::empty(), B = Alg::empty();
#pragma unroll
    for (int s = 0; s < SR; ++s)
      if (s < g.S1) {
        const double p = Alg::psi(a, r1[s]);
        Alg::add(A, Alg::diff(p, p1[s]));
        p1[s] = p;
      }
    for (int s = 0; s < x1; ++s) {
      double v[NV];
#pragma unroll
      for (int c = 0; c < NV; ++c) v[c] = l1[(c * x1 + s) * EHVI_LANES];
      const double p = Alg::psi(a, v);
      Alg::add(A, Alg::diff(p, lp1[s * EHVI_LANES]));
      lp1[s * EHVI_LANES] = p;
    }
#pragma unroll
    for (int t = 0; t < SR; ++t)
      if (t < g.S2) Alg::add(B, Alg::psi(b, r2[t]));
    for (int t = 0; t < x2; ++t) {
      double v[NV];
#pragma unroll
      for (int c = 0; c < NV; ++c) v[c] = l2[(c * x2 + t) * EHVI_LANES];
      Alg::add(B, Alg::psi(b, v));
    }
    Alg::add(score, Alg::times(Alg::mean(A, n1), Alg::mean(B, n2)));
  }
  g.out[j] = Alg::value(score);
}

template <class Alg>
size_t lds_bytes(int S1, int S2) {
  const int x1 = S1 > SR ? S1 - SR : 0, x2 = S2 > SR ? S2 - SR : 0;
  return sizeof(double) * EHVI_LANES * (size_t)((Alg::NV + 1) * x1 + Alg::NV * x2);
}

bool finite2(const double *p) { return std::isfinite(p[0]) && std::isfinite(p[1]); }

// 0: canonical.  Otherwise what is wrong, for the messages: 1 ref not finite; 2 point k not finite; 3 point k not strictly inside the
// box; 4 points k - 1, k not strictly ascending in the first objective; 5 point k dominated (the second does not descend strictly)
int front_defect(const double *front, int P, const double *ref, int *k_out) {
  *k_out = 0;
  if (!finite2(ref)) return 1;
  for (int k = 0; k < P; ++k) {
    const double *p = front + 2 * (size_t)k;
    *k_out = k;
    if (!finite2(p)) return 2;
    if (!(p[0] < ref[0] && p[1] < ref[1])) return 3;
    if (k > 0 && !(p[0] > p[-2])) return 4;
    if (k > 0 && !(p[1] < p[-1])) return 5;
  }
  return 0;
}

}  // namespace

// front_refuse is ts_hvi.hip's too (b7_internal.h)
int front_refuse(b7_ctx *c, const char *who, const double *front, int P, const double *ref) {
  if (!ref) return b7_fail(c, B7_ERR_INVALID, "%s: ref is NULL", who);
  if (P < 0 || P > B7_EHVI_PMAX) return b7_fail(c, B7_ERR_INVALID, "%s: a front of %d points (0..%d are built)", who, P, B7_EHVI_PMAX);
  if (P > 0 && !front) return b7_fail(c, B7_ERR_INVALID, "%s: front is NULL", who);
  int k = 0;
  switch (front_defect(front, P, ref, &k)) {
    case 0: return B7_OK;
    case 1: return b7_fail(c, B7_ERR_INVALID, "%s: the reference point (%g, %g) is not finite", who, ref[0], ref[1]);
    case 2: return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d (%g, %g) is not finite", who, k + 1, front[2 * k], front[2 * k + 1]);
    case 3:
      return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d (%g, %g) is not strictly inside the reference box (%g, %g)", who,
                     k + 1, front[2 * k], front[2 * k + 1], ref[0], ref[1]);
    case 4:
      return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: points %d and %d are not sorted, the first objective strictly ascending",
                     who, k, k + 1);
    default:
      return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d is dominated by point %d (the second objective descends strictly)",
                     who, k + 1, k);
  }
}

namespace {

// the front as the kernel reads it, on its way to c->ehvi_front on c's stream: the host block must outlive the copy (the callers wait)
int front_stage(b7_ctx *c, const double *front, int P, const double *ref, std::vector<double> *host) {
  host->resize(2 * (size_t)(P + 1));
  double *av = host->data(), *bv = av + (P + 1);
  for (int k = 0; k < P; ++k) av[k] = front[2 * k], bv[k + 1] = front[2 * k + 1];
  av[P] = ref[0], bv[0] = ref[1];
  B7_TRY(b7_ensure(c, c->ehvi_front, sizeof(double) * 2 * (B7_EHVI_PMAX + 1)));
  B7_HIP(c, hipMemcpyAsync(c->ehvi_front.p, host->data(), sizeof(double) * host->size(), hipMemcpyHostToDevice, c->stream));
  return B7_OK;
}

int samples_refuse(b7_ctx *c, const char *who, int S1, int S2) {
  if (S1 < 1 || S1 > B7_EHVI_SMAX || S2 < 1 || S2 > B7_EHVI_SMAX)
    return b7_fail(c, B7_ERR_INVALID, "%s: S1 = %d, S2 = %d hyper samples (1..%d each are built)", who, S1, S2, B7_EHVI_SMAX);
  return B7_OK;
}

// the score of M rows onto out (device), on c's stream; the front staged by front_stage
template <class Alg>
int launch_ehvi2(b7_ctx *c, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2, int P, int64_t M,
                 double *out) {
  PhaseScope ps(c, Alg::phase2);
  Ehvi2Args g;
  g.mu1 = mu1, g.var1 = var1, g.mu2 = mu2, g.var2 = var2;
  g.av = (const double *)c->ehvi_front.p, g.bv = g.av + (P + 1);
  g.M = (long long)M, g.S1 = S1, g.S2 = S2, g.P = P, g.out = out;
  const int64_t nb = (M + EHVI_LANES - 1) / EHVI_LANES;
  if (nb > 0x7fffffffLL) return b7_fail(c, B7_ERR_INVALID, "%s: %lld rows are more than one launch takes", Alg::phase2, (long long)M);
  const size_t lds = lds_bytes<Alg>(S1, S2);
  // dynamic LDS above the 64 KiB default needs an explicit opt-in, per device (gfx950 has 160 KiB per workgroup)
  if (lds > (size_t)(64 << 10))
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(ehvi2_kernel<Alg>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(ehvi2_kernel<Alg>, dim3((unsigned)nb), dim3(EHVI_LANES), lds, c->stream, g);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// b7_ehvi_compute / b7_logehvi_compute: the score of the caller's host arrays
int ehvi2_compute(b7_ctx *c, bool log, const char *who, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                  const double *front, int P, const double *ref, int64_t M, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || (M > 0 && (!mu1 || !var1 || !mu2 || !var2 || !out))) return b7_fail(c, B7_ERR_INVALID, "%s: bad arguments (M >= 0, arrays required)", who);
  B7_TRY(samples_refuse(c, who, S1, S2));
  B7_TRY(front_refuse(c, who, front, P, ref));
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t m = (size_t)M, n1 = (size_t)S1 * m, n2 = (size_t)S2 * m;
  B7_TRY(b7_ensure(c, c->ehvi_user, sizeof(double) * (2 * n1 + 2 * n2 + m)));  // a buffer of its own: the kept posterior stays
  double *d1 = (double *)c->ehvi_user.p, *v1 = d1 + n1, *d2 = v1 + n1, *v2 = d2 + n2, *od = v2 + n2;
  std::vector<double> fh;
  B7_TRY(front_stage(c, front, P, ref, &fh));
  B7_HIP(c, hipMemcpyAsync(d1, mu1, sizeof(double) * n1, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(v1, var1, sizeof(double) * n1, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(d2, mu2, sizeof(double) * n2, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(v2, var2, sizeof(double) * n2, hipMemcpyHostToDevice, c->stream));
  B7_TRY(log ? launch_ehvi2<EhviLog>(c, d1, v1, S1, d2, v2, S2, P, M, od) : launch_ehvi2<EhviLin>(c, d1, v1, S1, d2, v2, S2, P, M, od));
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staged front are consumed
  return B7_OK;
}

}  // namespace

int ehvi_nominate(b7_ctx *const *o, int n, bool log, const char *who, const double *front, int P, const double *ref, double *best_val,
                  int64_t *best_idx1) {
  static const char *const nth[3] = {"first", "second", "third"};
  b7_ctx *c = o[0];
  if (!c) return B7_ERR_INVALID;
  for (int m = 1; m < n; ++m)
    if (!o[m]) return b7_fail(c, B7_ERR_INVALID, "%s: the %s objective's context is NULL", who, nth[m]);
  if (!best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (best_val and best_idx1 are needed)", who);
  for (int m = 0; m < n; ++m)
    if (o[m]->group)
      return b7_fail(c, B7_ERR_STATE, "%s: a context belongs to a group (%s objectives over a sharded grid are not built)", who, n == 2 ? "two" : "three");
  for (int m = 1; m < n; ++m)
    if (o[m]->device != c->device)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the %s objective's context is on device %d, this one on device %d (a posterior across devices is not built)",
                     who, nth[m], o[m]->device, c->device);
  for (int m = 0; m < n; ++m)
    if (!o[m]->post_valid)  // (the two-objective calls' first message has always been the shorter one)
      return b7_fail(c, B7_ERR_STATE, "%s: no kept posterior of the %s objective (call b7_eval_posterior%s; a change of the grid or the data forgets it)",
                     who, nth[m], n == 2 && m == 0 ? "" : " on its context");
  for (int m = 1; m < n; ++m)
    if (o[m]->post_M != c->post_M)
      return b7_fail(c, B7_ERR_INVALID, "%s: the %s objective's grid has %lld rows, this one %lld", who, nth[m], (long long)o[m]->post_M,
                     (long long)c->post_M);
  int S[3] = {0, 0, 0};
  for (int m = 0; m < n; ++m) S[m] = o[m]->post_S;
  B7_TRY(n == 2 ? samples_refuse(c, who, S[0], S[1]) : samples3_refuse(c, who, S));
  B7_TRY(n == 2 ? front_refuse(c, who, front, P, ref) : front3_refuse(c, who, front, P, ref));
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->post_M;  // == c->M: a grid change would have forgotten the posterior
  const double *mu[3], *var[3];
  for (int m = 0; m < n; ++m) mu[m] = (const double *)o[m]->post.p, var[m] = mu[m] + (size_t)S[m] * (size_t)M;
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)M));
  double *acc = (double *)c->acc.p;
  // the staged front's host block outlives its copy: launch_finish waits
  std::vector<double> fh;
  Staged3 st;
  if (n == 2) B7_TRY(front_stage(c, front, P, ref, &fh));
  else stage3_host(front, P, ref, &st);
  B7_TRY(streams_order(o, n, true));
  // the accumulator is declared written (linear: zeros; log space: a log accumulator); the kernel then writes every row of it
  if (log) acc_declare_log_written(c);
  else B7_TRY(acc_write_zeros(c));
  if (n == 3) B7_TRY(launch_ehvi3(c, log, mu, var, S, st, M, acc));
  else if (log) B7_TRY(launch_ehvi2<EhviLog>(c, mu[0], var[0], S[0], mu[1], var[1], S[1], P, M, acc));
  else B7_TRY(launch_ehvi2<EhviLin>(c, mu[0], var[0], S[0], mu[1], var[1], S[1], P, M, acc));
  B7_TRY(streams_order(o, n, false));
  // score:max(1) of the accumulator, the divisor 1 (log space: log 1 == 0 is subtracted); waits, so the staged front is consumed
  return launch_finish(c, acc, M, 1.0, best_val, best_idx1, log);
}

extern "C" {

int b7_eval_posterior(b7_ctx *c, int S, const b7_hyp *hyps, double *jitter_out, int *info_out) {
  if (!c) return B7_ERR_INVALID;
  if (c->group) return b7_fail(c, B7_ERR_STATE, "eval_posterior: this context belongs to a group (a kept posterior over a sharded grid is not built)");
  if (jitter_out && S > 0) std::fill(jitter_out, jitter_out + S, 0.0);
  if (info_out && S > 0) std::fill(info_out, info_out + S, 0);
  if (c->comm && c->comm_world > 1)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_posterior: a communicator of %d ranks (a kept posterior over a sharded grid is not built)", c->comm_world);
  // the fits and posteriors are b7_eval_nominate's, asked for through a score that needs no f_min; its values are not used
  const b7_score_spec spec{B7_SCORE_CB, 0.0, 0, 1.0, nullptr};
  B7_TRY(eval_validate(c, S, hyps, &spec, 0));
  if (c->ycols != 1) return b7_fail(c, B7_ERR_UNSUPPORTED, "eval_posterior: %d response columns (one is built)", c->ycols);
  B7_HIP(c, hipSetDevice(c->device));
  c->post_valid = false;  // (not post_forget: neither the grid nor the data changes here)
  const size_t SM = (size_t)S * (size_t)c->M;
  B7_TRY(b7_ensure(c, c->post, sizeof(double) * 2 * SM));
  BelKeep keep;
  keep.mu = (double *)c->post.p, keep.var = keep.mu + SM;
  ScoreParams unused;  // the small regime leaves its score:add pending: it is never launched
  B7_TRY(eval_enqueue(c, S, hyps, &spec, &unused, &keep));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (!reports_clean(c, static_cast<const int *>(c->pin_eval.host), S, true)) {
    B7_TRY(eval_redo(c, S, hyps, &spec, jitter_out, info_out, &keep));
    B7_HIP(c, hipStreamSynchronize(c->stream));
  }
  acc_forget(c);       // what the inline routes scored is dropped with the pending score: no accumulator afterwards
  c->fitted = false;   // the context's own fit slot holds none of the samples, as after b7_eval_nominate
  c->predicted = false;
  c->post_S = S, c->post_M = c->M, c->post_valid = true;
  return B7_OK;
}

int b7_posterior_get(b7_ctx *c, int s, double *mean, double *var) {
  if (!c) return B7_ERR_INVALID;
  if (!c->post_valid) return b7_fail(c, B7_ERR_STATE, "posterior_get: no kept posterior on this context (call b7_eval_posterior; a change of the grid or the data forgets it)");
  if (s < 0 || s >= c->post_S) return b7_fail(c, B7_ERR_INVALID, "posterior_get: sample %d outside the %d kept", s, c->post_S);
  B7_HIP(c, hipSetDevice(c->device));
  const size_t M = (size_t)c->post_M, SM = (size_t)c->post_S * M;
  const double *mu = (const double *)c->post.p;
  if (mean) B7_HIP(c, hipMemcpyAsync(mean, mu + (size_t)s * M, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
  if (var) B7_HIP(c, hipMemcpyAsync(var, mu + SM + (size_t)s * M, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));
  return B7_OK;
}

int b7_pareto_front2(const double *Y, int64_t n, const double *ref, double *front_out, int64_t *rows1_out, int *P_out) {
  if (!ref || !P_out || n < 0 || (n > 0 && (!Y || !front_out))) return B7_ERR_INVALID;
  *P_out = 0;
  if (!finite2(ref)) return B7_ERR_INVALID;
  std::vector<int64_t> in;
  for (int64_t i = 0; i < n; ++i)
    if (finite2(Y + 2 * i) && Y[2 * i] < ref[0] && Y[2 * i + 1] < ref[1]) in.push_back(i);
  // by the first objective, then the second, then the row: a point stays iff it lowers the second objective's running minimum
  std::sort(in.begin(), in.end(), [&](int64_t p, int64_t q) {
    if (Y[2 * p] != Y[2 * q]) return Y[2 * p] < Y[2 * q];
    if (Y[2 * p + 1] != Y[2 * q + 1]) return Y[2 * p + 1] < Y[2 * q + 1];
    return p < q;
  });
  std::vector<int64_t> keep;
  double low = INFINITY;
  for (int64_t i : in)
    if (Y[2 * i + 1] < low) {
      keep.push_back(i);
      low = Y[2 * i + 1];
    }
  *P_out = keep.size() > (size_t)0x7fffffff ? 0x7fffffff : (int)keep.size();
  if (keep.size() > (size_t)B7_EHVI_PMAX) return B7_ERR_INVALID;
  for (size_t k = 0; k < keep.size(); ++k) {
    front_out[2 * k] = Y[2 * keep[k]], front_out[2 * k + 1] = Y[2 * keep[k] + 1];
    if (rows1_out) rows1_out[k] = keep[k] + 1;
  }
  return B7_OK;
}

int b7_hypervolume2(const double *front, int P, const double *ref, double *hv_out) {
  if (!ref || !hv_out || P < 0 || (P > 0 && !front)) return B7_ERR_INVALID;
  int k = 0;
  if (front_defect(front, P, ref, &k) != 0) return B7_ERR_INVALID;
  double hv = 0.0;
  for (k = 0; k < P; ++k) {
    const double next = (k + 1 < P) ? front[2 * (k + 1)] : ref[0];
    hv = hv + ((next - front[2 * k]) * (ref[1] - front[2 * k + 1]));
  }
  *hv_out = hv;
  return B7_OK;
}

int b7_ehvi_compute(b7_ctx *c, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                    const double *front, int P, const double *ref, int64_t M, double *out) {
  return ehvi2_compute(c, false, "ehvi_compute", mu1, var1, S1, mu2, var2, S2, front, P, ref, M, out);
}

int b7_logehvi_compute(b7_ctx *c, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                       const double *front, int P, const double *ref, int64_t M, double *out) {
  return ehvi2_compute(c, true, "logehvi_compute", mu1, var1, S1, mu2, var2, S2, front, P, ref, M, out);
}

int b7_ehvi_nominate(b7_ctx *c, b7_ctx *other, const double *front, int P, const double *ref, double *best_val, int64_t *best_idx1) {
  b7_ctx *const o[2] = {c, other};
  return ehvi_nominate(o, 2, false, "ehvi_nominate", front, P, ref, best_val, best_idx1);
}

int b7_logehvi_nominate(b7_ctx *c, b7_ctx *other, const double *front, int P, const double *ref, double *best_val, int64_t *best_idx1) {
  b7_ctx *const o[2] = {c, other};
  return ehvi_nominate(o, 2, true, "logehvi_nominate", front, P, ref, best_val, best_idx1);
}

}  // extern "C"

