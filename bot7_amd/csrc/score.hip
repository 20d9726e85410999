// Acquisition scoring and the arg-max, with the reference's operation order.
//
// Reference arithmetic replaced (one rounded op here per Torch tensor op there; contraction is off):
//   utils/math.lua:261-288  erf   A&S 7.1.26: t = 1/(1+p|x|); Horner in t; 1 - poly*exp(-x^2); sign 2*(x>=0)-1
//   utils/math.lua:305-312  norm_cdf = (erf(x/sqrt2) + 1) * 0.5       :293-300 norm_pdf = exp(-x^2/2)/sqrt(2pi)
//   scores/expected_improvement.lua:69-88  sigma = sqrt(var); imprv = (fmin - mu) - xi; z = imprv/sigma;
//                                          ei = clamp(imprv*Phi(z) + sigma*phi(z), 0, inf); row mean if c > 1
//   scores/confidence_bound.lua:70-106     LCB = mu - sqrt(var)*k, UCB = mu + sqrt(var)*k; sign flip (:89-93)
//   bots/bayesopt.lua:69-79                score:add(...) per hyper sample, score:div(nSamples)
//   bots/bayesopt.lua:96                   score:max(1): first maximum, first NaN wins (TH max)
// exp/sqrt/division are the correctly-rounded-or-1-ulp ocml double routines; everything else is exact IEEE.
//
// Log-space expected improvement (B7_SCORE_LOGEI) has NO counterpart in the reference's scores/: it is EI evaluated so that it
// never underflows (Ament et al., "Unexpected Improvements to Expected Improvement", NeurIPS 2023).  With the same first three
// operations as EI -- sigma = sqrt(var); imprv = (fmin - mu) - xi; z = imprv/sigma -- and h(z) = phi(z) + z Phi(z):
//   logEI = log(sigma) + log h(z)
//   z >  -1:  log h = log(phi(z) + z * erfc(-z/sqrt2)/2)
//   z <= -1:  log h = -z^2/2 - log(2 pi)/2 + log1p(-t sqrt(pi/2) erfcx(t/sqrt2)),  t = -z
//   t >= 1e5: log h = -z^2/2 - log(2 pi)/2 + (-2 log t + log1p(-3/t^2))
// through ocml's fp64 erfc, erfcx, log1p, log and exp: no tables.  The last line is the far tail of the one above it:
// r = t sqrt(pi/2) erfcx(t/sqrt2) = 1 - 1/t^2 + 3/t^4 - 15/t^6 + ..., so log(1 - r) = -2 log t + log1p(-3/t^2 + 15/t^4 - ...); at
// t >= 1e5 the dropped 15/t^4 is below 1.5e-19, far under an ulp of 2 log t.  It is there because r is within half an ulp of 1 from
// t ~ 3e7 and the roundings of its three multiplications then put it ABOVE 1 about as often as at it: log1p(-r) would be NaN for a
// finite input, and TH's max lets the first NaN win.  Below 1e5, 1 - r >= 1e-10 and r < 1 by a wide margin.  With the tail, log EI
// is finite and ordered down to t ~ 1.3e154, where z^2/2 overflows and the score is -inf.  Edge cases, beside EI's
// (EI: var NaN or < 0 -> NaN; var == 0 -> z = +-inf or NaN and the sum follows IEEE):
//   var NaN or var < 0        NaN (sigma is NaN)            mu NaN                NaN
//   var == 0, imprv > 0       log(imprv)                    var == 0, imprv <= 0  -inf
//   z = +inf (sigma > 0)      log(imprv)                    z = -inf              -inf
// A finite (mu, var, fmin, xi) with var >= 0 never scores NaN.
// Marginalisation is log((1/S) sum_s EI_s), not the mean of the logs: the accumulator of LogEI is a running log-sum-exp, empty at
// -inf, folded by a <- logaddexp(a, v) = max + log1p(exp(min - max)) in sample order (NaN if either is NaN, -inf / +inf when both are);
// c > 1 response columns are the same fold over the columns of a row, then - log(c); score:div becomes a - log(divisor), the
// log taken here.
//
// Max-value entropy search (B7_SCORE_MES) has NO counterpart in the reference's scores/ either (Wang & Jegelka, "Max-value Entropy
// Search for Efficient Bayesian Optimization", ICML 2017).  The library minimises, so the paper's maximum is the MINIMUM y*: with
// K quantiles y*_k of the grid minimum's distribution under a hyper sample (mes.hip finds them; they arrive as ScoreParams::ystar),
//   g_k = (mu - y*_k)/sigma,   h(g) = g phi(g)/(2 Phi(g)) - log Phi(g),   score = (1/K) sum_k h(g_k)        (mes_math.h)
// fmin, tradeoff, upper and sign are ignored; the accumulator is linear, as EI's, each sample with its own K values.  Row classes:
//   bad    mu or var NaN, or var < 0     NaN (the first NaN wins the arg-max, as everywhere)
//   exact  var == 0                      exactly 0.0 (nothing is left to learn there)
// A y* found by the search keeps g >= -Phi^-1(1 - 1/(2K)) >= -2.5; with a caller's y* (b7_mes_compute) the accuracy bar holds for
// g >= -8 and the value stays finite below.
//
// Log probability of improvement (B7_SCORE_LOGPI) has NO counterpart in the reference's scores/ either.  With EI's first three
// operations -- sigma = sqrt(var); imprv = (fmin - mu) - xi; z = imprv/sigma -- the value is log Phi(z), evaluated so that it neither
// underflows nor loses the upper tail (ocml's fp64 erfc, erfcx, log1p and log):
//   z >= 0:       log1p(-erfc(z/sqrt2)/2)
//   -1 < z < 0:   log(erfc(-z/sqrt2)/2)
//   z <= -1:      (-z^2/2 - log 2) + log(erfcx(-z/sqrt2))
// On a constraint's GP, with fmin = the threshold t_k and xi = 0, it is log Pr[c_k(x) <= t_k]: the log probability of feasibility of
// Gelbart et al. 2014 / Gardner et al. 2014 in the log-space form of Ament et al. 2023.  The accumulator is the log one, as LogEI's:
// the marginal is log((1/S) sum_s Phi(z_s)); c > 1 response columns fold as LogEI's do.  Row classes:
//   var NaN or var < 0        NaN (sigma is NaN)            mu NaN                NaN
//   var == 0, imprv >= 0      0.0                           var == 0, imprv < 0   -inf
//   z = +inf (sigma > 0)      0.0                           z = -inf              -inf
// A finite (mu, var, fmin, xi) with var >= 0 never scores NaN.  Beyond |z| ~ 1.3e154, z^2/2 overflows and the value is -inf.
// Relative accuracy is not promised where |log Phi| < 1e-300 (z beyond ~37: erfc has underflowed, the value is -0.0).
//
// The feasibility column (b7_feas_*, b7_eval_nominate_feasible): a per-context vector L[M] of log-weights over the resident grid.
// Between score:div and score:max(1) each row's score v becomes w(v, L[j]):
//   log accumulator (LogEI, LogPI)   w = v + L            linear accumulator (EI)   w = v * exp(L)
//   either operand NaN: NaN.  Otherwise L = -inf: -inf / 0.0 whatever v is, so that +inf - inf and inf * 0 are never formed for a
//   masked row.  (A FINITE L whose exp underflows against v = +inf, or L = +inf against v = -inf, follow IEEE: NaN.)
// score_finish_slot_feas_kernel is score_finish_slot_kernel with that one step ahead of the block reduction (the pending route of
// the small regime stays one launch); feas_finish_kernel is finish_kernel with it (the routes whose score has already been added).
// L is read, never written, by both.  That two contexts whose columns are combined (b7_feas_add_acc) hold the same grid rows is the
// caller's contract: only the row COUNT can be checked.
//
// Every score kind is written ONCE, as the per-kind pieces below (hoist / value / row_sign over the accumulator algebra empty / fold /
// div); the per-sample kernel, the S-batch kernel and the fused nomination kernel are templates over the kind that only arrange
// those pieces, which is what makes the one-call nomination equal the per-sample loop bit for bit.
#pragma clang fp contract(off)
#include <type_traits>

#include "b7_internal.h"
#include "logei_math.h"
#include "mes_math.h"

namespace {

__device__ __forceinline__ double b7_erf(double x) {
  const double c1 = 0.254829592, c2 = -0.284496736, c3 = 1.421413741, c4 = -1.453152027, c5 = 1.061405429,
               p = 0.3275911;
  double t = 1.0 / ((fabs(x) * p) + 1.0);
  double r = t * c5;
  r = r + c4;
  r = r * t;
  r = r + c3;
  r = r * t;
  r = r + c2;
  r = r * t;
  r = r + c1;
  r = r * t;
  double e = exp((x * x) * -1.0);
  r = ((r * e) * -1.0) + 1.0;
  double s = ((x >= 0.0) ? 1.0 : 0.0) * 2.0 + -1.0;
  return r * s;
}
__device__ __forceinline__ double b7_norm_cdf(double z) {
  double u = z * 0.70710678118654746;  // 1/math.sqrt(2), utils/math.lua:13
  return (b7_erf(u) + 1.0) * 0.5;
}
__device__ __forceinline__ double b7_norm_pdf(double z) {
  return exp((z * z) * -0.5) * 0.3989422804014327;  // 1/math.sqrt(2*math.pi), utils/math.lua:15
}

// (log-space EI and the log-sum-exp step, b7_logei / b7_logaddexp: logei_math.h, shared with ehvi_math.h)
// ---- log probability of improvement (see the header) ----
__device__ __forceinline__ double b7_logpi(double mu, double var, double fmin, double xi) {
  const double sigma = sqrt(var);
  const double imprv = (fmin + (-mu)) + (-xi);
  const double z = imprv / sigma;
  if (sigma == 0.0) return (imprv >= 0.0) ? 0.0 : ((imprv != imprv) ? imprv : -INFINITY);
  if (z == INFINITY) return 0.0;
  if (z == -INFINITY) return -INFINITY;
  if (z >= 0.0) return log1p(erfc(z * 0.70710678118654752440) * -0.5);  // 1 - Phi(z) = erfc(z/sqrt2)/2
  if (z > -1.0) return log(erfc(z * -0.70710678118654752440) * 0.5);    // Phi(z) = erfc(-z/sqrt2)/2
  // z <= -1; NaN comes this way too, and stays NaN
  return (((z * z) * -0.5) + -0.69314718055994530942) + log(erfcx(z * -0.70710678118654752440));
}
// ---- the feasibility weight (see the header): v = a row's score after score:div, L = its log-weight ----
template <bool LOG>
__device__ __forceinline__ double feas_weight(double v, double L) {
  if (v != v || L != L) return v + L;
  if (L == -INFINITY) return LOG ? -INFINITY : 0.0;
  if constexpr (LOG) return v + L;
  else return v * exp(L);
}
// ---- max-value entropy search (see the header): y = the sample's nlev quantiles of the grid minimum ----
__device__ __forceinline__ double b7_mes(double mu, double var, const double *__restrict__ y, int nlev) {
  if (!(var >= 0.0) || mu != mu) return NAN;
  if (var == 0.0) return 0.0;
  const double sigma = sqrt(var);
  double a = 0.0;
  for (int k = 0; k < nlev; ++k) a = a + b7_mes_h((mu + (-y[k])) / sigma);
  return a / (double)nlev;
}
// ---- a score kind K (B7_SCORE_*), once.  The accumulator algebra follows score_acc_kind(K): a linear sum or a log-sum-exp ----
template <int K>
__device__ __forceinline__ double empty() {  // torch.zeros (bots/bayesopt.lua:69); log: the empty log-sum-exp
  if constexpr (score_acc_kind(K) == B7_ACC_LOG) return -INFINITY;
  else return 0.0;
}
template <int K>
__device__ __forceinline__ double fold(double a, double v) {  // score:add, and the sum over the columns of a row
  if constexpr (score_acc_kind(K) == B7_ACC_LOG) return b7_logaddexp(a, v);
  else return a + v;
}
template <int K>
__device__ __forceinline__ double div(double a, double divisor) {  // score:div, and the row mean
  if constexpr (score_acc_kind(K) == B7_ACC_LOG) return a + (-log(divisor));
  else return a / divisor;
}
// what a candidate's variance contributes to every response column: sigma (EI), sqrt(var) * kappa (CB), the variance itself (LogEI,
// LogPI, MES)
template <int K>
__device__ __forceinline__ double hoist(double var, const ScoreParams &p) {
  if constexpr (K == B7_SCORE_EI) return sqrt(var);
  else if constexpr (K == B7_SCORE_CB) return sqrt(var) * p.tradeoff;
  else return var;
}
// one candidate, one response column of hyper sample s; h = hoist<K>(var)
template <int K>
__device__ __forceinline__ double value(double mu, double h, double fmin, const ScoreParams &p, int s) {
  if constexpr (K == B7_SCORE_EI) {
    double imprv = (fmin + (-mu)) + (-p.tradeoff);
    double z = imprv / h;
    double ei = (imprv * b7_norm_cdf(z)) + (h * b7_norm_pdf(z));
    return (ei < 0.0) ? 0.0 : ei;
  } else if constexpr (K == B7_SCORE_CB) {
    return p.upper ? (mu + h) : (mu + (-h));
  } else if constexpr (K == B7_SCORE_MES) {
    return b7_mes(mu, h, p.ystar + (long long)s * p.nlev, p.nlev);
  } else if constexpr (K == B7_SCORE_LOGPI) {
    return b7_logpi(mu, h, fmin, p.tradeoff);
  } else {
    return b7_logei(mu, h, fmin, p.tradeoff);
  }
}
// the sign flip of the confidence bound (scores/confidence_bound.lua:89-93), applied to a row's score: after the row mean
template <int K>
__device__ __forceinline__ double row_sign(double v, const ScoreParams &p) {
  if constexpr (K == B7_SCORE_CB) return (p.sign > 0.0) ? v : -v;
  else return v;
}
__device__ __forceinline__ double fmin_of(const ScoreParams &p, int k) {  // fmin == nullptr: one column, its f_min a kernel argument
  return p.fmin ? p.fmin[k] : p.fmin0;
}
// the score's derivatives at one candidate of one hyper sample, for b7_eval_nominate_refine (nothing else instantiates it):
// cm = dv/dmu and cs = dv/dsigma of row_sign(value<K>), so that grad v = cm grad mu + cs grad sigma, grad sigma = grad var / (2 sigma).
//   EI     -Phi(z), phi(z) with the score's own A&S Phi and phi: the exact-EI formula; it proposes directions, decisions are on values
//   CB     the row sign times (1, +-kappa), following value<CB>
//   LogEI  -(Phi/h)/sigma, (phi/h)/sigma, h = phi + z Phi; Phi/phi = sqrt(pi/2) erfcx(-z/sqrt2) (no exponential),
//          phi/h = 1/(1 + z Phi/phi), Phi/h = (Phi/phi)(phi/h); for z >= 0 the same two through phi/Phi, which stays finite
template <int K>
__device__ __forceinline__ void grad(double mu, double var, double fmin, const ScoreParams &p, double *cm, double *cs) {
  if constexpr (K == B7_SCORE_EI) {
    const double h = sqrt(var);
    const double z = ((fmin + (-mu)) + (-p.tradeoff)) / h;
    *cm = -b7_norm_cdf(z), *cs = b7_norm_pdf(z);
  } else if constexpr (K == B7_SCORE_CB) {
    const double sg = (p.sign > 0.0) ? 1.0 : -1.0;
    *cm = sg, *cs = sg * (p.upper ? p.tradeoff : -p.tradeoff);
  } else {
    static_assert(K == B7_SCORE_LOGEI, "grad<K>: EI, CB and LogEI have a gradient piece");
    const double sigma = sqrt(var);
    const double z = ((fmin + (-mu)) + (-p.tradeoff)) / sigma;
    const double R = 1.2533141373155002512 * erfcx(z * -0.70710678118654752440);  // Phi(z) / phi(z)
    double ph, Ph;                                                                // phi / h, Phi / h
    if (z < 0.0) {
      ph = 1.0 / (1.0 + (z * R));
      Ph = R * ph;
    } else {
      const double iR = 1.0 / R, den = z + iR;
      Ph = 1.0 / den;
      ph = iR / den;
    }
    *cm = -(Ph / sigma), *cs = ph / sigma;
  }
}
// candidate j's marginal value over the S samples -- fold / div in sample order, the grid's accumulator -- and NC components of its
// gradient, c = sub, sub + 16, ..: the mean of the per-sample gradients for a linear accumulator, sum_s softmax_s grad v_s with the
// weights exp(v_s - logsumexp) for LogEI.  mu / var: [S][M1], dmu / dvar: [S][M1][d].
// SIXTEEN threads serve a candidate (sub = 0 .. 15) and EVERY thread of the block calls: the samples go through in chunks of 16, a
// thread evaluating ONE sample's value<K> / grad<K> -- the transcendental work, done once per sample -- into the candidate's LDS
// slots sc[16][4] (v or weight | dv/dmu | dv/dsigma | 2 sigma); between two barriers every thread then adds the chunk onto its own
// gradient components in sample order.  LogEI: thread 0 of the candidate folds the log-sum-exp (into *sa), a second pass makes the
// weights.  The sums are those of a loop over s on one thread, in the same order.
template <int K, int NC>
__device__ __forceinline__ double marg_value_grad(const ScoreParams &p, const double *__restrict__ mu, const double *__restrict__ var,
                                                  const double *__restrict__ dmu, const double *__restrict__ dvar, long long M1,
                                                  long long j, int d, int sub, double (*sc)[4], double *sa, double (&G)[NC]) {
  constexpr bool LOG = score_acc_kind(K) == B7_ACC_LOG;
  const double fmin = fmin_of(p, 0);
  double a = empty<K>();
#pragma unroll
  for (int i = 0; i < NC; ++i) G[i] = 0.0;
  for (int pass = 0; pass < (LOG ? 2 : 1); ++pass) {
    for (int s0 = 0; s0 < p.S; s0 += 16) {
      const int s = s0 + sub, ns = (p.S - s0 < 16) ? p.S - s0 : 16;
      if (s < p.S) {
        const double m = mu[s * M1 + j], vr = var[s * M1 + j];
        const double v = row_sign<K>(value<K>(m, hoist<K>(vr, p), fmin, p, s), p);
        sc[sub][0] = (LOG && pass == 1) ? exp(v + (-a)) : v;
        if (!LOG || pass == 1) {
          double cm, cs;
          grad<K>(m, vr, fmin, p, &cm, &cs);
          sc[sub][1] = cm, sc[sub][2] = cs, sc[sub][3] = 2.0 * sqrt(vr);
        }
      }
      __syncthreads();
      if (!LOG) {
        for (int i = 0; i < ns; ++i) a = fold<K>(a, sc[i][0]);
      } else if (pass == 0 && sub == 0) {
        for (int i = 0; i < ns; ++i) a = fold<K>(a, sc[i][0]);
      }
      if (!LOG || pass == 1) {
        for (int i = 0; i < ns; ++i) {
          const double cm = sc[i][1], cs = sc[i][2], s2 = sc[i][3];
          const long long row = ((s0 + i) * M1 + j) * d;
#pragma unroll
          for (int e = 0; e < NC; ++e) {
            const int c = sub + 16 * e;
            if (c < d) {
              const double t = (cm * dmu[row + c]) + (cs * (dvar[row + c] / s2));
              G[e] = G[e] + (LOG ? sc[i][0] * t : t);
            }
          }
        }
      }
      __syncthreads();
    }
    if (LOG && pass == 0) {  // the log-sum-exp to every thread of the candidate
      if (sub == 0) *sa = a;
      __syncthreads();
      a = *sa;
    }
  }
  if (!LOG) {
#pragma unroll
    for (int i = 0; i < NC; ++i) G[i] = G[i] / (double)p.S;
  }
  return div<K>(a, (double)p.S);
}
constexpr int GRAD_NC = B7_MAX_D / 16;  // gradient components per thread: 16 threads to a candidate

// b7_score_grad_compute: 16 candidates per block, 16 threads each
template <int K>
__global__ void __launch_bounds__(256) score_grad_kernel(ScoreParams p, const double *__restrict__ mu, const double *__restrict__ var,
                                                         const double *__restrict__ dmu, const double *__restrict__ dvar, long long M1,
                                                         int d, double *__restrict__ value_out, double *__restrict__ grad_out) {
  __shared__ double sc[16][16][4], sa[16];
  const int r = threadIdx.x >> 4, sub = threadIdx.x & 15;
  const long long jj = (long long)blockIdx.x * 16 + r, j = (jj < M1) ? jj : M1 - 1;  // a row past the end repeats the last (no store)
  double G[GRAD_NC];
  const double v = marg_value_grad<K, GRAD_NC>(p, mu, var, dmu, dvar, M1, j, d, sub, sc[r], &sa[r], G);
  if (jj >= M1) return;
  if (sub == 0) value_out[j] = v;
#pragma unroll
  for (int i = 0; i < GRAD_NC; ++i)
    if (sub + 16 * i < d) grad_out[j * d + sub + 16 * i] = G[i];
}

// One iteration of b7_eval_nominate_refine after the posterior's launches: the marginal value and gradient of the 64 query columns
// (column = 4 start + rung), the ladder decision per start, the start's new state, its trace record and the next 64 query rows.
// One workgroup of 1024 threads = 64 columns x 16 (a sample's score pieces once per column, not once per thread); the only
// cross-thread traffic is LDS between barriers.
template <int K>
__global__ void __launch_bounds__(1024) refine_step_kernel(ScoreParams p, RefStep r) {
  __shared__ double sv[64];
  __shared__ double sx[B7_REFINE_MAX_STARTS][B7_MAX_D], sg[B7_REFINE_MAX_STARTS][B7_MAX_D];
  __shared__ double ssc[64][16][4], ssa[64];  // marg_value_grad's slots
  const int col = threadIdx.x >> 4, sub = threadIdx.x & 15, st = col >> 2, k = col & 3, d = r.d;
  double G[GRAD_NC];
  const double mv = marg_value_grad<K, GRAD_NC>(p, r.mu, r.var, r.dmu, r.dvar, 64, col, d, sub, ssc[col], &ssa[col], G);
  if (sub == 0) sv[col] = mv;
  // the start's state, read by every thread before any of them writes it
  double v = r.st->v[st];
  const double eta = r.st->eta[st];
  int status = r.st->status[st];
  const int active = r.st->active[st];
  __syncthreads();
  double cand[4] = {NAN, NAN, NAN, NAN}, eta_new = eta;
  int taken = -1;
  if (r.iter == 0) {
    taken = 0;  // the start itself
    v = sv[4 * st];
    if (!(status & B7_REFINE_NOT_RUN) && !(fabs(v) < INFINITY)) status |= B7_REFINE_NOT_RUN;
  } else if (active) {
    int kb = -1;
    double bv = 0.0;
    for (int q = 0; q < 4; ++q) {
      cand[q] = sv[4 * st + q];
      if (cand[q] == cand[q] && (kb < 0 || cand[q] > bv)) kb = q, bv = cand[q];  // the highest, the lowest rung on ties, never a NaN
    }
    if (kb >= 0 && bv > v) {
      const double tk = eta * (kb == 0 ? 1.0 : kb == 1 ? 0.25 : kb == 2 ? 0.0625 : 0.015625);
      taken = kb, v = bv, status |= B7_REFINE_MOVED;
      eta_new = (4.0 * tk < 1.0) ? 4.0 * tk : 1.0;
    } else {
      eta_new = eta / 256.0;
    }
    if (eta_new < 0x1p-40) status |= B7_REFINE_CONVERGED;
  }
  // the start's point and gradient after this iteration
  if (taken >= 0 ? k == taken : k == 0) {
#pragma unroll
    for (int i = 0; i < GRAD_NC; ++i) {
      const int c = sub + 16 * i;
      if (c < d) {
        sx[st][c] = (taken >= 0) ? r.xq[col * d + c] : r.st->x[st][c];
        sg[st][c] = (taken >= 0) ? G[i] : r.st->g[st][c];
      }
    }
  }
  __syncthreads();
  // the next ladder: g~ = grad o (hi - lo), m = max |g~|
  bool next = r.iter < r.iters && st < r.P && !(status & (B7_REFINE_NOT_RUN | B7_REFINE_CONVERGED));
  double m = 0.0;
  if (next) {
    bool bad = false;
    for (int c = 0; c < d; ++c) {
      const double a = fabs(sg[st][c] * (r.hi[c] + (-r.lo[c])));
      bad = bad || a != a;
      if (a > m) m = a;
    }
    if (bad || m == 0.0 || !(m < INFINITY)) status |= B7_REFINE_FLAT, next = false;
  }
  const double tk = eta_new * (k == 0 ? 1.0 : k == 1 ? 0.25 : k == 2 ? 0.0625 : 0.015625);
#pragma unroll
  for (int i = 0; i < GRAD_NC; ++i) {
    const int c = sub + 16 * i;
    if (c < d) {
      double x = sx[st][c];
      if (next) {
        const double b = r.hi[c] + (-r.lo[c]);
        const double rc = (sg[st][c] * b) / m;
        x = x + ((tk * rc) * b);
        x = (x > r.lo[c]) ? x : r.lo[c];
        x = (x < r.hi[c]) ? x : r.hi[c];
      }
      r.xq_next[col * d + c] = x;
    }
  }
  if (k != 0 || st >= r.P) return;
  double *rec = r.trace ? r.trace + ((long long)st * (r.iters + 1) + r.iter) * B7_REFINE_TRACE_WIDTH : nullptr;
#pragma unroll
  for (int i = 0; i < GRAD_NC; ++i) {
    const int c = sub + 16 * i;
    if (c < d) {
      r.st->x[st][c] = sx[st][c];
      r.st->g[st][c] = sg[st][c];
      if (rec) rec[c] = sx[st][c], rec[d + 1 + c] = sg[st][c];
    }
  }
  if (sub == 0) {
    r.st->v[st] = v;
    r.st->eta[st] = eta_new;
    r.st->status[st] = status;
    r.st->active[st] = next ? 1 : 0;
    if (rec) {
      rec[d] = v;
      rec[2 * d + 1] = eta;
      for (int q = 0; q < 4; ++q) rec[2 * d + 2 + q] = cand[q];
      rec[2 * d + 6] = (r.iter == 0) ? -1.0 : (double)taken;
      rec[2 * d + 7] = (double)status;
    }
  }
}

// The score of ONE hyper sample (p.S == 1) over c response columns, the row mean if c > 1.  accumulate 0 writes it, 1 folds it
// onto out, 2 folds it onto an empty accumulator that is not read: the first score:add onto torch.zeros (0.0 + v, not v)
template <int K>
__global__ void __launch_bounds__(256) score_kernel(ScoreParams p, int64_t M, int c, double *__restrict__ out, int accumulate) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    const double h = hoist<K>(p.var[j], p);
    double row;
    if (c == 1) {
      row = value<K>(p.mu[j], h, fmin_of(p, 0), p, 0);
    } else {
      row = empty<K>();
      for (int k = 0; k < c; ++k) row = fold<K>(row, value<K>(p.mu[j * c + k], h, fmin_of(p, k), p, 0));
      row = div<K>(row, (double)c);
    }
    row = row_sign<K>(row, p);
    out[j] = accumulate == 1 ? fold<K>(out[j], row) : (accumulate == 2 ? fold<K>(empty<K>(), row) : row);
  }
}

// S hyper samples of candidate j (one response column) folded onto a in sample order: a = fold(..fold(fold(a, s_0), s_1).., s_S-1),
// exactly what S score:add calls leave (bots/bayesopt.lua:76)
template <int K>
__device__ __forceinline__ double fold_samples(const ScoreParams &p, int64_t j, double a) {
  for (int s = 0; s < p.S; ++s) {
    const double m = p.mu[s * p.stride + j], h = hoist<K>(p.var[s * p.stride + j], p);
    a = fold<K>(a, row_sign<K>(value<K>(m, h, fmin_of(p, 0), p, s), p));
  }
  return a;
}
// fresh: the accumulator is torch.zeros (bots/bayesopt.lua:69; log: an empty log-sum-exp), not read
template <int K>
__global__ void __launch_bounds__(256) score_batch_kernel(ScoreParams p, int64_t M, double *__restrict__ out, int fresh) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride)
    out[j] = fold_samples<K>(p, j, fresh ? empty<K>() : out[j]);
}

__global__ void __launch_bounds__(256) fill_kernel(double *__restrict__ p, int64_t n, double v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) p[j] = v;
}

// (value, index) ordering of TH's max: the first NaN wins; otherwise the larger value; ties -> lower index (argbest.h).
using Better = OrderMaxNanFirst;  // Better()(a, b): is a strictly preferred to b

// acc[j] /= divisor (score:div; a log accumulator: acc[j] -= log(divisor)), then per-block best.
__global__ void __launch_bounds__(256)
    finish_kernel(double *__restrict__ acc, int64_t M, double divisor, ArgBest *__restrict__ part, int logacc) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    double v = logacc ? acc[j] + (-log(divisor)) : acc[j] / divisor;
    acc[j] = v;
    ArgBest cnd{v, j};
    if (Better()(cnd, b)) b = cnd;
  }
  b = block_best<Better>(b, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ void __launch_bounds__(256) argmax_final_kernel(const ArgBest *__restrict__ part, int n, ArgBest *__restrict__ out) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  for (int j = threadIdx.x; j < n; j += blockDim.x)
    if (Better()(part[j], b)) b = part[j];
  b = block_best<Better>(b, sh);
  if (threadIdx.x == 0) out[0] = b;
}

// The global-exchange form of argmax_final_kernel: this rank's record of the exchange table (b7_internal.h: value bits,
// 1-based GLOBAL index, status 0, shard rows, the winner's grid row).  With all_slots the records of every other rank are
// zeroed as well (comm.hip sums the tables of all ranks); a single-process group merges records on the host and needs
// only this one.
// this rank's record (and, with all_slots, zeros for every other rank's) from the local best b; every thread of the block calls
__device__ __forceinline__ void write_record(ArgBest b, unsigned long long *__restrict__ tab, int rank, int world, long long offset,
                                             long long rows, const double *__restrict__ grid, int d, int all_slots,
                                             unsigned long long *__restrict__ host_rec, unsigned *__restrict__ host_done) {
  if (all_slots)
    for (int e = threadIdx.x; e < world * B7_TAB_W; e += blockDim.x)
      if (e / B7_TAB_W != rank) tab[e] = 0ull;
  unsigned long long *rec = tab + (size_t)rank * B7_TAB_W;
  const bool have = b.i >= 0;
  for (int e = threadIdx.x; e < B7_TAB_W; e += blockDim.x) {
    unsigned long long w = 0ull;
    if (e == B7_TAB_VAL) w = have ? (unsigned long long)__double_as_longlong(b.v) : 0ull;
    else if (e == B7_TAB_IDX) w = have ? (unsigned long long)(offset + b.i + 1) : 0ull;
    else if (e == B7_TAB_ROWS) w = (unsigned long long)rows;
    else if (e >= B7_TAB_ROW0 && e - B7_TAB_ROW0 < d && have && grid)
      w = (unsigned long long)__double_as_longlong(grid[b.i * d + (e - B7_TAB_ROW0)]);
    rec[e] = w;
    if (host_rec) host_rec[e] = w;  // the same record straight into mapped host memory: no copy launch behind this kernel
  }
  if (host_done) {
    // the host spins on this word instead of waiting for the stream: every thread's part of the record is pushed out to
    // system scope before the barrier, thread 0's release store comes after it
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(host_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void __launch_bounds__(256) argmax_slot_kernel(const ArgBest *__restrict__ part, int n, unsigned long long *__restrict__ tab,
                                                          int rank, int world, long long offset, long long rows,
                                                          const double *__restrict__ grid, int d, int all_slots,
                                                          long long forced_local, unsigned long long *__restrict__ host_rec,
                                                          unsigned *__restrict__ host_done) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  if (n > 0) {
    for (int j = threadIdx.x; j < n; j += blockDim.x)
      if (Better()(part[j], b)) b = part[j];
    b = block_best<Better>(b, sh);
  } else if (forced_local >= 0) {  // no scores: the record names a given row (b7_nominate_commit's broadcast)
    b = ArgBest{0.0, forced_local};
  }
  write_record(b, tab, rank, world, offset, rows, grid, d, all_slots, host_rec, host_done);
}

// The tail of the fused nomination kernel: per-block best, and the LAST block to arrive (a ticket from one atomic counter; every
// block's partial is fenced before its ticket) reduces the partials and writes the record.
// Every thread of the block calls; sh: 4 ArgBest, last: one word, both in LDS.
__device__ __forceinline__ void block_best_ticket_record(ArgBest b, ArgBest *sh, unsigned *last, ArgBest *__restrict__ part,
                                                         unsigned *__restrict__ ticket, unsigned long long *__restrict__ tab, int rank,
                                                         int world, long long offset, long long M, const double *__restrict__ grid, int d,
                                                         int all_slots, unsigned long long *__restrict__ host_rec,
                                                         unsigned *__restrict__ host_done) {
  b = block_best<Better>(b, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = b;
    __threadfence();  // the partial is visible device-wide before the ticket is taken
    const unsigned t = atomicAdd(ticket, 1u);
    *last = (t == gridDim.x - 1) ? 1u : 0u;
  }
  __syncthreads();
  if (!*last) return;
  __threadfence();  // the other blocks' partials, published before their tickets
  ArgBest f{0.0, -1};
  for (int j = threadIdx.x; j < (int)gridDim.x; j += blockDim.x) {
    ArgBest pj;  // agent-scope loads: the partials of other CUs, not a stale line of this CU's cache
    pj.v = __hip_atomic_load(&part[j].v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pj.i = __hip_atomic_load(&part[j].i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (Better()(pj, f)) f = pj;
  }
  __syncthreads();
  f = block_best<Better>(f, sh);
  if (threadIdx.x == 0) *ticket = 0u;  // ready for the next launch (stream order: nobody else touches it meanwhile)
  write_record(f, tab, rank, world, offset, M, grid, d, all_slots, host_rec, host_done);
}

// score:add over the S hyper samples of a nomination, score:div, score:max(1) and this rank's exchange record in ONE launch
// (bots/bayesopt.lua:76-79, :96): score_batch_kernel + finish_kernel + argmax_slot_kernel, the same operations in the same order
// per candidate -- fold_samples onto the accumulator, div by the divisor -- then the tail above.  Three dependent launches at the
// ~4.5 us dispatch floor each become one.  (One kernel per kind: ocml's erfcx / log1p / log give the LogEI instance three times the
// registers of the EI and CB ones.)
template <int K>
__global__ void __launch_bounds__(256)
    score_finish_slot_kernel(ScoreParams p, int fresh, double *__restrict__ acc, long long M, double divisor, ArgBest *__restrict__ part,
                             unsigned *__restrict__ ticket, unsigned long long *__restrict__ tab, int rank, int world, long long offset,
                             const double *__restrict__ grid, int d, int all_slots, unsigned long long *__restrict__ host_rec,
                             unsigned *__restrict__ host_done) {
  __shared__ ArgBest sh[4];
  __shared__ unsigned last;
  ArgBest b{0.0, -1};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    const double v = div<K>(fold_samples<K>(p, j, fresh ? empty<K>() : acc[j]), divisor);
    acc[j] = v;
    ArgBest cnd{v, j};
    if (Better()(cnd, b)) b = cnd;
  }
  block_best_ticket_record(b, sh, &last, part, ticket, tab, rank, world, offset, M, grid, d, all_slots, host_rec, host_done);
}

// The same with rows left out of the arg-max (b7_eval_nominate_batch: the rows already picked).  Their score is computed and
// written like any other; only the candidate for the block reduction is withheld, so a NaN there does not win.
template <int K>
__global__ void __launch_bounds__(256)
    score_finish_slot_excl_kernel(ScoreParams p, int fresh, double *__restrict__ acc, long long M, double divisor, ArgBest *__restrict__ part,
                                  unsigned *__restrict__ ticket, unsigned long long *__restrict__ tab, int rank, int world,
                                  long long offset, const double *__restrict__ grid, int d, int all_slots,
                                  unsigned long long *__restrict__ host_rec, unsigned *__restrict__ host_done, ExclRows excl) {
  __shared__ ArgBest sh[4];
  __shared__ unsigned last;
  ArgBest b{0.0, -1};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    const double v = div<K>(fold_samples<K>(p, j, fresh ? empty<K>() : acc[j]), divisor);
    acc[j] = v;
    bool out = false;
    for (int e = 0; e < excl.n; ++e) out = out || excl.row[e] == j;
    ArgBest cnd{v, j};
    if (!out && Better()(cnd, b)) b = cnd;
  }
  block_best_ticket_record(b, sh, &last, part, ticket, tab, rank, world, offset, M, grid, d, all_slots, host_rec, host_done);
}

// The same with the feasibility column weighted in ahead of the block reduction (b7_eval_nominate_feasible): the row's score after
// score:div becomes w(v, feas[j]) (see the header), and that is what the accumulator holds and the arg-max sees.
template <int K>
__global__ void __launch_bounds__(256)
    score_finish_slot_feas_kernel(ScoreParams p, int fresh, double *__restrict__ acc, long long M, double divisor, ArgBest *__restrict__ part,
                                  unsigned *__restrict__ ticket, unsigned long long *__restrict__ tab, int rank, int world,
                                  long long offset, const double *__restrict__ grid, int d, int all_slots,
                                  unsigned long long *__restrict__ host_rec, unsigned *__restrict__ host_done,
                                  const double *__restrict__ feas) {
  __shared__ ArgBest sh[4];
  __shared__ unsigned last;
  ArgBest b{0.0, -1};
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    const double v = div<K>(fold_samples<K>(p, j, fresh ? empty<K>() : acc[j]), divisor);
    const double w = feas_weight<score_acc_kind(K) == B7_ACC_LOG>(v, feas[j]);
    acc[j] = w;
    ArgBest cnd{w, j};
    if (Better()(cnd, b)) b = cnd;
  }
  block_best_ticket_record(b, sh, &last, part, ticket, tab, rank, world, offset, M, grid, d, all_slots, host_rec, host_done);
}

// finish_kernel with the feasibility column: acc[j] <- w(acc[j] / divisor, feas[j]) (a log accumulator: - log(divisor)), then the
// per-block best; argmax_slot_kernel follows, a launch boundary away.
__global__ void __launch_bounds__(256) feas_finish_kernel(double *__restrict__ acc, const double *__restrict__ feas, int64_t M,
                                                          double divisor, ArgBest *__restrict__ part, int logacc) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    const double v = logacc ? acc[j] + (-log(divisor)) : acc[j] / divisor;
    const double w = logacc ? feas_weight<true>(v, feas[j]) : feas_weight<false>(v, feas[j]);
    acc[j] = w;
    ArgBest cnd{w, j};
    if (Better()(cnd, b)) b = cnd;
  }
  b = block_best<Better>(b, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

// the column's own kernels: L[j] += src[j] (b7_feas_add, b7_feas_add_acc) and the per-block best of L, which is only read
// (b7_feas_nominate; argmax_final_kernel follows)
__global__ void __launch_bounds__(256) feas_add_kernel(double *__restrict__ L, const double *__restrict__ src, int64_t M) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) L[j] = L[j] + src[j];
}
__global__ void __launch_bounds__(256) feas_best_kernel(const double *__restrict__ L, int64_t M, ArgBest *__restrict__ part) {
  __shared__ ArgBest sh[4];
  ArgBest b{0.0, -1};
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < M; j += stride) {
    ArgBest cnd{L[j], j};
    if (Better()(cnd, b)) b = cnd;
  }
  b = block_best<Better>(b, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ void __launch_bounds__(256) keep_record_kernel(unsigned long long *__restrict__ tab, int rank, int world) {
  for (int e = threadIdx.x; e < world * B7_TAB_W; e += blockDim.x)
    if (e / B7_TAB_W != rank) tab[e] = 0ull;
}

int nblocks(b7_ctx *c, int64_t n) {
  int64_t b = (n + 255) / 256, cap = (int64_t)c->cus * 8;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

// 0: out = score; 1: out += score; 2: out = 0.0 + score -- the context's accumulator was declared torch.zeros without being
// filled (b7_eval_nominate: bots/bayesopt.lua:69 costs no launch of its own) and this is the first score:add onto it.  A score
// written (not added) onto the accumulator is the accumulator from then on (bots/bayesopt.lua:65-66: the DNGO branch)
// kind: what this launch adds, a linear sum (EI, CB) or a log-sum-exp (LogEI).  The first add after a reset decides what the
// accumulator holds -- a log one then starts from -inf whatever the reset wrote --; adding the other kind onto it is -1 (the
// launchers answer B7_ERR_STATE through acc_mode_or_fail)
static int acc_mode(b7_ctx *c, const double *out, bool accumulate, int kind = B7_ACC_LINEAR) {
  if (out != (const double *)c->acc.p) return accumulate ? 1 : 0;
  if (accumulate && c->acc_kind != B7_ACC_NONE && c->acc_kind != kind) return -1;
  const bool fresh = c->acc_fresh || (accumulate && kind == B7_ACC_LOG && c->acc_kind == B7_ACC_NONE);
  c->acc_fresh = false;
  c->acc_kind = kind;
  if (!accumulate) c->acc_valid = true;
  return accumulate ? (fresh ? 2 : 1) : 0;
}
static int acc_mode_or_fail(b7_ctx *c, const double *out, bool accumulate, int kind, int *mode) {
  *mode = acc_mode(c, out, accumulate, kind);
  if (*mode < 0)
    return b7_fail(c, B7_ERR_STATE, "score: the accumulator holds a %s; a %s cannot be added onto it (b7_score_reset first)",
                   c->acc_kind == B7_ACC_LOG ? "log-sum-exp (LogEI / LogPI)" : "linear sum (EI / CB)",
                   kind == B7_ACC_LOG ? "log score" : "linear score");
  return B7_OK;
}

// THE step from a run-time score kind to its template instance: f(std::integral_constant<int, B7_SCORE_*>).  An unknown kind would
// run as CB: the entry points validate the kind (nominate_args, score_entry's fixed specs) before any launcher is reached
template <class F>
static void with_score_kind(int kind, F f) {
  switch (kind) {
    case B7_SCORE_EI: return f(std::integral_constant<int, B7_SCORE_EI>());
    case B7_SCORE_LOGEI: return f(std::integral_constant<int, B7_SCORE_LOGEI>());
    case B7_SCORE_MES: return f(std::integral_constant<int, B7_SCORE_MES>());
    case B7_SCORE_LOGPI: return f(std::integral_constant<int, B7_SCORE_LOGPI>());
    default: return f(std::integral_constant<int, B7_SCORE_CB>());  // (every launcher is reached only after nominate_args / its entry point has validated the kind)
  }
}

// one hyper sample: the score of mu (M x ycols) / var (M), written to out or added onto it
int launch_score(b7_ctx *c, ScoreParams p, const double *mu, const double *var, int64_t M, int ycols, double *out, bool accumulate) {
  PhaseScope ps(c, "score");
  if (M <= 0) return B7_OK;
  if (score_needs_fmin(p.kind) && !p.fmin && ycols != 1)
    return b7_fail(c, B7_ERR_INVALID, "%s: f_min of %d columns must be staged on the device", score_kind_name(p.kind), ycols);
  int mode;
  B7_TRY(acc_mode_or_fail(c, out, accumulate, score_acc_kind(p.kind), &mode));
  p.mu = mu, p.var = var, p.S = 1, p.stride = 0;
  with_score_kind(p.kind, [&](auto k) {
    hipLaunchKernelGGL(score_kernel<decltype(k)::value>, dim3(nblocks(c, M)), dim3(256), 0, c->stream, p, M, ycols, out, mode);
  });
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// the S hyper samples of p (one response column) added onto acc in sample order
int launch_score_batch(b7_ctx *c, const ScoreParams &p, double *acc, int64_t M) {
  PhaseScope ps(c, "score");
  if (M <= 0) return B7_OK;
  int mode;
  B7_TRY(acc_mode_or_fail(c, acc, true, score_acc_kind(p.kind), &mode));
  with_score_kind(p.kind, [&](auto k) {
    hipLaunchKernelGGL(score_batch_kernel<decltype(k)::value>, dim3(nblocks(c, M)), dim3(256), 0, c->stream, p, M, acc, mode == 2 ? 1 : 0);
  });
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_fill(b7_ctx *c, double *p, int64_t n, double v) {
  if (n <= 0) return B7_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(nblocks(c, n)), dim3(256), 0, c->stream, p, n, v);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// ---- the accumulator's state: set here and nowhere else ----
// torch.zeros(X_hid:size(1)), bots/bayesopt.lua:69, declared without a launch: the first score launch onto it starts from 0.0
// (score_kind: what the nomination will add.  LogEI: an empty log-sum-exp, -inf, declared the same way)
void acc_declare_zeros(b7_ctx *c, int score_kind) {
  c->acc_valid = true;
  c->acc_fresh = true;
  c->acc_kind = score_acc_kind(score_kind) == B7_ACC_LOG ? B7_ACC_LOG : B7_ACC_NONE;  // a linear one: the first add decides
}

// the same zeros written now (the caller has sized c->acc for c->M)
int acc_write_zeros(b7_ctx *c) {
  B7_TRY(launch_fill(c, (double *)c->acc.p, c->M, 0.0));
  c->acc_valid = true;
  c->acc_fresh = false;
  c->acc_kind = B7_ACC_NONE;  // the first add decides (acc_mode)
  return B7_OK;
}

// a finished log score is being written over every row of the accumulator (b7_logehvi_nominate, b7_logehvi3_nominate): what
// b7_score_finish and b7_feas_add_acc then find is a log accumulator with something in it
void acc_declare_log_written(b7_ctx *c) {
  c->acc_valid = true;
  c->acc_fresh = false;
  c->acc_kind = B7_ACC_LOG;
}

// the grid changed: there is no accumulator until the next reset or nomination
void acc_forget(b7_ctx *c) {
  c->acc_valid = false;
  c->acc_fresh = false;
  c->acc_kind = B7_ACC_NONE;
}

// zeros that were only declared and never met a score launch: written before anybody reads the accumulator (a declared log
// accumulator: -inf, the empty log-sum-exp)
int acc_materialize(b7_ctx *c) {
  if (!c->acc_fresh) return B7_OK;
  if (c->acc_kind != B7_ACC_LOG) return acc_write_zeros(c);
  B7_TRY(launch_fill(c, (double *)c->acc.p, c->M, -INFINITY));
  c->acc_fresh = false;
  return B7_OK;
}

// ---- the feasibility column's state: set here and nowhere else ----
void feas_forget(b7_ctx *c) { c->feas_valid = false; }

// L := 0.0 over the resident grid
int feas_write_zeros(b7_ctx *c) {
  B7_TRY(b7_ensure(c, c->feas, sizeof(double) * (size_t)c->M));
  B7_TRY(launch_fill(c, (double *)c->feas.p, c->M, 0.0));
  c->feas_valid = true;
  return B7_OK;
}

// L[j] += src[j], src a device vector of c->M doubles, on c's stream
int launch_feas_add(b7_ctx *c, const double *src) {
  PhaseScope ps(c, "feas");
  hipLaunchKernelGGL(feas_add_kernel, dim3(nblocks(c, c->M)), dim3(256), 0, c->stream, (double *)c->feas.p, src, (int64_t)c->M);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// score:max(1) of L alone; L is read only
int launch_feas_best(b7_ctx *c, double *best_val, int64_t *best_idx1) {
  PhaseScope ps(c, "argmax");
  const int nb = nblocks(c, c->M);
  B7_TRY(b7_ensure(c, c->part, sizeof(ArgBest) * (size_t)(nb + 1)));
  ArgBest *part = (ArgBest *)c->part.p;
  hipLaunchKernelGGL(feas_best_kernel, dim3(nb), dim3(256), 0, c->stream, (const double *)c->feas.p, (int64_t)c->M, part);
  ArgBest *res_dev = &c->pinned_dev->best;
  const ArgBest &h = c->pinned->best;
  hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(256), 0, c->stream, (const ArgBest *)part, nb, res_dev);
  B7_HIP(c, hipGetLastError());
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (best_val) *best_val = h.v;
  if (best_idx1) *best_idx1 = h.i + 1;
  return B7_OK;
}

int launch_finish(b7_ctx *c, double *acc, int64_t M, double divisor, double *best_val, int64_t *best_idx1, bool logacc) {
  PhaseScope ps(c, "argmax");
  if (M <= 0) return b7_fail(c, B7_ERR_INVALID, "finish: empty score vector");
  const int nb = nblocks(c, M);
  B7_TRY(b7_ensure(c, c->part, sizeof(ArgBest) * (size_t)(nb + 1)));
  ArgBest *part = (ArgBest *)c->part.p;
  hipLaunchKernelGGL(finish_kernel, dim3(nb), dim3(256), 0, c->stream, acc, M, divisor, part, logacc ? 1 : 0);
  // the final (value, index) goes straight into pinned, device-mapped host memory: no copy, just the synchronisation
  ArgBest *res_dev = &c->pinned_dev->best;
  const ArgBest &h = c->pinned->best;
  hipLaunchKernelGGL(argmax_final_kernel, dim3(1), dim3(256), 0, c->stream, (const ArgBest *)part, nb, res_dev);
  B7_HIP(c, hipGetLastError());
  B7_HIP(c, hipStreamSynchronize(c->stream));
  if (best_val) *best_val = h.v;
  if (best_idx1) *best_idx1 = h.i + 1;
  return B7_OK;
}

// launch_finish without the host round trip: the local result stays on the device, in this rank's record of the
// exchange table, together with the grid row it names.  M == 0 (an empty shard) writes an all-zero record.
// host_rec / host_done (nullable): device addresses of a mapped host copy of this rank's record and of the word the kernel
// sets once that copy is complete (comm.hip: exch_local with a mirror).
int launch_finish_slot(b7_ctx *c, double *acc, int64_t M, double divisor, uint64_t *tab_dev, int rank, int world,
                       int64_t offset, const double *grid, int d, bool all_slots, uint64_t *host_rec, unsigned *host_done,
                       bool logacc, const double *feas) {
  PhaseScope ps(c, "argmax");
  const int nb = M > 0 ? nblocks(c, M) : 0;
  B7_TRY(b7_ensure(c, c->part, sizeof(ArgBest) * (size_t)(nb + 1)));
  ArgBest *part = (ArgBest *)c->part.p;
  if (nb > 0 && feas)
    hipLaunchKernelGGL(feas_finish_kernel, dim3(nb), dim3(256), 0, c->stream, acc, feas, M, divisor, part, logacc ? 1 : 0);
  else if (nb > 0)
    hipLaunchKernelGGL(finish_kernel, dim3(nb), dim3(256), 0, c->stream, acc, M, divisor, part, logacc ? 1 : 0);
  hipLaunchKernelGGL(argmax_slot_kernel, dim3(1), dim3(256), 0, c->stream, (const ArgBest *)part, nb,
                     (unsigned long long *)tab_dev, rank, world, (long long)offset, (long long)M, grid, d, all_slots ? 1 : 0,
                     -1ll, (unsigned long long *)host_rec, host_done);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// The fused form: the S-sample score, score:div, the local arg-max and the record in one launch.
int launch_score_finish_slot(b7_ctx *c, const ScoreParams &p, double *acc, int64_t M, double divisor, uint64_t *tab_dev,
                             int rank, int world, int64_t offset, const double *grid, int d, bool all_slots, uint64_t *host_rec,
                             unsigned *host_done, const ExclRows *excl, const double *feas) {
  PhaseScope scope(c, "score");
  if (feas && (p.kind == B7_SCORE_CB || p.kind == B7_SCORE_MES || (excl && excl->n > 0)))
    return b7_fail(c, B7_ERR_UNSUPPORTED, "score: the feasibility weight is built for EI, LogEI and LogPI, without excluded rows");
  // (one-wave blocks for small grids -- 313 instead of 79 workgroups for 2e4 candidates -- measured SLOWER: 145 vs 139 us per
  // nomination at N = 100, S = 10; the last block's pass over four times as many partials costs more than the spread saves.
  // Likewise the S scores of a candidate on S threads side by side, parked in LDS and added in order by one of them, over 512
  // blocks: 137 vs 132 us.  The kernel's 15 us are launch, ticket and the last block's pass, not the ten scores in a row)
  const int threads = 256;
  const int nb = nblocks(c, M);
  B7_TRY(b7_ensure(c, c->part, sizeof(ArgBest) * (size_t)(nb + 1)));
  ArgBest *part = (ArgBest *)c->part.p;
  if (!c->ticket.p) {  // the ticket counter: a word of its own (c->part is shared scratch), zero between launches
    B7_TRY(b7_ensure(c, c->ticket, 64));
    B7_HIP(c, hipMemsetAsync(c->ticket.p, 0, 64, c->stream));
  }
  unsigned *ticket = (unsigned *)c->ticket.p;
  int mode;
  B7_TRY(acc_mode_or_fail(c, acc, true, score_acc_kind(p.kind), &mode));
  with_score_kind(p.kind, [&](auto k) {
    constexpr int K = decltype(k)::value;
    if constexpr (K == B7_SCORE_EI || K == B7_SCORE_LOGEI || K == B7_SCORE_LOGPI) {  // the kinds the weight has a form for
      if (feas) {
        hipLaunchKernelGGL(score_finish_slot_feas_kernel<K>, dim3(nb), dim3(threads), 0, c->stream, p, mode == 2 ? 1 : 0, acc, (long long)M,
                           divisor, part, ticket, (unsigned long long *)tab_dev, rank, world, (long long)offset, grid, d,
                           all_slots ? 1 : 0, (unsigned long long *)host_rec, host_done, feas);
        return;
      }
    }
    if (excl && excl->n > 0)
      hipLaunchKernelGGL(score_finish_slot_excl_kernel<decltype(k)::value>, dim3(nb), dim3(threads), 0, c->stream, p, mode == 2 ? 1 : 0,
                         acc, (long long)M, divisor, part, ticket, (unsigned long long *)tab_dev, rank, world, (long long)offset, grid,
                         d, all_slots ? 1 : 0, (unsigned long long *)host_rec, host_done, *excl);
    else
      hipLaunchKernelGGL(score_finish_slot_kernel<decltype(k)::value>, dim3(nb), dim3(threads), 0, c->stream, p, mode == 2 ? 1 : 0, acc,
                         (long long)M, divisor, part, ticket, (unsigned long long *)tab_dev, rank, world, (long long)offset, grid, d,
                         all_slots ? 1 : 0, (unsigned long long *)host_rec, host_done);
  });
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// The record of a row broadcast: the rank that holds global row idx1_global (local0 >= 0, 0-based within its shard) writes
// (0.0, idx1_global, 0, rows, the row); every other rank writes zeros.
int launch_row_slot(b7_ctx *c, uint64_t *tab_dev, int rank, int world, int64_t idx1_global, int64_t local0, const double *grid,
                    int d) {
  hipLaunchKernelGGL(argmax_slot_kernel, dim3(1), dim3(256), 0, c->stream, (const ArgBest *)nullptr, 0,
                     (unsigned long long *)tab_dev, rank, world, (long long)(idx1_global - 1 - (local0 >= 0 ? local0 : 0)),
                     (long long)c->M, grid, d, 1, (long long)local0, (unsigned long long *)nullptr, (unsigned *)nullptr);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_keep_record(b7_ctx *c, uint64_t *tab_dev, int rank, int world) {
  hipLaunchKernelGGL(keep_record_kernel, dim3(1), dim3(256), 0, c->stream, (unsigned long long *)tab_dev, rank, world);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// ---- the refinement's score pieces (b7_eval_nominate_refine, b7_score_grad_compute) ----
template <class F>
static int with_grad_kind(b7_ctx *c, int kind, F f) {
  switch (kind) {
    case B7_SCORE_EI: f(std::integral_constant<int, B7_SCORE_EI>()); return B7_OK;
    case B7_SCORE_LOGEI: f(std::integral_constant<int, B7_SCORE_LOGEI>()); return B7_OK;
    case B7_SCORE_CB: f(std::integral_constant<int, B7_SCORE_CB>()); return B7_OK;
    default: return b7_fail(c, B7_ERR_UNSUPPORTED, "score gradient: kind %d has no gradient piece", kind);
  }
}

int launch_score_grad(b7_ctx *c, const ScoreParams &p, const double *mu, const double *var, const double *dmu, const double *dvar,
                      int64_t M1, int d, double *value, double *grad) {
  PhaseScope ps(c, "refine:score");
  if (M1 <= 0) return B7_OK;
  B7_TRY(with_grad_kind(c, p.kind, [&](auto k) {
    hipLaunchKernelGGL(score_grad_kernel<decltype(k)::value>, dim3((unsigned)((M1 + 15) / 16)), dim3(256), 0, c->stream, p, mu, var, dmu,
                       dvar, (long long)M1, d, value, grad);
  }));
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int launch_refine_step(b7_ctx *c, const ScoreParams &p, const RefStep &r) {
  PhaseScope ps(c, "refine:step");
  B7_TRY(with_grad_kind(c, p.kind, [&](auto k) {
    hipLaunchKernelGGL(refine_step_kernel<decltype(k)::value>, dim3(1), dim3(1024), 0, c->stream, p, r);
  }));
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}
