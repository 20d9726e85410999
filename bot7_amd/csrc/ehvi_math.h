// The arithmetic of the expected hypervolume improvement, once: Psi, and the two policies (EhviLin, EhviLog) that make the linear
// scores b7_ehvi_* / b7_ehvi3_* and the log-space scores b7_logehvi_* / b7_logehvi3_* out of the same three kernel bodies
// (ehvi.hip's ehvi2_kernel, ehvi3.hip's ehvi3_table_kernel and ehvi3_box_kernel).  No counterpart in the reference's scores/.  All
// objectives are minimised.  Every translation unit that includes this compiles with contraction off (the pragma below); erfc, erfcx,
// exp, expm1, log, log1p are ocml's: one rounded operation per operator.
//
// A policy says what the kernels stage per sample (NV values, made from (mu, var) once, ahead of the strips / cuts), what
// psi(cut, sample) is, how terms are folded (a Fold starts as empty(), add() takes a term, value() reads it, mean() divides it by the
// sample count that count() prepared; none() is the value of an empty one, and Psi(-inf)), how a difference diff(u, l) and a product
// times(x, y) are formed, and the names of its phases.  The linear Fold is a plain double.
//
// LINEAR (EhviLin).  Psi(a; mu, sigma) = E[(a - y)+] = (a - mu) Phi(z) + sigma phi(z),  z = (a - mu) / sigma,  Psi(-inf) = 0, in the
// POSITIVE-TERM FORM of kg.hip's kg_f: with d = a - mu and t = |d| / sigma,
//   f = max(phi(t) - t erfc(t / sqrt2) / 2, 0)        (= phi(-t) - t Phi(-t), the one subtraction there is); f = 0 for t > 37.5,
//                                                      where both terms are below the smallest normal double
//   Psi = sigma f (d <= 0),   d + sigma f (d > 0: two positive terms);   sigma == 0: max(d, 0) exactly.
// A sum is a running double from 0, a mean is the sum divided once by its sample count, diff(u, l) = max(u - l, 0) (Psi is monotone in
// a; only rounding can break that, and the clamp keeps every term non-negative), times is the product.
//
// LOG SPACE (EhviLog): log of the linear score, evaluated so that it never underflows -- the multi-objective twin of LogEI (Ament et
// al., "Unexpected Improvements to Expected Improvement", NeurIPS 2023).  The linear scores are exactly 0 wherever a Psi has z < -37.5
// in every strip or box (a reference point no observation has reached, late trials, most of a large grid), and score:max(1) then
// nominates row 1; this score still ranks those rows.
// Arithmetic (the same text in bot7hip.h and in tests/_logehvi_ref.py's numpy restatement):
//   logPsi(a; mu, var) = b7_logei(mu, var, fmin = a, xi = 0)           logei_math.h: its three branches, its edge cases; a = -inf: -inf
//   ldiff(u, l) = log(e^u - e^l):   l == -inf: u exactly;   !(l < u): -inf (the linear code's clamp at 0);
//                                   d = l - u:  u + log(-expm1(d)) if d > -ln 2, else u + log1p(-exp(d))
//   LSE over terms t_1 .. t_n in a fixed order, RUNNING-MAX form: (m, acc) = (-inf, 0); a term t == -inf is skipped; otherwise
//                                   e = exp(-|t - m|) and (m, acc) = (t, acc e + 1) if t > m, else (m, acc + e);
//                                   the value is -inf if m == -inf, else m + log(acc).  One exp per term, one log at the end; an empty
//                                   sum is -inf, a single term comes back exactly (acc = 1), and the error does not grow with |value|.
//   two objectives, strips as in ehvi.hip (a_0 = -inf, a_P+1 = r1, b_0 = r2):
//     log score = LSE_k[(LSE_s ldiff(logPsi(a_k+1; s), logPsi(a_k; s)) - log S1) + (LSE_t logPsi(b_k; t) - log S2)]
//     k ascending, s / t ascending within it; logPsi(a_k+1; s) is evaluated once and kept as strip k + 1's logPsi(a_k; s).
//   three objectives, boxes of b7_nondominated_boxes3 in its order, LT_m(c) = LSE_s logPsi(c; s) - log S_m, LT_m(-inf) = -inf:
//     log score = LSE_b[(ldiff(LT1(u1), LT1(l1)) + ldiff(LT2(u2), LT2(l2))) + LT3(u3)]
// log S is ocml's log of the sample count (S = 1: exactly 0).  Per sample (mu, sigma = sqrt(var), log sigma) are taken once.
// Thin strips need no special care: a strip's cancellation error is a few eps |log Psi| of Psi1(a_k+1) B_k, and the total is at least
// that product because the strips below it have the larger B (three objectives: the non-dominated region is down-closed).
// Row classes: NaN exactly where the linear score is NaN -- any mu or var NaN, any var < 0, in any objective.  Otherwise, for finite
// input, never NaN and never +inf; -inf is a legal value (every var == 0 and the point dominated).
//
// The log nominations write the marginal log score into the first context's accumulator as a LOG accumulator (score.hip's acc_*
// state), so b7_score_finish(1) downloads it and b7_feas_add_acc takes it: constrained multi-objective nomination is b7_feas_reset,
// b7_feas_add / b7_feas_add_acc, b7_feas_nominate.
//
// Out of scope, for the log scores as for the linear ones: four or more objectives, correlated objectives / multi-task GPs, batches,
// refinement, sharded grids and groups, the Bayesian-linear head, trust regions with three objectives, the bot's
// config.bot.constraints combined with objectives.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "logei_math.h"

// f(-t) = phi(t) - t Phi(-t) for t >= 0, clamped at 0.  Beyond t = 37.5 it is 0: there phi(t) and t Phi(-t) fall below 2^-1022,
// their difference (a 1 / t^2 of either) would be made of the few bits a subnormal has left; t = inf and NaN end here too
__device__ __forceinline__ double ehvi_f(double t) {
  if (!(t <= 37.5)) return 0.0;
  const double pdf = exp((t * t) * -0.5) * 0.39894228040143267794;  // 1/sqrt(2 pi)
  const double q = erfc(t * 0.70710678118654752440) * 0.5;          // Phi(-t) = erfc(t/sqrt2)/2
  const double f = pdf - (t * q);
  return f > 0.0 ? f : 0.0;
}
__device__ __forceinline__ double ehvi_psi(double a, double m, double sd) {
  const double d = a - m;
  if (sd == 0.0) return d > 0.0 ? d : 0.0;
  const double g = sd * ehvi_f(fabs(d / sd));
  return d > 0.0 ? d + g : g;
}

// log(e^u - e^l) (the header)
__device__ __forceinline__ double ldiff(double u, double l) {
  if (l == -INFINITY) return u;
  if (!(l < u)) return -INFINITY;
  const double d = l - u;
  return d > -0.69314718055994530942 ? u + log(-expm1(d)) : u + log1p(-exp(d));
}

// the running-max log-sum-exp (the header)
struct Lse {
  double m = -INFINITY, acc = 0.0;
  __device__ __forceinline__ void add(double t) {
    if (t == -INFINITY) return;
    const bool up = t > m;
    const double e = exp(up ? m - t : t - m);
    acc = up ? (acc * e) + 1.0 : acc + e;
    m = up ? t : m;
  }
  __device__ __forceinline__ double value() const { return m == -INFINITY ? -INFINITY : m + log(acc); }
};

struct EhviLin {
  static constexpr const char *phase2 = "ehvi", *name3 = "ehvi3", *phase3_tab = "ehvi3_tab", *phase3_box = "ehvi3_box";
  static constexpr int NV = 2;  // mu, sigma
  using Fold = double;
  static __device__ __forceinline__ Fold empty() { return 0.0; }
  static __device__ __forceinline__ void add(Fold &f, double t) { f = f + t; }
  static __device__ __forceinline__ double value(const Fold &f) { return f; }
  static __device__ __forceinline__ double none() { return 0.0; }
  static __device__ __forceinline__ void stage(double m, double var, double *v) { v[0] = m, v[1] = sqrt(var); }
  static __device__ __forceinline__ double psi(double a, const double *v) { return ehvi_psi(a, v[0], v[1]); }
  static __device__ __forceinline__ double count(int S) { return (double)S; }
  static __device__ __forceinline__ double mean(const Fold &f, double n) { return f / n; }
  static __device__ __forceinline__ double diff(double u, double l) {
    const double d = u - l;
    return d > 0.0 ? d : 0.0;
  }
  static __device__ __forceinline__ double times(double x, double y) { return x * y; }
};

struct EhviLog {
  static constexpr const char *phase2 = "logehvi", *name3 = "logehvi3", *phase3_tab = "logehvi3_tab", *phase3_box = "logehvi3_box";
  static constexpr int NV = 3;  // mu, sigma, log sigma
  using Fold = Lse;
  static __device__ __forceinline__ Fold empty() { return Lse(); }
  static __device__ __forceinline__ void add(Fold &f, double t) { f.add(t); }
  static __device__ __forceinline__ double value(const Fold &f) { return f.value(); }
  static __device__ __forceinline__ double none() { return -INFINITY; }
  static __device__ __forceinline__ void stage(double m, double var, double *v) {
    const double sd = sqrt(var);
    v[0] = m, v[1] = sd, v[2] = log(sd);
  }
  static __device__ __forceinline__ double psi(double a, const double *v) { return b7_logei_core<true>(v[0], v[1], v[2], a, 0.0); }
  static __device__ __forceinline__ double count(int S) { return log((double)S); }
  static __device__ __forceinline__ double mean(const Fold &f, double ln) { return f.value() - ln; }
  static __device__ __forceinline__ double diff(double u, double l) { return ldiff(u, l); }
  static __device__ __forceinline__ double times(double x, double y) { return x + y; }
};
