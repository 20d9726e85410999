// Log-space expected improvement and the log-sum-exp step, once: score.hip's B7_SCORE_LOGEI and ehvi_math.h's log Psi read the same
// text.  The formula, its three branches and its edge cases are described in score.hip's header.  Every translation unit that includes
// this compiles with contraction off (the pragma below); erfc, erfcx, exp, log and log1p are ocml's.
#pragma once
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

// log EI from sigma = sqrt(var).  HOISTED: lsigma = log(sigma) comes from the caller, who scores one (mu, var) against many thresholds
// and takes the logarithm once; otherwise it is taken here, where the value is log(sigma) + log h(z), and lsigma is not read
template <bool HOISTED>
__device__ __forceinline__ double b7_logei_core(double mu, double sigma, double lsigma, double fmin, double xi) {
  const double imprv = (fmin + (-mu)) + (-xi);
  const double z = imprv / sigma;
  if (sigma == 0.0 || z == INFINITY) return (imprv > 0.0) ? log(imprv) : ((imprv != imprv) ? imprv : -INFINITY);
  if (z == -INFINITY) return -INFINITY;
  double lh;
  if (z > -1.0) {
    const double pdf = exp((z * z) * -0.5) * 0.39894228040143267794;  // 1/sqrt(2 pi)
    const double cdf = erfc(z * -0.70710678118654752440) * 0.5;       // Phi(z) = erfc(-z/sqrt2)/2
    lh = log(pdf + (z * cdf));
  } else {  // NaN comes this way too, and stays NaN
    const double t = -z;
    double l1r;  // log(1 - r), r = t sqrt(pi/2) erfcx(t/sqrt2) = -z Phi(z)/phi(z)
    if (t >= 1e5) {
      l1r = (log(t) * -2.0) + log1p(-3.0 / (t * t));  // 1 - r = (1 - 3/t^2 + ..)/t^2: r itself rounds to 1 or past it out here
    } else {
      const double r = (t * 1.2533141373155002512) * erfcx(t * 0.70710678118654752440);
      l1r = log1p(-r);
    }
    lh = (((z * z) * -0.5) + -0.91893853320467274178) + l1r;  // log phi(z) + log(1 - r)
  }
  return (HOISTED ? lsigma : log(sigma)) + lh;
}
// ---- log-space EI (score.hip's header) ----
__device__ __forceinline__ double b7_logei(double mu, double var, double fmin, double xi) {
  const double sigma = sqrt(var);
  return b7_logei_core<false>(mu, sigma, 0.0, fmin, xi);
}
__device__ __forceinline__ double b7_logaddexp(double a, double v) {
  if (a != a || v != v) return a + v;
  const double m = (a > v) ? a : v, n = (a > v) ? v : a;
  if (m == -INFINITY || n == INFINITY) return m;  // both -inf, both +inf: n - m would be NaN
  return m + log1p(exp(n + (-m)));
}
