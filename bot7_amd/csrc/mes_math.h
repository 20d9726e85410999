// The two scalar functions of max-value entropy search (mes.hip: the search; score.hip: the score), through ocml's fp64 erfc,
// erfcx, log1p, log and exp as LogEI's are.  Included after `#pragma clang fp contract(off)`: one rounded operation per operator.
#pragma once
#include <hip/hip_runtime.h>

// log Phi(g), Phi(g) = erfc(-g/sqrt2)/2:
//   g >  0:       log1p(-erfc(g/sqrt2)/2)                      (Phi is within 1/2 of 1: its distance from 1 is what is known well)
//   -1 < g <= 0:  log(erfc(-g/sqrt2)/2)
//   g <= -1:      -g^2/2 + log(erfcx(-g/sqrt2)/2)              (Phi = exp(-g^2/2) erfcx(-g/sqrt2)/2; NaN comes this way and stays NaN)
__device__ __forceinline__ double b7_log_ndtr(double g) {
  const double u = g * 0.70710678118654752440;  // g/sqrt2
  if (g > 0.0) return log1p(erfc(u) * -0.5);
  if (g > -1.0) return log(erfc(-u) * 0.5);
  return ((g * g) * -0.5) + log(erfcx(-u) * 0.5);
}

// h(g) = g phi(g) / (2 Phi(g)) - log Phi(g): the entropy reduction of a Gaussian truncated at the optimum's value (Wang & Jegelka,
// "Max-value Entropy Search for Efficient Bayesian Optimization", ICML 2017, eq. 6), g = (mu - y*)/sigma for a MINIMUM y*.
// For g <= -1 the exp(-g^2/2) of phi and of Phi cancel on paper: phi/Phi = sqrt(2/pi) / erfcx(-g/sqrt2).  Held to
// 1e-13 max(1, |h|) for g >= -8; below that the same form stays finite (down to g ~ -1e154) but g^2/2 and g phi/(2 Phi) cancel
// ever more digits.  phi == 0 (g beyond ~38.6, +inf included): the first term is 0, not inf * 0.
__device__ __forceinline__ double b7_mes_h(double g) {
  const double u = g * 0.70710678118654752440;
  if (g > -1.0) {
    const double pdf = exp((g * g) * -0.5) * 0.39894228040143267794;  // 1/sqrt(2 pi)
    double cdf, lcdf;
    if (g > 0.0) {
      const double q = erfc(u) * 0.5;  // 1 - Phi
      cdf = 1.0 + (-q);
      lcdf = log1p(-q);
    } else {
      cdf = erfc(-u) * 0.5;
      lcdf = log(cdf);
    }
    const double a = (pdf == 0.0) ? 0.0 : (g * (pdf / cdf)) * 0.5;
    return a + (-lcdf);
  }
  const double e = erfcx(-u);
  const double a = (g * (0.79788456080286535588 / e)) * 0.5;  // sqrt(2/pi) / erfcx = phi/Phi
  return (a + ((g * g) * 0.5)) + (-log(e * 0.5));
}
