// The three scalar functions of the probit likelihood Pr[v = 1 | h] = Phi(h) (laplace.hip), through ocml's fp64 erfc, erfcx, log1p
// and log, as LogPI's and MES's pieces are.  Included after `#pragma clang fp contract(off)`: one rounded operation per operator.
// Held to 1e-13 max(1, |value|) of 50-digit arithmetic over z in [-1e6, 40] (tests/test_laplace_host.py states the same formulas in
// float64; tests/test_gpu_laplace.py holds these).
#pragma once
#include <hip/hip_runtime.h>

// log Phi(z): the three branches of b7_log_ndtr (mes_math.h) and b7_logpi (score.hip), restated here so that neither of those
// translation units changes:
//   z >  0:       log1p(-erfc(z/sqrt2)/2)
//   -1 < z <= 0:  log(erfc(-z/sqrt2)/2)
//   z <= -1:      -z^2/2 + log(erfcx(-z/sqrt2)/2)        (NaN comes this way and stays NaN)
__device__ __forceinline__ double b7_probit_logcdf(double z) {
  const double u = z * 0.70710678118654752440;  // z/sqrt2
  if (z > 0.0) return log1p(erfc(u) * -0.5);
  if (z > -1.0) return log(erfc(-u) * 0.5);
  return ((z * z) * -0.5) + log(erfcx(-u) * 0.5);
}

// rho(z) = phi(z)/Phi(z) = sqrt(2/pi) / erfcx(-z/sqrt2), as grad<LOGEI> forms it (score.hip): no exponential, so neither factor
// underflows on the left (rho ~ -z) and the quotient is 0 on the right once erfcx has overflowed (z beyond ~37.5, where phi/Phi is
// below 1e-300 anyway).
__device__ __forceinline__ double b7_probit_ratio(double z) { return 0.79788456080286535588 / erfcx(z * -0.70710678118654752440); }

// W(z) = -d^2/dz^2 log Phi(z) = rho (rho + z), in [0, 1]; rho = b7_probit_ratio(z).
// For z >= -6 the product as written (the sum cancels at most eps z^2 <= 36 eps).  Below, rho + z is what is left of two numbers that
// agree to 1/z^2, and it is taken from the continued fraction of the Mills ratio instead, which has no cancellation: with t = -z,
//   rho = t + 1/(t + 2/(t + 3/(t + ...)))   =>   rho + z = 1/(t + 2/(t + 3/(t + ... + 24/t)))
// evaluated from the bottom; 24 levels are within 1e-17 of the limit at t = 6 and closer beyond.  Clamped at 0 from below (a rounding
// of the product at the far right, where W ~ 1e-300, must not make B = I + W^1/2 K W^1/2 indefinite).
__device__ __forceinline__ double b7_probit_w(double z, double rho) {
  double w;
  if (z > -6.0) {
    w = rho * (rho + z);
  } else {
    const double t = -z;
    double v = t;
#pragma unroll 1
    for (int k = 24; k >= 2; --k) v = t + (double)k / v;
    w = rho * (1.0 / v);
  }
  return (w > 0.0) ? w : 0.0;  // (NaN: 0 -- the likelihood term is NaN already and the fit reports it through nll)
}
