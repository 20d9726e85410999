// The ARD-SE and ARD Matern-5/2 covariances, shared by covar.hip (K(X*,X), K(X,X)), gp_small.hip, kpost_small.hip and
// nll_small.hip (the fused small-N kernels): identical code, so identical bits.
#pragma once
#include <hip/hip_runtime.h>

#include "bot7hip.h"
#include "exp_table.h"
#ifndef B7_KSX_ABLATE
#define B7_KSX_ABLATE 0
#endif

// amp * exp(min(arg, 0)) with NaN passing (utils/math.lua:106's clamp of the distance at 0 is TH's: it compares, it does not
// sanitise), in 16 VALU instructions (the Taylor-13 form it replaces took 27: 36 -> 27 per output of the kernel, which is
// bound by VALU + MFMA issue on the one fp64 pipe):
//   a  = max(min(arg, 0), -1000)               v_min / v_max drop a NaN; it is put back below
//   nb = fma(a, 128/ln2, 1.5 * 2^52)           the low mantissa bits of nb ARE n = rint(a * 128/ln2) (two's complement)
//   r  = a - n * ln2/128 in two pieces         HEAD has 35 bits, so n * HEAD is exact for |n| < 2^18; |r| <= ln2/256
//   q  = r * (1 + r/2 + r^2/6 + r^3/24 + r^4/120)        e^r - 1, truncation r^6/720 <= 5.5e-19
//   q  = fma(arg, 0.0, q)                      NaN (or inf) in arg -> NaN; otherwise adds a signed zero
//   amp * exp(a) = 2^(n >> 7) * T[n & 127] * (1 + q),  T[j] = amp * 2^(j/128) in LDS, v_ldexp for the power of two
// (gradual underflow; a = -1000 gives exactly 0).  Measured on the device against mpmath over the whole domain [-1000, 0]
// (tests/test_gpu_numerics.py, amp = 2^-40 .. 2^40): <= 2 ulp where amp * exp(arg) is normal, <= 2^-1074 absolute where it is
// subnormal (tools/gen_exp_table.py writes the table and the constants).
// Padding observations carry zs/2 = 1e300 (not +inf: inf * 0 would make the NaN carrier fire): arg = -1e300 -> exactly 0.
// Four arguments at a time, stage by stage: one such chain is 14 dependent fp64 instructions (8.6 cycles each when the next
// one waits for it, 4.8 when it does not), and the compiler, left to itself, ran the four chains of a 16x16 tile nearly one
// after the other -- the epilogue was bound by latency, not by issue (tools/ksx_ablate.py: a third fewer instructions
// changed nothing).  Written as stages over r = 0..3 the four chains interleave and each instruction's latency is covered
// by the other three.
// keeps the instruction scheduler from moving anything across: without it the four Horner chains are emitted one after the
// other again (it minimises live registers; there are plenty here)
#define B7_STAGE() __builtin_amdgcn_sched_barrier(0)
__device__ __forceinline__ void amp_exp_nonpos4(const double (&arg)[4], const double *__restrict__ tab, double (&out)[4]) {
  double a[4], nb[4], nf[4], r[4], p[4], q[4], t[4];
  int n[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = __builtin_fmin(arg[i], 0.0);
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = __builtin_fmax(a[i], -1000.0);
#pragma unroll
  for (int i = 0; i < 4; ++i) nb[i] = __builtin_fma(a[i], B7_EXP_INV, B7_EXP_MAGIC);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    n[i] = __double2loint(nb[i]);
#if B7_KSX_ABLATE & 2    // every lane reads the same table entry: no LDS bank conflicts
    t[i] = tab[(n[i] >> 20) & 1];
#else
    t[i] = tab[n[i] & 127];
#endif
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) nf[i] = nb[i] - B7_EXP_MAGIC;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_fma(nf[i], -B7_EXP_HEAD, a[i]);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_fma(nf[i], -B7_EXP_TAIL, r[i]);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(r[i], 1.0 / 120.0, 1.0 / 24.0);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 1.0 / 6.0);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 0.5);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 1.0);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = r[i] * p[i];
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = __builtin_fma(arg[i], 0.0, q[i]);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = __builtin_ldexp(__builtin_fma(t[i], q[i], t[i]), n[i] >> 7);
}

// ARD Matern-5/2 on the same argument arg = -D/2 (D = sum_k (x_k - z_k)^2 / lenscale_sq_k, clamped at 0 as above):
//   s = sqrt(5 D) = sqrt(-10 a),  k = amp (1 + s + s^2/3) exp(-s)
// with exp(-s) by the table exponential above and these differences:
//   s   = min(sqrt(-10 a), 1000)               IEEE sqrt (correctly rounded).  The clamp keeps padding's s ~ 3e150 (zs/2 = 1e300)
//                                              out of the polynomial, where it would overflow: amp m exp(-1000) is exactly 0
//   m   = 1 + s (1 + s/3)                      the polynomial, Horner
//   out = 2^(n >> 7) * (m * T[n & 127] (1 + q))            m goes on BEFORE the power of two, so a normal result for s in
//                                              ~700..760 is not built from a subnormal amp exp(-s): one rounding, in v_ldexp
// NaN and inf in arg come through the same carrier on q.  Error: the exponential's and m's few ulp, plus the inherent 0.75 s ulp
// of exp(-s) that comes from rounding s itself (-10 a and the sqrt: 1/4 + 1/2 ulp of s).  k(x, x) = amp as for the SE, so the
// posterior-variance kernels need no form of their own.  Same four-at-a-time staging as amp_exp_nonpos4.  Measured on the
// device against mpmath (tests/test_gpu_matern.py, s in [0, 2000], amp = 2^-40 .. 2^40, both paths): <= s + 2.14 ulp where the
// result is normal, <= 2^-1073 absolute beyond the same relative s term where it is subnormal.
__device__ __forceinline__ void amp_matern52_nonpos4(const double (&arg)[4], const double *__restrict__ tab, double (&out)[4]) {
  double a[4], s[4], nb[4], nf[4], r[4], p[4], q[4], t[4], m[4];
  int n[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = __builtin_fmin(arg[i], 0.0);
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = __builtin_sqrt(-10.0 * a[i]);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = __builtin_fmin(s[i], 1000.0);
#pragma unroll
  for (int i = 0; i < 4; ++i) nb[i] = __builtin_fma(s[i], -B7_EXP_INV, B7_EXP_MAGIC);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    n[i] = __double2loint(nb[i]);
    t[i] = tab[n[i] & 127];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) nf[i] = nb[i] - B7_EXP_MAGIC;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_fma(nf[i], -B7_EXP_HEAD, -s[i]);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = __builtin_fma(nf[i], -B7_EXP_TAIL, r[i]);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(r[i], 1.0 / 120.0, 1.0 / 24.0);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 1.0 / 6.0);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 0.5);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) p[i] = __builtin_fma(p[i], r[i], 1.0);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = r[i] * p[i];
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = __builtin_fma(s[i], 1.0 / 3.0, 1.0);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = __builtin_fma(s[i], m[i], 1.0);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = __builtin_fma(arg[i], 0.0, q[i]);
  B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) t[i] = __builtin_fma(t[i], q[i], t[i]);
B7_STAGE();
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = __builtin_ldexp(m[i] * t[i], n[i] >> 7);
}

// The covariance of the context's kernel (b7_gp_set_kernel), four entries at a time.  KERN is a template parameter of every
// kernel that forms covariance entries (ksx_kernel, gp_small_kernel, kpost_small_kernel, nll_small_kernel) and of their
// launchers, never a run-time branch: the ARD-SE instances are the code they were before the Matern branch existed.  The small
// kernels and the general path share this one function, so they give the same bits under either kernel.
template <int KERN>
__device__ __forceinline__ void cov_nonpos4(const double (&arg)[4], const double *__restrict__ tab, double (&out)[4]) {
  static_assert(KERN == B7_KERNEL_ARDSE || KERN == B7_KERNEL_MATERN52, "covariance kernel");
  if constexpr (KERN == B7_KERNEL_ARDSE)
    amp_exp_nonpos4(arg, tab, out);
  else
    amp_matern52_nonpos4(arg, tab, out);
}

// The covariance AND its radial factor g, with dk/dx_c = -g (x_c - z_c) / lenscale_sq_c, for the kernels that need the posterior's
// gradient (refine.hip; nothing else instantiates it).  k is cov_nonpos4<KERN>'s own bits: the ARD-SE branch calls it (g = k); the
// Matern branch is amp_matern52_nonpos4 stage by stage, sharing its s and exponential, with one more polynomial on the way out:
//   g = (5/3) amp (1 + s) exp(-s)          finite at D = 0, where the difference factor is 0
template <int KERN>
__device__ __forceinline__ void cov_grad_nonpos4(const double (&arg)[4], const double *__restrict__ tab, double (&out)[4],
                                                 double (&g)[4]) {
  static_assert(KERN == B7_KERNEL_ARDSE || KERN == B7_KERNEL_MATERN52, "covariance kernel");
  if constexpr (KERN == B7_KERNEL_ARDSE) {
    amp_exp_nonpos4(arg, tab, out);
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = out[i];
  } else {
    double a[4], s[4], nb[4], nf[4], r[4], p[4], q[4], t[4], m[4], m2[4];
    int n[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = __builtin_fmin(arg[i], 0.0);
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = __builtin_fmin(__builtin_sqrt(-10.0 * a[i]), 1000.0);
#pragma unroll
    for (int i = 0; i < 4; ++i) nb[i] = __builtin_fma(s[i], -B7_EXP_INV, B7_EXP_MAGIC);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      n[i] = __double2loint(nb[i]);
      t[i] = tab[n[i] & 127];
      nf[i] = nb[i] - B7_EXP_MAGIC;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = __builtin_fma(nf[i], -B7_EXP_TAIL, __builtin_fma(nf[i], -B7_EXP_HEAD, -s[i]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p[i] = __builtin_fma(r[i], 1.0 / 120.0, 1.0 / 24.0);
      p[i] = __builtin_fma(p[i], r[i], 1.0 / 6.0);
      p[i] = __builtin_fma(p[i], r[i], 0.5);
      p[i] = __builtin_fma(p[i], r[i], 1.0);
      q[i] = __builtin_fma(arg[i], 0.0, r[i] * p[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      m[i] = __builtin_fma(s[i], __builtin_fma(s[i], 1.0 / 3.0, 1.0), 1.0);
      m2[i] = __builtin_fma(s[i], 5.0 / 3.0, 5.0 / 3.0);
      t[i] = __builtin_fma(t[i], q[i], t[i]);
      out[i] = __builtin_ldexp(m[i] * t[i], n[i] >> 7);
      g[i] = __builtin_ldexp(m2[i] * t[i], n[i] >> 7);
    }
  }
}
