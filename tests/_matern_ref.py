"""Host references for the ARD Matern-5/2 covariance (b7_gp_set_kernel(ctx, B7_KERNEL_MATERN52)):
    K = amp (1 + s + s^2/3) exp(-s),  s = sqrt(5 D),  D = sum_k (x_k - z_k)^2 / lenscale_sq_k
in numpy (the oracle's distance, oracle/gp.py:pdist), in 40-digit arithmetic at exact arguments (tests/_exact.py's constructors),
and the LAPACK fit / posterior / likelihood on that K.  Checked on the CPU by tests/test_matern_host.py."""
import math

import mpmath
import numpy as np
from scipy.linalg import lapack, solve_triangular

import _exact as E


def matern52(X, Z, lenscale_sq, amp):
    """amp (1 + s + s^2/3) exp(-s) with s = sqrt(5 D), D the oracle's clamped distance (GEMM form, as the device's)."""
    from oracle import gp
    D = gp.pdist(X, Z, lenscale_sq)
    s = np.sqrt(5.0 * D)
    return amp * (1.0 + s + s * s / 3.0) * np.exp(-s)


# ---- exact arguments: arg = -D/2 as the kernels form it; s = sqrt(-10 arg) ---------------------------------------------------
def matern_targets(dense=4000, seed=0):
    """Kernel arguments arg = -s^2/10 for s over a dense sweep of [0, 1000], the band s in [700, 760] (where amp m exp(-s) crosses
    into the subnormal range for the amplitudes of the sweep), the neighbourhood of 0 and the clamp at s = 1000."""
    rng = np.random.default_rng(seed)
    s = list(np.linspace(0.0, 1000.0, dense)) + list(np.linspace(700.0, 760.0, 1500)) + list(rng.uniform(0.0, 1000.0, 512))
    s += list(np.exp(rng.uniform(np.log(1e-6), np.log(1.0), 256))) + [1000.0, 1000.5, 1100.0, 2000.0]
    return [-(v * v) / 10.0 for v in s]


def matern_points(d, dense=4000, seed=0):
    """Rows X with an exact float64 argument against an observation at the origin (lenscale_sq = 1): exp_points over
    matern_targets, plus _exact.special_exp_rows (the origin itself, -2^-1001, -1000 and -1e4).  Returns (X, exact args)."""
    X, args = E.exp_points(matern_targets(dense, seed), d, 0)
    Xs, sargs = E.special_exp_rows(d)
    return np.concatenate([X, Xs]), args + sargs


def matern_truth(amp, args, dps=40):
    """amp (1 + s + s^2/3) exp(-s) at s = sqrt(-10 arg) for exact arguments (Fractions), as (hi, lo) pairs and the s values."""
    with mpmath.workdps(dps):
        out, ss = [], []
        for a in args:
            s = mpmath.sqrt(-10 * mpmath.mpf(a.numerator) / a.denominator)
            out.append(mpmath.mpf(amp) * (1 + s + s * s / 3) * mpmath.exp(-s))
            ss.append(float(s))
        hi, lo = E.pairs(out)
    return hi, lo, np.array(ss)


def within_matern_bar(got, hi, lo, s, extra=4.0):
    """The Matern bar: (extra + s) ulp of the truth where it is normal -- the s term covers the 0.75 s ulp that rounding s itself
    costs (-10 arg and the sqrt round; exp(-s) turns an absolute error of s into a relative one of the result) --, and below
    that 2^-1073 absolute PLUS the same relative s term, s 2^-52 |truth|: that error is inherent, it does not stop at the
    normal range (at s ~ 745 it is ~1e-13 of the value, ~400 subnormal ulps just below 2^-1022).  Returns (ok, worst normal
    error in ulp minus s, worst subnormal error beyond the relative s term, absolute)."""
    normal = np.abs(hi) >= E.TINY
    u = E.ulp_errors(got, hi, lo)
    a = E.abs_errors(got, hi, lo)
    rel = s * E.EPS * np.abs(hi)
    ok = bool(np.all(u[normal] <= extra + s[normal]) and np.all(a[~normal] <= E.SUB_BAR + rel[~normal]))
    wu = float(np.max(u[normal] - s[normal])) if normal.any() else 0.0
    wa = float(np.max(a[~normal] - rel[~normal])) if (~normal).any() else 0.0
    return ok, wu, wa


# ---- LAPACK fits -------------------------------------------------------------------------------------------------------------
def chol_jitter(K, eps=1e-8, growth=1.1):
    from oracle import gp
    return gp.chol_jitter(K, eps, growth)


def lapack_fit(X, Y, lenscale_sq, amp, noise, mean, Xs=None, jitter=None):
    """The GP algebra of oracle/gp.py on the Matern K: utils.math.chol's jitter schedule (or a GIVEN jitter), alpha, NLL, and at
    Xs the posterior mean and latent variance.  Returns dict(nll, jitter, info, L, alpha, mu, var)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64).reshape(-1, 1)
    K = matern52(X, None, lenscale_sq, amp)
    K[np.diag_indices(K.shape[0])] += noise
    if jitter is None:
        L, jit, info = chol_jitter(K)
    else:
        Kj = K.copy()
        Kj[np.diag_indices(K.shape[0])] += jitter
        L, info = lapack.dpotrf(Kj, lower=1, clean=1)
        if info != 0:
            return None
        jit = jitter
    r = y - mean
    alpha = solve_triangular(L, solve_triangular(L, r, lower=True), lower=True, trans="T")
    out = {"L": L, "alpha": alpha, "jitter": jit, "info": int(info),
           "nll": float(0.5 * np.sum(r * alpha) + np.sum(np.log(np.diag(L))) + 0.5 * X.shape[0] * math.log(2.0 * math.pi))}
    if Xs is not None:
        Ks = matern52(Xs, X, lenscale_sq, amp)
        out["mu"] = mean + (Ks @ alpha)[:, 0]
        V = solve_triangular(L, Ks.T, lower=True, check_finite=False)
        out["var"] = amp - np.einsum("ij,ij->j", V, V)
    return out


def ei(mu, var, fmin, tradeoff=0.0):
    """The oracle's EI (scores/expected_improvement.lua:69-88) on host vectors."""
    from oracle import cport
    return cport.ei(np.asarray(mu, dtype=np.float64).reshape(-1, 1), np.asarray(var, dtype=np.float64), [fmin], tradeoff)


def cb(mu, var, tradeoff=1.0, upper=False, sign=-1.0):
    from oracle import cport
    return cport.cb(np.asarray(mu, dtype=np.float64).reshape(-1, 1), np.asarray(var, dtype=np.float64), tradeoff, upper, sign)
