"""References for the log probability of improvement and the feasibility weight (tests/test_feas_host.py, tests/test_gpu_feas.py):
50-digit arithmetic (mpmath) on the exact values of the float inputs, a float64 numpy/scipy restatement of the three branches as
the device writes them (bot7_amd/csrc/score.hip: b7_logpi), the weight rule w(v, L) in numpy, TH's first-maximum rule, and the
float64 restatement of a constrained nomination on the oracle's posterior.  No GPU needed here."""
import math

import mpmath
import numpy as np
from scipy import special

from _logei_ref import BAR, DPS, HOST_BAR, SQRT1_2, logmeanexp_mp, scaled_errors, to_float  # noqa: F401  (the project's bars)

LOG2 = 0.69314718055994530942


# ---- 50 digits ------------------------------------------------------------------------------------------------------------
def _z_mp(mu, var, fmin, xi):
    return (mpmath.mpf(float(fmin)) - mpmath.mpf(float(mu)) - mpmath.mpf(float(xi))) / mpmath.sqrt(mpmath.mpf(float(var)))


def phi_cdf_mp(mu, var, fmin, xi):
    """Phi(z) as an mpf, z from the exact values of the four doubles.  Call inside mpmath.workdps(DPS)."""
    return mpmath.erfc(-_z_mp(mu, var, fmin, xi) / mpmath.sqrt(2)) / 2


def logpi_mp(mu, var, fmin, xi=0.0):
    """log Phi(z) of every row (mu, var: equal-length vectors; fmin, xi: scalars) as a list of mpf.  For z >= 0 through
    log1p(-(1 - Phi)): 1 - Phi falls below the 50 digits long before it leaves the doubles."""
    out = []
    with mpmath.workdps(DPS):
        for m, v in zip(np.ravel(mu), np.ravel(var)):
            z = _z_mp(m, v, fmin, xi)
            if z >= 0:
                out.append(mpmath.log1p(-mpmath.erfc(z / mpmath.sqrt(2)) / 2))
            else:
                out.append(mpmath.log(mpmath.erfc(-z / mpmath.sqrt(2)) / 2))
    return out


def logpi_mean_mp(mu_cols, var, fmins, xi=0.0):
    """log((1/c) sum_k Phi(z_k)) per row: mu_cols M x c, var M, fmins c."""
    mu_cols = np.asarray(mu_cols, dtype=np.float64)
    c = mu_cols.shape[1]
    with mpmath.workdps(DPS):
        return [mpmath.log(sum(phi_cdf_mp(mu_cols[j, k], var[j], fmins[k], xi) for k in range(c)) / c) for j in range(len(var))]


# ---- float64: the three branches as the device writes them -----------------------------------------------------------------
def logpi_np(mu, var, fmin, xi=0.0):
    """log Phi(z) in float64 with scipy's erfc / erfcx: the same branches (z >= 0; -1 < z < 0; z <= -1), operation order and row
    classes as b7_logpi."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        sigma = np.sqrt(var)
        imprv = (fmin + (-mu)) + (-xi)
        z = imprv / sigma
        up = np.log1p(special.erfc(z * SQRT1_2) * -0.5)
        mid = np.log(special.erfc(z * -SQRT1_2) * 0.5)
        lo = ((z * z) * -0.5 + -LOG2) + np.log(special.erfcx(z * -SQRT1_2))
        out = np.where(z >= 0.0, up, np.where(z > -1.0, mid, lo))
        out = np.where(z == np.inf, 0.0, np.where(z == -np.inf, -np.inf, out))
        flat = np.where(imprv >= 0.0, 0.0, np.where(np.isnan(imprv), imprv, -np.inf))
        return np.where(sigma == 0.0, flat, out)


def feas_weight_np(v, L, log):
    """w(v, L) of score.hip's header: v + L on a log accumulator, v * exp(L) on a linear one; NaN if either operand is NaN;
    otherwise L = -inf gives -inf / 0.0 whatever v is."""
    v, L = np.asarray(v, dtype=np.float64), np.asarray(L, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = v + L if log else v * np.exp(L)
        w = np.where(L == -np.inf, -np.inf if log else 0.0, w)
        return np.where(np.isnan(v) | np.isnan(L), np.nan, w)


def first_max(w):
    """score:max(1) under TH's rule -> 0-based index: the first NaN wins, else the first maximum."""
    w = np.asarray(w)
    nan = np.flatnonzero(np.isnan(w))
    return int(nan[0]) if nan.size else int(np.argmax(w))


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def z_set(rng, n):
    """n rows (mu, var) with fmin = 0, xi = 0 whose z covers: uniform [-40, 8], log-uniform [-1e6, -1], uniform [8, 40], and -- at
    sigma = 1, so that the device's z is exact -- the branch points -1, its two neighbours, and 0.  sigma log-uniform in [1e-6, 1]."""
    k = n // 3
    z = np.concatenate([rng.uniform(-40.0, 8.0, n - 2 * k), -np.exp(rng.uniform(0.0, math.log(1e6), k)), rng.uniform(8.0, 40.0, k)])
    sigma = np.exp(rng.uniform(math.log(1e-6), 0.0, n))
    z[:4] = [-1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), 0.0]
    sigma[:4] = 1.0
    var = sigma * sigma
    mu = -(z * np.sqrt(var))
    mu[3] = 0.0
    return mu, var


# ---- the constrained toy in float64 on the oracle's posterior ----------------------------------------------------------------
def constrained_scores(orc, X_obs, Y, Cobs, X_hid, hyps_obj, hyps_con, threshold, fmin):
    """log((1/S) sum_s EI_s) + log((1/S) sum_s Phi((t - mu_c,s)/sigma_c,s)) over X_hid in float64: the oracle's GP posterior under
    every hyper sample, scipy's logsumexp for the two marginals, the float64 restatements for the per-sample values."""
    from _logei_ref import logei_np
    lei = np.stack([logei_np(*_post(orc, X_obs, Y, X_hid, h), fmin, 0.0) for h in hyps_obj])
    lpf = np.stack([logpi_np(*_post(orc, X_obs, Cobs, X_hid, h), threshold, 0.0) for h in hyps_con])
    a = special.logsumexp(lei, axis=0) - math.log(len(hyps_obj))
    L = special.logsumexp(lpf, axis=0) - math.log(len(hyps_con))
    return a, L


def _post(orc, X_obs, Y, X_hid, h):
    f = orc.gp.fit(X_obs, np.asarray(Y, dtype=np.float64).reshape(len(X_obs), -1), h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    mean, var = orc.gp.predict(f, X_hid)[:2]
    return np.asarray(mean, dtype=np.float64).reshape(len(X_hid), -1)[:, 0], np.asarray(var, dtype=np.float64).ravel()
