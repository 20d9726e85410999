"""References for log-space expected improvement (tests/test_logei_host.py, tests/test_gpu_logei.py): 50-digit arithmetic
(mpmath) on the exact values of the float inputs, and a float64 numpy/scipy restatement of the formula the device evaluates
(bot7_amd/csrc/score.hip: b7_logei, b7_logaddexp).  No GPU needed here."""
import math

import mpmath
import numpy as np
from scipy import special

DPS = 50
BAR = 1e-13          # |err| <= BAR * max(1, |ref|): the device's bar (test_gpu_logei)
HOST_BAR = 1e-14     # the same measure for the scipy restatement (test_logei_host)


# ---- 50 digits ------------------------------------------------------------------------------------------------------------
def ei_mp(mu, var, fmin, xi):
    """sigma * (phi(z) + z Phi(z)) as an mpf, z = ((fmin - mu) - xi) / sqrt(var), from the exact values of the four doubles.
    Call inside mpmath.workdps(DPS).  phi + z Phi cancels to phi / z^2 in the lower tail: 12 of the 50 digits at z = -1e6."""
    sigma = mpmath.sqrt(mpmath.mpf(float(var)))
    imprv = mpmath.mpf(float(fmin)) - mpmath.mpf(float(mu)) - mpmath.mpf(float(xi))
    z = imprv / sigma
    pdf = mpmath.exp(-z * z / 2) / mpmath.sqrt(2 * mpmath.pi)
    cdf = mpmath.erfc(-z / mpmath.sqrt(2)) / 2
    return sigma * (pdf + z * cdf)


def logei_mp(mu, var, fmin, xi=0.0):
    """log EI of every row (mu, var: equal-length vectors; fmin, xi: scalars) as a list of mpf."""
    with mpmath.workdps(DPS):
        return [mpmath.log(ei_mp(m, v, fmin, xi)) for m, v in zip(np.ravel(mu), np.ravel(var))]


def logei_mean_mp(mu_cols, var, fmins, xi=0.0):
    """log((1/c) sum_k EI_k) per row: mu_cols M x c, var M, fmins c -- what c response columns (fantasies) score."""
    mu_cols = np.asarray(mu_cols, dtype=np.float64)
    c = mu_cols.shape[1]
    with mpmath.workdps(DPS):
        return [mpmath.log(sum(ei_mp(mu_cols[j, k], var[j], fmins[k], xi) for k in range(c)) / c) for j in range(len(var))]


def logmeanexp_mp(cols):
    """log((1/S) sum_s exp(l_s)) per row for S lists of mpf: the marginal over S hyper samples."""
    S = len(cols)
    with mpmath.workdps(DPS):
        out = []
        for ls in zip(*cols):
            m = max(ls)
            out.append(m + mpmath.log(sum(mpmath.exp(l - m) for l in ls) / S))
        return out


def to_float(vals):
    return np.array([float(v) for v in vals], dtype=np.float64)


def scaled_errors(got, ref_mp):
    """|got - ref| / max(1, |ref|) per row, the difference taken in 50 digits."""
    with mpmath.workdps(DPS):
        return np.array([float(abs(mpmath.mpf(float(g)) - r) / max(mpmath.mpf(1), abs(r))) for g, r in zip(got, ref_mp)])


# ---- float64: the formula as the device writes it ----------------------------------------------------------------------------
SQRT1_2 = 0.70710678118654752440
SQRT_PI_2 = 1.2533141373155002512
HALF_LOG_2PI = 0.91893853320467274178
INV_SQRT_2PI = 0.39894228040143267794


def logei_np(mu, var, fmin, xi=0.0):
    """log EI in float64 with scipy's erfc / erfcx / log1p: the same branches (z > -1; -1e5 < z <= -1; the far tail z <= -1e5) and
    operation order as b7_logei."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        sigma = np.sqrt(var)
        imprv = (fmin + (-mu)) + (-xi)
        z = imprv / sigma
        up = np.log(np.exp((z * z) * -0.5) * INV_SQRT_2PI + z * (special.erfc(z * -SQRT1_2) * 0.5))
        t = -z
        near = np.log1p(-((t * SQRT_PI_2) * special.erfcx(t * SQRT1_2)))     # log(1 - r); NaN wherever r rounds past 1 ...
        far = (np.log(t) * -2.0) + np.log1p(-3.0 / (t * t))                    # ... which the tail t >= 1e5 never evaluates
        lo = ((z * z) * -0.5 + -HALF_LOG_2PI) + np.where(t >= 1e5, far, near)
        out = np.log(sigma) + np.where(z > -1.0, up, lo)
        flat = np.where(imprv > 0.0, np.log(imprv), np.where(np.isnan(imprv), imprv, -np.inf))
        out = np.where((sigma == 0.0) | (z == np.inf), flat, out)
        return np.where(z == -np.inf, -np.inf, out)


def logaddexp_np(a, v):
    """m + log1p(exp(n - m)), m = max, n = min; -inf (+inf) when both are; NaN if either is."""
    a, v = np.asarray(a, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        m, n = np.where(a > v, a, v), np.where(a > v, v, a)
        out = m + np.log1p(np.exp(n + (-m)))
        out = np.where((m == -np.inf) | (n == np.inf), m, out)
        return np.where(np.isnan(a) | np.isnan(v), a + v, out)


def packed_z(rng, n):
    """n draws of z over [-1e6, 8]: a log-uniform lower tail, a uniform body, and a third packed tightly around the branch point
    -1 and the two places where EI's ingredients die: -8.6 (Phi of the A&S erf is exactly 0) and -38.6 (phi underflows)."""
    k = n // 6
    parts = [-np.exp(rng.uniform(math.log(1.0), math.log(1e6), n - 5 * k)), rng.uniform(-40.0, 8.0, 2 * k)]
    for centre in (-1.0, -8.6, -38.6):
        parts.append(centre + rng.normal(scale=0.05, size=k))
    z = np.concatenate(parts)
    z[:4] = [-1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -1e6]
    return z


def far_tail_t(rng, n):
    """n draws of t = -z, log-uniform over [1e7, 1e12], increasing: where t sqrt(pi/2) erfcx(t/sqrt2) is within an ulp of 1 and a
    log1p(-r) taken from it is NaN or -inf in turns."""
    return np.sort(np.exp(rng.uniform(math.log(1e7), math.log(1e12), n)))
