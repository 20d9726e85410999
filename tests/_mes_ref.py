"""References for max-value entropy search (tests/test_mes_host.py, tests/test_gpu_mes.py).  No GPU needed here.

The score's h(g) = g phi(g) / (2 Phi(g)) - log Phi(g) in 50-digit arithmetic (mpmath) on the exact values of the float inputs; the
log-survival of the grid minimum L(y) = sum_j log Phi((mu_j - y)/sigma_j) as math.fsum of scipy's log_ndtr; y* by BISECTION of
L(y) = t_k to adjacent doubles on the bracket [min_j(mu_j - 10 sigma_j), min_j(mu_j + 10 sigma_j)] -- not the device's 15-probe
rounds --; the row classes (bad: NaN; exact: 0.0; live) and the nominee rule (first NaN, else max, ties to the lowest index)."""
import math

import mpmath
import numpy as np
from scipy import special

DPS = 50
BAR = 1e-13                      # |err| <= BAR * max(1, |ref|): the project's bar for a score through ocml (LogEI's)
P, R = 15, 10                    # the device's probes per round and rounds ...
RESOLUTION = 0.5 * (P + 1.0) ** -R   # ... leave the root within this fraction of (hi0 - lo0) of the last bracket's midpoint
KMAX = 64


# ---- 50 digits ------------------------------------------------------------------------------------------------------------
def h_mp(g):
    """h(g) as an mpf, g an mpf or a float.  Call inside mpmath.workdps(DPS).  For g > 0, Phi is taken from its distance to 1
    (erfc(g/sqrt2)/2 has the whole exponent range of an mpf), so h is resolved down to the 1e-300s."""
    g = mpmath.mpf(g)
    pdf = mpmath.exp(-g * g / 2) / mpmath.sqrt(2 * mpmath.pi)
    if g > 0:
        q = mpmath.erfc(g / mpmath.sqrt(2)) / 2
        cdf, lcdf = 1 - q, mpmath.log1p(-q)
    else:
        cdf = mpmath.erfc(-g / mpmath.sqrt(2)) / 2
        lcdf = mpmath.log(cdf)
    return g * pdf / (2 * cdf) - lcdf


def log_ndtr_mp(g):
    g = mpmath.mpf(g)
    if g > 0:
        return mpmath.log1p(-mpmath.erfc(g / mpmath.sqrt(2)) / 2)
    return mpmath.log(mpmath.erfc(-g / mpmath.sqrt(2)) / 2)


def classes(mu, var):
    """(bad, exact, live) boolean masks."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = np.isnan(mu) | np.isnan(var) | (var < 0)
    exact = ~bad & (var == 0)
    return bad, exact, ~bad & ~exact


def mes_ref(mu, var, ystar):
    """The score of every row with the K values ystar: a list of mpf (live rows), 0 (exact rows) and NaN (bad rows); g is formed
    in 50 digits from the exact values of the doubles."""
    bad, exact, _ = classes(mu, var)
    ys = [float(y) for y in np.ravel(ystar)]
    out = []
    with mpmath.workdps(DPS):
        for j, (m, v) in enumerate(zip(np.ravel(mu), np.ravel(var))):
            if bad[j]:
                out.append(mpmath.nan)
            elif exact[j]:
                out.append(mpmath.mpf(0))
            else:
                s = mpmath.sqrt(mpmath.mpf(float(v)))
                out.append(sum(h_mp((mpmath.mpf(float(m)) - mpmath.mpf(y)) / s) for y in ys) / len(ys))
    return out


def mean_mp(cols):
    """(1/S) sum_s per row for S lists of mpf: the marginal over S hyper samples."""
    with mpmath.workdps(DPS):
        return [sum(vs) / len(vs) for vs in zip(*cols)]


def scaled_errors(got, ref_mp):
    """|got - ref| / max(1, |ref|) per row, the difference taken in 50 digits; a NaN on both sides is 0, on one side inf."""
    out = []
    with mpmath.workdps(DPS):
        for g, r in zip(got, ref_mp):
            if mpmath.isnan(r) or np.isnan(g):
                out.append(0.0 if (mpmath.isnan(r) and np.isnan(g)) else np.inf)
            else:
                out.append(float(abs(mpmath.mpf(float(g)) - r) / max(mpmath.mpf(1), abs(r))))
    return np.array(out)


def nominee(scores):
    """TH's max over a list of mpf / floats: the first NaN wins, else the largest value, ties to the lowest index.  0-based."""
    best = None
    for j, v in enumerate(scores):
        if mpmath.isnan(v):
            return j
        if best is None or v > scores[best]:
            best = j
    return best


def top2_gap(scores):
    """The winner's lead over the runner-up (a float), NaN rows aside."""
    with mpmath.workdps(DPS):
        vals = sorted((v for v in scores if not mpmath.isnan(v)), reverse=True)
        return float(vals[0] - vals[1])


# ---- float64: the search's reference ---------------------------------------------------------------------------------------
def targets(K):
    """t_k = log1p(-u_k), u_k = (k - 1/2)/K, k = 1..K."""
    return np.log1p(-((np.arange(1, K + 1) - 0.5) / K))


def bracket(mu, var):
    """(lo0, hi0) over the live rows, each step one rounded operation: s = sqrt(var); t = s * 10; mu - t; mu + t; the minima."""
    _, _, live = classes(mu, var)
    m, v = np.asarray(mu, dtype=np.float64)[live], np.asarray(var, dtype=np.float64)[live]
    if m.size == 0:
        return np.nan, np.nan
    t = np.sqrt(v) * 10.0
    return float((m - t).min()), float((m + t).min())


def _terms(y, m, s):
    return special.log_ndtr((m - y) / s)


def log_survival(y, mu, var):
    """L(y) over the live rows: math.fsum of scipy's log_ndtr."""
    _, _, live = classes(mu, var)
    m, s = np.asarray(mu, dtype=np.float64)[live], np.sqrt(np.asarray(var, dtype=np.float64)[live])
    return math.fsum(_terms(y, m, s))


def ystar_ref(mu, var, K):
    """y*_k, k = 1..K, by bisection of L(y) = t_k from [lo0, hi0] down to adjacent doubles; the value returned is the upper one
    (the root lies in (lo, hi]: L(lo) > t_k >= L(hi)).  Rows whose term is exactly 0.0 at the current upper end are exactly 0.0
    at every y below it (log Phi is monotone and <= 0) and are dropped from the sum as the bracket shrinks: the same sums, fewer
    evaluations.  No live row: NaN."""
    _, _, live = classes(mu, var)
    m0, s0 = np.asarray(mu, dtype=np.float64)[live], np.sqrt(np.asarray(var, dtype=np.float64)[live])
    lo0, hi0 = bracket(mu, var)
    out = np.full(K, np.nan)
    if m0.size == 0:
        return out
    for k, t in enumerate(targets(K)):
        lo, hi, m, s = lo0, hi0, m0, s0
        while True:
            mid = lo + (hi - lo) / 2
            if mid <= lo or mid >= hi:
                break
            terms = _terms(mid, m, s)
            if math.fsum(terms) > t:
                lo = mid
            else:
                hi = mid
                keep = terms != 0.0
                if keep.sum() < 0.8 * m.size:
                    m, s = m[keep], s[keep]
        out[k] = hi
    return out


def ystar_bar(lo0, hi0, allowance):
    """|y* - ref| <= (RESOLUTION + allowance) * (hi0 - lo0): the last bracket's half width, derived, and a rounding allowance."""
    return (RESOLUTION + allowance) * (hi0 - lo0)


# ---- the distributions the search is checked on ------------------------------------------------------------------------------
def distribution(name, M):
    """(mu, var) of M rows.  u1..u3: mu ~ U(-2, 2), sigma log-uniform in [1e-3, 1], default_rng(1..3).  Boundary shapes:
    'one'   a single sharp row far below the rest (mu = -5, sigma = 1e-3): L is one term, steep in a sliver of the bracket
    'same'  every row (0, 1): L = M log Phi(-y), every partial sum alike
    'wide'  mu ~ U(-2e3, 2e3), sigma log-uniform in [1e-6, 1e2]: a bracket of width ~2e3 and terms of every scale"""
    if name in ("u1", "u2", "u3"):
        rng = np.random.default_rng(int(name[1]))
        mu = rng.uniform(-2.0, 2.0, M)
        sigma = np.exp(rng.uniform(math.log(1e-3), 0.0, M))
    elif name == "one":
        rng = np.random.default_rng(11)
        mu = rng.uniform(-2.0, 2.0, M)
        sigma = np.exp(rng.uniform(math.log(1e-3), 0.0, M))
        mu[M // 2], sigma[M // 2] = -5.0, 1e-3
    elif name == "same":
        mu, sigma = np.zeros(M), np.ones(M)
    elif name == "wide":
        rng = np.random.default_rng(13)
        mu = rng.uniform(-2e3, 2e3, M)
        sigma = np.exp(rng.uniform(math.log(1e-6), math.log(1e2), M))
    else:
        raise KeyError(name)
    return mu, sigma * sigma


# ---- float64: the score as the device writes it (bot7_amd/csrc/mes_math.h) -----------------------------------------------------
SQRT1_2 = 0.70710678118654752440
INV_SQRT_2PI = 0.39894228040143267794
SQRT_2_PI = 0.79788456080286535588


def h_np(g):
    """h(g) in float64 with scipy's erfc / erfcx: the same three branches (g > 0; -1 < g <= 0; g <= -1) and operation order as
    b7_mes_h."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        u = g * SQRT1_2
        pdf = np.exp((g * g) * -0.5) * INV_SQRT_2PI
        q = special.erfc(u) * 0.5
        cdf_lo = special.erfc(-u) * 0.5
        cdf = np.where(g > 0.0, 1.0 + (-q), cdf_lo)
        lcdf = np.where(g > 0.0, np.log1p(-q), np.log(cdf_lo))
        up = np.where(pdf == 0.0, 0.0, (g * (pdf / cdf)) * 0.5) + (-lcdf)
        e = special.erfcx(-u)
        lo = ((g * (SQRT_2_PI / e)) * 0.5 + (g * g) * 0.5) + (-np.log(e * 0.5))
        return np.where(g > -1.0, up, lo)
