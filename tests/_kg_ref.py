"""References for the knowledge gradient (b7_kg_nominate / b7_kg_compute; bot7_amd/csrc/kg.hip).

  kg_mp          Frazier's sort-and-prune algorithm (Frazier, Powell & Dayanik 2009, algorithm 1) in mpmath at 50 digits: the
                 yardstick of the envelope arithmetic.
  kg_numpy       the library's O(L^2) form restated in numpy float64, one rounded operation per operator: the "how well can
                 float64 do" term of the envelope bar, and (fed with long-double slopes) the reference value vector of a nomination.
  posterior_ld   the GP posterior and its covariance against a set of rows in numpy long double (own Cholesky: numpy.linalg has
                 none at that precision): mu, var, cov(x, a_i).
  slopes_ref     alpha (S x n) and the slopes (S x M x (n + 1), column 0 the own line, NaN where the row is in A) from it.

The library minimises.  Lines (alpha_i, b_i); KG = min_i alpha_i - E[min_i (alpha_i + b_i Z)], Z ~ N(0, 1)."""
import math

import mpmath
import numpy as np

EPS = 2.0 ** -53
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ---- the envelope at 50 digits ----------------------------------------------------------------------------------------------
def kg_mp(alpha, b, dps=50):
    """One set of lines (1-d arrays; a NaN slope: the line takes no part) -> mpf.  Sort by slope (descending: the lower envelope is
    walked from z = -inf, where the steepest line is the lowest), among equal slopes keep the smallest intercept, prune the lines
    that never reach the envelope, then sum (b_k - b_k+1) f(-|c_k|) over the breakpoints c_k, f(z) = phi(z) + z Phi(z)."""
    with mpmath.workdps(dps):
        lines = [(mpmath.mpf(float(a)), mpmath.mpf(float(s))) for a, s in zip(alpha, b) if not math.isnan(float(s))]
        lines.sort(key=lambda t: (-t[1], t[0]))
        uniq = []
        for a, s in lines:
            if uniq and uniq[-1][1] == s:
                continue
            uniq.append((a, s))
        env, start = [], []   # the envelope's lines in order and where each one starts
        for a, s in uniq:
            while env:
                a0, s0 = env[-1]
                c = (a - a0) / (s0 - s)   # a0 + s0 z = a + s z
                if c <= start[-1]:
                    env.pop()
                    start.pop()
                    continue
                env.append((a, s))
                start.append(c)
                break
            if not env:
                env.append((a, s))
                start.append(mpmath.mpf("-inf"))
        total = mpmath.mpf(0)
        for k in range(1, len(env)):
            c = -abs(start[k])
            total += (env[k - 1][1] - env[k][1]) * (mpmath.npdf(c) + c * mpmath.ncdf(c))
        return total


def kg_mp_rows(alpha, b):
    """kg_mp per row -> (hi, lo) float64 arrays with hi + lo the 50-digit value to ~1e-32 relative."""
    hi, lo = np.empty(len(alpha)), np.empty(len(alpha))
    for r in range(len(alpha)):
        v = kg_mp(alpha[r], b[r])
        hi[r] = float(v)
        with mpmath.workdps(50):
            lo[r] = float(v - mpmath.mpf(hi[r]))
    return hi, lo


def err_vs_mp(got, hi, lo):
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


# ---- the library's form in float64 ----------------------------------------------------------------------------------------------
def _f(z):
    pdf = np.exp((z * z) * -0.5) * 0.39894228040143267794
    cdf = _erfc(z * -0.70710678118654752440) * 0.5
    return np.maximum(pdf + z * cdf, 0.0)


def kg_numpy(alpha, b, want_cond=False):
    """alpha, b: M1 x L, column 0 the own line (index 0 wins ties), a NaN slope: the line takes no part.  Line i lives on
    [lo_i, hi_i]: hi_i = min over the flatter lines j of (alpha_j - alpha_i) / (b_i - b_j) (the flattest among equal quotients takes
    over), lo_i = max over the steeper ones of (alpha_i - alpha_j) / (b_j - b_i); equal slopes keep the smaller intercept, then the
    lower index.  Sum of (b_i - b_next) f(-|hi_i|) over the lines with lo_i < hi_i < inf: lanes 1 .. 16 by the tree 1, 2, 4, 8, the own
    line's term last.  want_cond: also sum term_i (1 + hi_i^2)^2, what the rounding error of each term grows with."""
    a, b = np.asarray(alpha, dtype=np.float64), np.asarray(b, dtype=np.float64)
    M1, L = a.shape
    act = ~np.isnan(b)
    ai, aj, bi, bj = a[:, :, None], a[:, None, :], b[:, :, None], b[:, None, :]
    on = act[:, None, :] & act[:, :, None]
    idx = np.arange(L)
    j_first = (idx[None, :] < idx[:, None])[None]
    with np.errstate(all="ignore"):
        below, above = on & (bj < bi), on & (bj > bi)
        z = np.where(below, (aj - ai) / (bi - bj), np.where(above, (ai - aj) / (bj - bi), np.nan))
        hi = np.where(below, z, np.inf).min(axis=2)
        bn = np.where(below & (z == hi[:, :, None]), bj, np.inf).min(axis=2)
        lo = np.where(above, z, -np.inf).max(axis=2)
        dead = (on & (bj == bi) & ((aj < ai) | ((aj == ai) & j_first))).any(axis=2) | ~act
        inn = ~dead & (lo < hi) & (hi < np.inf)
        zz = np.where(inn, -np.abs(hi), 0.0)
        term = np.where(inn, (b - np.where(inn, bn, 0.0)) * _f(zz), 0.0)
        cond = np.where(inn, term * (1.0 + zz * zz) ** 2, 0.0).sum(axis=1)
    lanes = np.zeros((M1, 16))
    lanes[:, :L - 1] = term[:, 1:]
    for o in (1, 2, 4, 8):
        lanes = lanes + lanes[:, np.arange(16) ^ o]
    out = lanes[:, 0] + term[:, 0]
    return (out, cond) if want_cond else out


def closed_form_two(alpha, b):
    """L = 2 at 50 digits: |b_0 - b_1| f(-|alpha_0 - alpha_1| / |b_0 - b_1|) -> (hi, lo)."""
    hi, lo = np.empty(len(alpha)), np.empty(len(alpha))
    with mpmath.workdps(50):
        for r in range(len(alpha)):
            a0, a1, b0, b1 = (mpmath.mpf(float(v)) for v in (alpha[r, 0], alpha[r, 1], b[r, 0], b[r, 1]))
            if b0 == b1:
                v = mpmath.mpf(0)
            else:
                c = -abs(a0 - a1) / abs(b0 - b1)
                v = abs(b0 - b1) * (mpmath.npdf(c) + c * mpmath.ncdf(c))
            hi[r] = float(v)
            lo[r] = float(v - mpmath.mpf(hi[r]))
    return hi, lo


def envelope_cases(M1=65, seed=20):
    """name -> (alpha, b), M1 rows each: the cases of the envelope test."""
    rng = np.random.default_rng(seed)
    out = {}
    for L in (1, 2, 3, 16, 17):
        out["L%d" % L] = (rng.standard_normal((M1, L)), rng.standard_normal((M1, L)) * rng.choice([0.05, 1.0, 3.0], (M1, 1)))
    a, b = rng.standard_normal((M1, 9)), np.round(rng.standard_normal((M1, 9)), 1)   # slopes from a coarse lattice: many are equal
    out["duplicated slopes"] = (a, b)
    a, b = rng.standard_normal((M1, 12)), rng.standard_normal((M1, 12))
    a[:, 6:], b[:, 6:] = a[:, :6], b[:, :6]                                           # every line twice
    out["duplicated lines"] = (a, b)
    # three lines through one point: slopes, z0 and y0 on a dyadic lattice, alpha_i = y0 - b_i z0 exactly
    b3 = rng.integers(-16, 17, (M1, 3)) / 4.0
    b3[:, 1] = np.where(b3[:, 1] == b3[:, 0], b3[:, 0] + 0.25, b3[:, 1])
    b3[:, 2] = np.where((b3[:, 2] == b3[:, 0]) | (b3[:, 2] == b3[:, 1]), b3[:, :2].max(axis=1) + 0.5, b3[:, 2])
    z0, y0 = rng.integers(-8, 9, (M1, 1)) / 4.0, rng.integers(-32, 33, (M1, 1)) / 16.0
    a3 = y0 - b3 * z0
    extra_a, extra_b = y0 + np.abs(rng.standard_normal((M1, 2))) + 0.5 + 3.0 * np.abs(z0), rng.integers(-2, 3, (M1, 2)) / 4.0
    out["three lines through one point"] = (np.hstack([a3, extra_a]), np.hstack([b3, extra_b]))
    out["all slopes zero"] = (rng.standard_normal((M1, 17)), np.zeros((M1, 17)))
    scale = 10.0 ** np.linspace(-8.0, 8.0, M1)[:, None]
    out["slope scales 1e-8 .. 1e8"] = (rng.standard_normal((M1, 10)), rng.standard_normal((M1, 10)) * scale)
    a, b = rng.standard_normal((M1, 8)), rng.standard_normal((M1, 8))
    a[:, 5] += 1e6
    out["one dominated line far above"] = (a, b)
    return out


# ---- the posterior covariance in long double ---------------------------------------------------------------------------------------
LD = np.longdouble


def cov_ld(X, Z, lenscale_sq, amp, kernel="ardse"):
    X, Z = np.asarray(X, dtype=LD), np.asarray(Z, dtype=LD)
    w = LD(1.0) / np.asarray(lenscale_sq, dtype=LD).ravel()
    D = np.zeros((len(X), len(Z)), dtype=LD)
    for k in range(X.shape[1]):
        D += (X[:, k][:, None] - Z[:, k][None, :]) ** 2 * w[k]
    if kernel == "ardse":
        return LD(amp) * np.exp(LD(-0.5) * D)
    s = np.sqrt(LD(5.0) * D)
    return LD(amp) * (LD(1.0) + s + s * s / LD(3.0)) * np.exp(-s)


def chol_ld(K):
    L = np.array(K, dtype=LD)
    n = len(L)
    for j in range(n):
        L[j, j] = np.sqrt(L[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        L[j, j + 1:] = 0
    return L


def solve_lower_ld(L, B):
    """inv(L) B, B n x m, by forward substitution."""
    Y = np.array(B, dtype=LD)
    for i in range(len(L)):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def posterior_ld(X, y, Xs, hyp, kernel, rows0, jitter=0.0):
    """One hyper sample: mu[M], var[M] (latent), C[M][n] = cov(f(x), f(a_i) | data) for the grid rows rows0 (0-based), long double."""
    y = np.asarray(y, dtype=LD).ravel()
    N = len(X)
    K = cov_ld(X, X, hyp["lenscale_sq"], hyp["amp"], kernel) + (LD(hyp["noise"]) + LD(max(float(jitter), 0.0))) * np.eye(N, dtype=LD)
    L = chol_ld(K)
    Ks = cov_ld(Xs, X, hyp["lenscale_sq"], hyp["amp"], kernel)          # M x N
    V = solve_lower_ld(L, Ks.T)                                          # N x M: inv(L) K*'
    r = solve_lower_ld(L, (y - LD(hyp["mean"]))[:, None])[:, 0]
    mu = LD(hyp["mean"]) + V.T @ r
    var = LD(hyp["amp"]) - (V * V).sum(axis=0)
    A = np.asarray(Xs)[np.asarray(rows0, dtype=int)]
    C = cov_ld(Xs, A, hyp["lenscale_sq"], hyp["amp"], kernel) - V.T @ V[:, np.asarray(rows0, dtype=int)]
    return mu, var, C


def slopes_ref(X, y, Xs, hyps, kernel, rows0=None, n=None, jitter=0.0):
    """-> rows0 (the given ones, or the n rows of lowest marginal mean, ties to the lowest index), alpha S x n, slopes S x M x (n + 1)
    (column 0 the own line var / sqrt(var + noise + jitter): NaN where the row is in A), mu S x M; float64 roundings of long double."""
    S, M = len(hyps), len(Xs)
    jit = np.broadcast_to(np.asarray(jitter, dtype=np.float64), (S,))
    if rows0 is None:
        mus = [posterior_ld(X, y, Xs, h, kernel, [0], jit[s])[0] for s, h in enumerate(hyps)]
        mbar = sum(mus[1:], mus[0]) / LD(S)
        rows0 = np.argsort(np.asarray(mbar, dtype=np.float64), kind="stable")[:n]
    rows0 = np.asarray(rows0, dtype=int)
    n = len(rows0)
    alpha, slopes, mu_all = np.empty((S, n)), np.empty((S, M, n + 1)), np.empty((S, M))
    for s, h in enumerate(hyps):
        mu, var, C = posterior_ld(X, y, Xs, h, kernel, rows0, jit[s])
        rs = np.sqrt(var + LD(h["noise"]) + LD(max(float(jit[s]), 0.0)))
        alpha[s] = np.asarray(mu[rows0], dtype=np.float64)
        slopes[s, :, 1:] = np.asarray(C / rs[:, None], dtype=np.float64)
        slopes[s, :, 0] = np.asarray(var / rs, dtype=np.float64)
        slopes[s, rows0, 0] = np.nan
        mu_all[s] = np.asarray(mu, dtype=np.float64)
    return rows0, alpha, slopes, mu_all


def values_ref(alpha, slopes, mu):
    """The per-sample knowledge gradient S x M of reference alpha / slopes / mu (kg_numpy on the n + 1 lines of every row)."""
    S, M, L = slopes.shape
    out = np.empty((S, M))
    for s in range(S):
        a = np.empty((M, L))
        a[:, 0], a[:, 1:] = mu[s], alpha[s][None, :]
        out[s] = kg_numpy(a, slopes[s])
    return out


def nominee_ref(marginal):
    """b7_eval_nominate's rule: the first NaN, else the maximum, ties to the lowest index (0-based)."""
    nan = np.flatnonzero(np.isnan(marginal))
    return int(nan[0]) if len(nan) else int(np.argmax(marginal))
