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


def lowest_rows(own_alpha, n):
    """kg_rows_part_kernel's rule on the device's own means (S x M): the n lowest of ((mu_0 + mu_1) + ..) / S, the lower index
    first among equals, a NaN counting as +inf."""
    m = own_alpha[0].copy()
    for s in range(1, len(own_alpha)):
        m = m + own_alpha[s]
    m = m / float(len(own_alpha))
    return np.argsort(np.where(np.isnan(m), np.inf, m), kind="stable")[:n]


# ---- the lines held to exact arithmetic (tests/test_kg_exact_host.py, tests/test_gpu_kg_exact.py) -------------------------------
# What kg_kernel must return for one grid row x under one hyper sample, GIVEN the device's own W = inv(K) k(X, a_i) (diagnostic
# build: b7dbg_kg_operands), its own latent variance var(x) (b7_eval_posterior) and t's second operand fl(noise + jitter):
#     c_i(x) = k(x, a_i) - sum_j k(x, x_j) W_ji       k as (hi, lo) pairs from 50 digits on an exact argument, error-free products, exact sums
#     b_i = c_i / sqrt(t),  b_0 = var / sqrt(t),  t = var + fl(noise + jitter)                                       at 50 digits
# The bar of c_i, nothing of it from the device's output: gp_bar(e_np, scale_c) + dk(x, a_i) + sum_j |W_ji| dk_j, with scale_c =
# |k(x, a_i)| + sum_j |k(x, x_j) W_ji|, e_np numpy float64's own error on k_hi(x, a) - k_hi W over the judged rows, dk
# _post_ref.kstar_bound.  The bar of b_i: that over sqrt(t), plus SLOPE_ROUNDINGS u |b_i| for what follows c_i on the device: the add
# in t (u on t, u / 2 on b), the square root (within one ulp, 2 u) and the division (correctly rounded, u): 3.5 u, taken as 4.
# b_0 has those roundings alone.  bar / scale <= CAP on every judged row, scale = scale_c / sqrt(t).
import _exact as E  # noqa: E402
import _post_ref as PR  # noqa: E402
from _blr_ref import _dd_sum, _two_prod  # noqa: E402

U = 2.0 ** -53
CAP = PR.CAP
SLOPE_ROUNDINGS = 4.0
KL = 16
#               N    d   kernel        n  S   M     test_gpu_kg.CASES, then one per dpad class of kg_slab at N = 24
EXACT_CASES = [(5, 1, "ardse", 1, 1, 200), (64, 6, "ardmatern52", 5, 3, 257), (65, 33, "ardse", 16, 1, 200), (128, 6, "ardse", 16, 3, 257),
               (129, 65, "ardmatern52", 5, 1, 200), (300, 6, "ardse", 16, 1, 257), (300, 33, "ardmatern52", 1, 3, 200),
               (24, 3, "ardmatern52", 1, 2, 257), (24, 12, "ardse", 5, 2, 200), (24, 24, "ardmatern52", 16, 2, 257),
               (24, 40, "ardse", 1, 2, 200), (24, 60, "ardmatern52", 5, 2, 257), (24, 96, "ardse", 16, 2, 200)]
ROUTES_CASE = (150, 5, "ardse", 16, 3, 200)
#         name      N    d  S          the jitter redo: the small regime, the general layout, the general layout by d > 32
REDO = {"small": (40, 3, 3), "general": (150, 5, 3), "wide": (24, 33, 2)}


def exact_problem(N, d, M, S, n, dup=0):
    """tests/test_gpu_kg.py's problem and hyper samples at given sizes; grid rows 1, 16 and M - 2 are observations; the n rows of A
    are seeded, two of them among the judged rows 0 .. 16.  dup > 0: the last dup observations repeat the first dup, and the second
    hyper sample has noise 0 (the plain factorisation fails, the jitter schedule takes over)."""
    rng = np.random.default_rng(7 * N + d)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    if dup:
        X[N - dup:] = X[:dup]
    y = np.sin(3.0 * X.sum(axis=1, keepdims=True)) + X[:, -1:] ** 2 + 0.05 * rng.standard_normal((N, 1))
    if dup:
        y[N - dup:] = y[:dup]
    amp = float(np.var(y)) if N > 1 else 1.0
    hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-2 * amp, "mean": float(np.mean(y))}
    hyps = [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.3 * s), amp=hyp["amp"] * (1.0 + 0.2 * s), mean=hyp["mean"] + 0.05 * s,
                 noise=hyp["noise"] * (1.0 + 0.5 * s)) for s in range(S)]
    if dup:
        hyps[1] = dict(hyps[1], noise=0.0)
    Xc[1], Xc[16], Xc[M - 2] = X[0], X[N - 1], X[N // 2]
    pool = np.setdiff1d(np.arange(M), [0, 15])
    arows = np.sort(np.concatenate([[0, 15][:min(n, 2)], rng.choice(pool, size=max(n - 2, 0), replace=False)])).astype(np.int64)
    rows = np.unique(np.concatenate([PR.judged_rows(M), arows]))
    return X, y, Xc, hyps, arows, rows


class LineRef(object):
    __slots__ = ("b", "b0", "bar", "bar0", "scale", "e_np", "e_np_u", "share", "cap")


def lines_exact(X, Xs, A, hyp, kernel, W, var, tnoise):
    """Reference slopes of the rows Xs under one hyper sample: b (hi, lo) R x n, b0 (hi, lo) R, their bars and scale_c / sqrt(t).
    A: the n points of A; W: N x n; var: the R variances; tnoise: fl(noise + jitter)."""
    X, Xs, A, W = (np.asarray(v, dtype=np.float64) for v in (X, Xs, A, W))
    var = np.asarray(var, dtype=np.float64)
    ls, amp = hyp["lenscale_sq"], hyp["amp"]
    R, n = len(Xs), len(A)
    cov, covA = PR.true_cov_rows(Xs, X, ls, amp, kernel), PR.true_cov_rows(Xs, A, ls, amp, kernel)
    dk, dkA = PR.kstar_bound(cov, PR.arg_bound(Xs, X, ls), kernel), PR.kstar_bound(covA, PR.arg_bound(Xs, A, ls), kernel)
    ch, cl, scale_c = np.empty((R, n)), np.empty((R, n)), np.empty((R, n))
    for i in range(n):
        P, Er = _two_prod(cov.hi, W[None, :, i])
        Lm = cov.lo * W[None, :, i]
        for r in range(R):
            ch[r, i], cl[r, i] = _dd_sum([covA.hi[r, i], covA.lo[r, i]] + (-P[r]).tolist() + (-Er[r]).tolist() + (-Lm[r]).tolist())
        scale_c[:, i] = np.abs(covA.hi[:, i]) + np.abs(P).sum(1)
    ref = LineRef()
    ref.e_np = float(np.max(E.abs_errors(covA.hi - cov.hi @ W, ch, cl)))
    ref.e_np_u = ref.e_np / (U * float(scale_c.max()))   # numpy's error in u of the largest scale_c
    ks = dk @ np.abs(W) + dkA
    bar_c = E.gp_bar(ref.e_np, scale_c) + ks
    ref.share = ks / bar_c
    bh, bl, b0h, b0l = np.empty((R, n)), np.empty((R, n)), np.empty(R), np.empty(R)
    with mpmath.workdps(50):
        for r in range(R):
            rs = mpmath.sqrt(mpmath.mpf(float(var[r])) + mpmath.mpf(float(tnoise)))
            b0h[r], b0l[r] = E.mp_to_pair(mpmath.mpf(float(var[r])) / rs)
            for i in range(n):
                bh[r, i], bl[r, i] = E.mp_to_pair((mpmath.mpf(ch[r, i]) + mpmath.mpf(cl[r, i])) / rs)
    rt = np.sqrt(var + tnoise)[:, None]
    ref.b, ref.b0 = (bh, bl), (b0h, b0l)
    ref.bar = bar_c / rt + SLOPE_ROUNDINGS * U * np.abs(bh)
    ref.bar0 = SLOPE_ROUNDINGS * U * np.abs(b0h)
    ref.scale = scale_c / rt
    ref.cap = float(np.max(ref.bar / ref.scale))
    return ref


def judge_lines(ref, slopes, own):
    """error / bar of slopes (R x (n + 1), column 0 the own line) against the reference: (R x n ratios, R own-line ratios -- 0 where
    the row has no own line, which must then be a NaN)."""
    slopes = np.asarray(slopes, dtype=np.float64)
    r0 = np.where(own, E.abs_errors(slopes[:, 0], *ref.b0) / np.maximum(ref.bar0, 1e-300), np.where(np.isnan(slopes[:, 0]), 0.0, np.inf))
    return E.abs_errors(slopes[:, 1:], *ref.b) / ref.bar, r0


def kcol_ratio(X, A, hyp, kernel, kcol):
    """error / bar, entry by entry, of kcol (N x n) = k(x_j, a_i) against 50 digits: cov_entry_bar at the value the device's own
    argument can reach, plus the argument's counted roundings (_post_ref.kstar_bound)."""
    cov = PR.true_cov_rows(X, A, hyp["lenscale_sq"], hyp["amp"], kernel)
    return E.abs_errors(kcol, cov.hi, cov.lo) / PR.kstar_bound(cov, PR.arg_bound(X, A, hyp["lenscale_sq"]), kernel)


def w_residual(X, hyp, kernel, tnoise, kcol, W):
    """max_j |((K + tnoise I) W[:, i] - kcol[:, i])_j| per column in long double, and the bound 64 N 2^-53 ||K||_inf max |W[:, i]|."""
    N = len(X)
    K = cov_ld(X, X, hyp["lenscale_sq"], hyp["amp"], kernel)
    res = np.abs(K @ np.asarray(W, dtype=LD) + LD(tnoise) * np.asarray(W, dtype=LD) - np.asarray(kcol, dtype=LD)).max(axis=0)
    knorm = float(np.abs(K).sum(axis=1).max()) + tnoise
    return np.asarray(res, dtype=np.float64), 64.0 * N * U * knorm * np.abs(W).max(axis=0)


# ---- the device algebra restated in float64 (host tests) -------------------------------------------------------------------------
def host_operands(X, Xs, A, hyp, kernel, tnoise):
    """kcol (N x n), W (N x n) and the latent variance at Xs as the device makes them, in float64 with LAPACK."""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    K = PR.device_kstar(X, X, hyp["lenscale_sq"], hyp["amp"], kernel)
    K[np.diag_indices(len(X))] = hyp["amp"] + tnoise
    kcol = PR.device_kstar(X, A, hyp["lenscale_sq"], hyp["amp"], kernel)
    cf = cho_factor(K, lower=True)
    V = solve_triangular(np.tril(cf[0]), PR.device_kstar(Xs, X, hyp["lenscale_sq"], hyp["amp"], kernel).T, lower=True)
    return kcol, cho_solve(cf, kcol), hyp["amp"] - (V * V).sum(axis=0)


def lines_host(X, Xs, A, hyp, kernel, W, var, tnoise, wrong=None, Xs_next=None, ls0=None):
    """The float64 restatement of kg_kernel's slopes at the rows Xs: R x (n + 1), column 0 the own line.  wrong names one way the
    kernel goes wrong (tests/test_kg_exact_host.py): ("slab", start, width), ("swap", i), ("hql",) with Xs_next the neighbouring
    queries, ("ls0",) with ls0 sample 0's lengthscales in the k(x, a_i) tile, ("nojit", noise) with t = var + noise."""
    kind = wrong[0] if wrong else None
    ls, amp = hyp["lenscale_sq"], hyp["amp"]
    Ks = PR.device_kstar(Xs, X, ls, amp, kernel)
    if kind == "hql":
        w = 1.0 / np.asarray(ls, dtype=np.float64).ravel()
        hq, hk = 0.5 * ((Xs_next * Xs_next) @ w), 0.5 * ((X * X) @ w)
        arg = np.minimum(((Xs @ (X * w).T) - hq[:, None]) - hk[None, :], 0.0)
        sq = np.sqrt(-10.0 * arg)
        Ks = amp * np.exp(arg) if kernel == PR.SE else amp * (1.0 + sq * (1.0 + sq / 3.0)) * np.exp(-sq)
    if kind == "slab":
        Ks[:, wrong[1]:wrong[1] + wrong[2]] = 0.0
    W = np.array(W, dtype=np.float64)
    if kind == "swap":
        W[:, [wrong[1], wrong[1] + 1]] = W[:, [wrong[1] + 1, wrong[1]]]
    KA = PR.device_kstar(Xs, A, ls0 if kind == "ls0" else ls, amp, kernel)
    rs = np.sqrt(var + (wrong[1] if kind == "nojit" else tnoise))
    return np.concatenate([(var / rs)[:, None], (KA - Ks @ W) / rs[:, None]], axis=1)
