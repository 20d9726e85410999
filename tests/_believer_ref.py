"""Float64 numpy references for kriging-believer batch nomination (tests/test_believer_host.py, tests/test_gpu_believer.py):
the rank-one variance downdate as include/bot7hip.h states it, the refit it must equal (the believed point appended to the data
at its own posterior mean), the three acquisition scores as bot7_amd/csrc/score.hip evaluates them, and the greedy pick sequence
with its top-2 gaps; and the same refit in 50-digit arithmetic (believer_truth), the truth both the float64 restatements and the
device are measured against.  No GPU needed here."""
import mpmath
import numpy as np
from scipy import special
from scipy.linalg import cholesky, solve_triangular


def cov(X, Z, lenscale_sq, amp, kernel="ardse"):
    """k(X, Z) from the differences: D = sum_k (x_k - z_k)^2 / lenscale_sq_k; ARD-SE amp exp(-D/2), ARD Matern-5/2
    amp (1 + s + s^2/3) exp(-s) with s = sqrt(5 D)."""
    X, Z = np.atleast_2d(np.asarray(X, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    w = 1.0 / np.asarray(lenscale_sq, dtype=np.float64).ravel()
    D = np.einsum("ijk,k->ij", (X[:, None, :] - Z[None, :, :]) ** 2, w)
    if kernel == "ardse":
        return amp * np.exp(-0.5 * D)
    s = np.sqrt(5.0 * D)
    return amp * (1.0 + s + s * s / 3.0) * np.exp(-s)


class Posterior(object):
    """GP regression of (X, y) under one hyper sample: mean and LATENT variance over the candidates Xc."""

    def __init__(self, X, y, Xc, hyp, kernel="ardse"):
        self.X, self.Xc, self.hyp, self.kernel = np.asarray(X, dtype=np.float64), np.asarray(Xc, dtype=np.float64), hyp, kernel
        ls, amp = hyp["lenscale_sq"], hyp["amp"]
        K = cov(self.X, self.X, ls, amp, kernel) + hyp["noise"] * np.eye(len(self.X))
        self.L = cholesky(K, lower=True)
        r = np.asarray(y, dtype=np.float64).ravel() - hyp["mean"]
        self.alpha = solve_triangular(self.L, solve_triangular(self.L, r, lower=True), lower=True, trans="T")
        self.Ks = cov(self.Xc, self.X, ls, amp, kernel)
        self.mu = hyp["mean"] + self.Ks @ self.alpha
        V = solve_triangular(self.L, self.Ks.T, lower=True)
        self.var = amp - np.einsum("ij,ij->j", V, V)


class Believer(object):
    """The recurrence, one hyper sample: after believe(j1), .var is the variance given every believed row so far; .mu never moves.
      c_j(x) = k(x, x_j) - K*(x, X) w_j,  w_j = inv(K) k(X, x_j);  u_j = (c_j - sum_{i<j} u_i u_i(x_j)) / sqrt(var(x_j) + noise)"""

    def __init__(self, X, y, Xc, hyp, kernel="ardse"):
        self.p = Posterior(X, y, Xc, hyp, kernel)
        self.mu, self.var, self.u = self.p.mu, self.p.var.copy(), []

    def believe(self, row0):
        p, h = self.p, self.p.hyp
        kj = cov(p.X, p.Xc[row0], h["lenscale_sq"], h["amp"], p.kernel).ravel()
        w = solve_triangular(p.L, solve_triangular(p.L, kj, lower=True), lower=True, trans="T")
        c = cov(p.Xc, p.Xc[row0], h["lenscale_sq"], h["amp"], p.kernel).ravel() - p.Ks @ w
        for ui in self.u:
            c = c - ui * ui[row0]
        u = c / np.sqrt(self.var[row0] + h["noise"])
        self.u.append(u)
        self.var = self.var - u * u


def refit(X, y, Xc, hyp, kernel, rows0):
    """The GP the believer stands for: the rows rows0 of Xc appended to the data one after the other, each observed at the
    posterior mean the model had just before it.  Returns (mu, var) over Xc after the last of them."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
    p = Posterior(X, y, Xc, hyp, kernel)
    for r in rows0:
        X, y = np.vstack([X, np.asarray(Xc)[r]]), np.append(y, p.mu[r])
        p = Posterior(X, y, Xc, hyp, kernel)
    return p.mu, p.var


# ---- the refit at 50 digits --------------------------------------------------------------------------------------------------
def believer_truth(X, y, Xc, hyp, kernel, rows0, probes, after=None, jitter=0.0, dps=50):
    """The GP the believer stands for, in dps-digit arithmetic: the rows rows0 of Xc appended to the data one after the other, each
    observed at the posterior mean of the model just before it; K + (noise + jitter) I on the diagonal, believed rows included.
    Returns {j: (mu, var)} for every j in `after` (default: len(rows0) only): the posterior mean and LATENT variance at the rows
    `probes` of Xc once the first j of rows0 are believed, as lists of mpf.  ARD-SE amp exp(-D/2); ARD Matern-5/2
    amp (1 + s + s^2/3) exp(-s), s = sqrt(5 D) (tests/_matern_ref.py), D = sum_k (x_k - z_k)^2 / lenscale_sq_k from the float64
    inputs.  One factorisation serves every j: the factor of the first N + j points is the leading block of the factor of all of
    them, and so are inv(L) k and inv(L) (y - mean)."""
    X, Xc = np.asarray(X, dtype=np.float64), np.asarray(Xc, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    rows0 = [int(r) for r in rows0]
    after = [len(rows0)] if after is None else sorted(int(j) for j in after)
    N, d, q = X.shape[0], X.shape[1], len(rows0)
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        ls = [mpf(float(v)) for v in np.asarray(hyp["lenscale_sq"], dtype=np.float64).ravel()]
        A, m = mpf(float(hyp["amp"])), mpf(float(hyp["mean"]))
        diag = mpf(float(hyp["noise"])) + mpf(float(jitter))
        pts = [[mpf(float(v)) for v in r] for r in np.vstack([X, Xc[rows0].reshape(q, d)])]

        def k(a, b):
            D = mpmath.fsum((a[i] - b[i]) ** 2 / ls[i] for i in range(d))
            if kernel == "ardse":
                return A * mpmath.exp(-D / 2)
            s = mpmath.sqrt(5 * D)
            return A * (1 + s + s * s / 3) * mpmath.exp(-s)

        # row-by-row Cholesky of the (N + q)-point K; t = inv(L) (y - mean), the believed values made on the way
        n = N + q
        L = [[mpf(0)] * n for _ in range(n)]
        t = []
        for i in range(n):
            for j in range(i + 1):
                kij = k(pts[i], pts[j]) + (diag if i == j else 0)
                acc = kij - mpmath.fsum(L[i][c] * L[j][c] for c in range(j))
                L[i][j] = mpmath.sqrt(acc) if i == j else acc / L[j][j]
            # the response of point i less the mean: the data's, or the posterior mean of the first i points at a believed row,
            # k' inv(K) r = (inv(L) k) . (inv(L) r), whose inv(L) k is row i of L itself
            r = (mpf(float(y[i])) - m) if i < N else mpmath.fsum(L[i][c] * t[c] for c in range(i))
            t.append((r - mpmath.fsum(L[i][c] * t[c] for c in range(i))) / L[i][i])
        out = {j: ([], []) for j in after}
        for p in probes:
            z = [mpf(float(v)) for v in Xc[int(p)]]
            v = []
            for i in range(n):
                v.append((k(z, pts[i]) - mpmath.fsum(L[i][c] * v[c] for c in range(i))) / L[i][i])
            for j in after:
                out[j][0].append(m + mpmath.fsum(v[c] * t[c] for c in range(N + j)))
                out[j][1].append(A - mpmath.fsum(v[c] ** 2 for c in range(N + j)))
        return out


def err_vs_truth(got, truth):
    """max |got - truth| over a float64 vector and a list of mpf, evaluated at the truth's precision."""
    with mpmath.workdps(50):
        return float(max(abs(mpmath.mpf(float(g)) - tv) for g, tv in zip(np.asarray(got, dtype=np.float64).ravel(), truth)))


# ---- the scores, as score.hip evaluates them ---------------------------------------------------------------------------------
def _erf_as(x):   # utils/math.lua:261-288 (Abramowitz & Stegun 7.1.26), the operation order of b7_erf
    c1, c2, c3, c4, c5, p = 0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429, 0.3275911
    t = 1.0 / ((np.abs(x) * p) + 1.0)
    r = ((((t * c5 + c4) * t + c3) * t + c2) * t + c1) * t
    return (1.0 - r * np.exp(-(x * x))) * np.where(x >= 0.0, 1.0, -1.0)


def score(kind, mu, var, fmin=None, tradeoff=0.0, upper=False, sign=-1.0):
    """One hyper sample's score per candidate: "ei", "cb" or "logei"."""
    with np.errstate(all="ignore"):
        sigma = np.sqrt(var)
        if kind == "cb":
            v = mu + sigma * tradeoff if upper else mu - sigma * tradeoff
            return v if sign > 0.0 else -v
        imprv = (fmin - mu) - tradeoff
        z = imprv / sigma
        if kind == "ei":
            cdf = (_erf_as(z * 0.70710678118654746) + 1.0) * 0.5
            pdf = np.exp(z * z * -0.5) * 0.3989422804014327
            return np.maximum(imprv * cdf + sigma * pdf, 0.0)
        lh = np.where(z > -1.0, np.log(np.exp(-0.5 * z * z) * 0.39894228040143267794 + z * special.ndtr(z)),
                      -0.5 * z * z - 0.91893853320467274178 +
                      np.log1p(-(-z * 1.2533141373155002512) * special.erfcx(-z * 0.70710678118654752440)))
        return np.log(sigma) + lh


def marginal(kind, per_sample):
    """score:add over the samples and score:div: the mean (EI, CB) or log-mean-exp (LogEI)."""
    A = np.asarray(per_sample, dtype=np.float64)
    if kind == "logei":
        return special.logsumexp(A, axis=0) - np.log(A.shape[0])
    return A.sum(axis=0) / A.shape[0]


def top2(scores, picked0):
    """(arg-max, gap to the runner-up) with the rows picked0 left out (TH order: the first maximum)."""
    s = np.array(scores, dtype=np.float64)
    s[list(picked0)] = -np.inf
    best = int(np.argmax(s))
    rest = s.copy()
    rest[best] = -np.inf
    return best, float(s[best] - rest.max())


def greedy(X, y, Xc, hyps, kernel, q, kind, how="downdate", **spec):
    """The q greedy picks (0-based rows), the marginal score vector of every pick, its top-2 gap and the per-sample variances
    before every pick; how: "downdate" (the recurrence) or "refit" (the (N + j)-point GPs it must equal)."""
    picks, scores, gaps, variances = [], [], [], []
    bel = [Believer(X, y, Xc, h, kernel) for h in hyps]
    for j in range(q):
        if how == "refit" and j > 0:
            mv = [refit(X, y, Xc, h, kernel, picks) for h in hyps]
        else:
            mv = [(b.mu, b.var) for b in bel]
        sc = marginal(kind, [score(kind, m, v, **spec) for m, v in mv])
        best, gap = top2(sc, picks)
        variances.append([np.array(v) for _, v in mv])
        picks.append(best), scores.append(sc), gaps.append(gap)
        if how == "downdate":
            for b in bel:
                b.believe(best)
    return picks, scores, gaps, variances
