"""The probit GP classifier by Laplace's method (csrc/laplace.hip), stated once on the host: the float64 restatement of the rule the
device follows, the same rule in numpy.longdouble with a hand-written Cholesky (the truth for N > 24), and the 50-digit solution of
the mode equation f = mean + K g(f) (the truth for N <= 24).  Checked on the CPU by tests/test_laplace_host.py; the yardsticks of
tests/test_gpu_laplace.py come from here.

Labels v in {0, 1}, 1 = VIOLATED; s = 2 v - 1; Pr[v = 1 | h] = Phi(h).  Hyper vector [lenscale_sq_1..d, amp, noise, mean]: noise is
ignored, mean is the latent's constant prior mean.  K has no diagonal term.
    start       a = 0, f = mean, psi(a, f) = -a'(f - mean)/2 + sum log Phi(s f)
    it = 1..32  rho = phi/Phi at s f, g = s rho, W = max(rho (rho + s f), 0), B = I + W^1/2 K W^1/2 = L L', b = W (f - mean) + g,
                a+ = b - W^1/2 L^-T L^-1 W^1/2 K b, delta = |a+ - a|_inf;  delta <= 2^-26 max(1, |a+|_inf): a = a+, stop, converged;
                else the first t of 1, 1/2, .., 2^-10 with psi(a + t (a+ - a)) >= psi(a), the last one if none.  Always f = mean + K a.
    afterwards  rho, W, B, L at f^;  Linv = L^-1 W^1/2, alpha = a, nll = -(psi(a, f^) - sum log L_ii).
The latent posterior at x*: mu = mean + k*' a, var = amp - |Linv k*|^2."""
import functools

import mpmath
import numpy as np
from scipy import special
from scipy.linalg import solve_triangular

ITMAX, HALVINGS, TOL = 32, 10, 2.0 ** -26
EPS = 2.0 ** -52
SE, MATERN = "ardse", "ardmatern52"
DPS = 50


# ---- covariance ---------------------------------------------------------------------------------------------------------------
def cov(X, Z, lenscale_sq, amp, kern, dtype=np.float64):
    """K(X, Z) without a diagonal term: amp exp(-D/2) (ARD-SE) or amp (1 + s + s^2/3) exp(-s), s = sqrt(5 D) (Matern-5/2),
    D = sum_k (x_k - z_k)^2 / lenscale_sq_k, in the difference form, in dtype."""
    X, Z = np.asarray(X, dtype=dtype), np.asarray(Z, dtype=dtype)
    w = np.asarray(lenscale_sq, dtype=dtype)
    diff = X[:, None, :] - Z[None, :, :]
    D = np.sum(diff * diff / w, axis=2)
    amp = dtype(amp)
    if kern == SE:
        return amp * np.exp(-D / dtype(2))
    s = np.sqrt(dtype(5) * D)
    return amp * (dtype(1) + s + s * s / dtype(3)) * np.exp(-s)


def cov_mp(X, Z, lenscale_sq, amp, kern):
    """The same from the float64 inputs themselves in DPS-digit arithmetic (mpmath.matrix)."""
    out = mpmath.matrix(len(X), len(Z))
    w = [mpmath.mpf(float(v)) for v in lenscale_sq]
    for i, x in enumerate(X):
        for j, z in enumerate(Z):
            D = mpmath.fsum((mpmath.mpf(float(a)) - mpmath.mpf(float(b))) ** 2 / wk for a, b, wk in zip(x, z, w))
            if kern == SE:
                out[i, j] = mpmath.mpf(float(amp)) * mpmath.exp(-D / 2)
            else:
                s = mpmath.sqrt(5 * D)
                out[i, j] = mpmath.mpf(float(amp)) * (1 + s + s * s / 3) * mpmath.exp(-s)
    return out


# ---- the probit pieces --------------------------------------------------------------------------------------------------------
def logcdf(z):
    """log Phi(z), the device's three branches (csrc/probit_math.h) in float64."""
    z = np.asarray(z, dtype=np.float64)
    u = z * 0.70710678118654752440
    with np.errstate(all="ignore"):
        return np.where(z > 0.0, np.log1p(special.erfc(u) * -0.5),
                        np.where(z > -1.0, np.log(special.erfc(-u) * 0.5), (z * z) * -0.5 + np.log(special.erfcx(-u) * 0.5)))


def ratio(z):
    """phi(z)/Phi(z) = sqrt(2/pi) / erfcx(-z/sqrt2)."""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(all="ignore"):
        return 0.79788456080286535588 / special.erfcx(z * -0.70710678118654752440)


def wfun(z, rho):
    """W(z) = rho (rho + z) for z > -6; below, rho + z from the continued fraction 1/(t + 2/(t + 3/(t + .. + 24/t))), t = -z (no
    cancellation); clamped at 0 from below."""
    z, rho = np.asarray(z, dtype=np.float64), np.asarray(rho, dtype=np.float64)
    t = np.where(z > -6.0, 6.0, -z)
    v = t.copy()
    for k in range(24, 1, -1):
        v = t + k / v
    with np.errstate(all="ignore"):
        w = np.where(z > -6.0, rho * (rho + z), rho * (1.0 / v))
    return np.where(w > 0.0, w, 0.0)


def pieces_mp(z):
    """(log Phi, phi/Phi, W) at one z in DPS digits."""
    z = mpmath.mpf(z)
    if z < -5:
        # Phi(z) = erfc(-z/sqrt2)/2 keeps its relative accuracy on the left; rho + z cancels 2 log10|z| digits: 40 guard digits cover 1e6
        with mpmath.workdps(DPS + 40):
            cdf = mpmath.erfc(-z / mpmath.sqrt(2)) / 2
            lp = mpmath.log(cdf)
            rho = mpmath.npdf(z) / cdf if cdf != 0 else -z
            return lp, rho, rho * (rho + z)
    cdf = mpmath.ncdf(z)
    rho = mpmath.npdf(z) / cdf
    return mpmath.log(cdf), rho, rho * (rho + z)


def _to_long(v):
    hi = float(v)
    return np.longdouble(hi) + np.longdouble(float(v - hi))


def pieces(z, dtype=np.float64):
    """(log Phi(z), rho(z), W(z)) elementwise; float64: the formulas above; longdouble: DPS-digit values rounded to longdouble."""
    if dtype is np.float64:
        r = ratio(z)
        return logcdf(z), r, wfun(z, r)
    out = np.empty((3, len(z)), dtype=np.longdouble)
    with mpmath.workdps(DPS):
        for i, zi in enumerate(z):
            zz = mpmath.mpf(float(zi)) + mpmath.mpf(float(zi - np.longdouble(float(zi))))
            p = pieces_mp(zz)
            out[:, i] = [_to_long(p[0]), _to_long(p[1]), _to_long(max(p[2], 0))]
    return out[0], out[1], out[2]


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def chol_loop(B):
    """Lower Cholesky factor by a hand-written loop in B's own dtype (numpy has no longdouble LAPACK)."""
    n = B.shape[0]
    L = np.zeros_like(B)
    for j in range(n):
        d = np.sqrt(B[j, j] - np.dot(L[j, :j], L[j, :j]))
        L[j, j] = d
        if j + 1 < n:
            L[j + 1:, j] = (B[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / d
    return L


def tri_solve(L, r, trans=False):
    """L x = r (or L' x = r) by substitution in L's dtype."""
    n = L.shape[0]
    x = np.array(r, dtype=L.dtype, copy=True).reshape(n, -1)   # (one column per right-hand side)
    if not trans:
        for j in range(n):
            x[j] = x[j] / L[j, j]
            x[j + 1:] = x[j + 1:] - L[j + 1:, j:j + 1] * x[j][None, :]
    else:
        for j in range(n - 1, -1, -1):
            x[j] = x[j] / L[j, j]
            x[:j] = x[:j] - L[j, :j][:, None] * x[j][None, :]
    return x.reshape(np.shape(r))


def _factor(B):
    return np.linalg.cholesky(B) if B.dtype == np.float64 else chol_loop(B)


def _solve(L, r, trans=False):
    if L.dtype == np.float64:
        return solve_triangular(L, r, lower=True, trans="T" if trans else "N", check_finite=False)
    return tri_solve(L, r, trans)


def laplace_fit(K, labels, mean, dtype=np.float64):
    """The rule on K (N x N, no diagonal term), labels (0 / 1) and the prior mean, in dtype.  Returns dict(f, a, W, sw, L, nll, psi,
    iters, converged, psi_trace (psi after every accepted step, the start first), halvings (per iteration))."""
    K = np.asarray(K, dtype=dtype)
    n = K.shape[0]
    s = (2.0 * np.asarray(labels, dtype=np.float64) - 1.0).astype(dtype)
    mean = dtype(mean)
    I = np.eye(n, dtype=dtype)

    def psi_of(a, f):
        return dtype(-0.5) * np.dot(a, f - mean) + np.sum(pieces(s * f, dtype)[0])

    a, f = np.zeros(n, dtype=dtype), np.full(n, mean, dtype=dtype)
    psi = psi_of(a, f)
    trace, halvings, iters, converged = [psi], [], 0, False
    for it in range(1, ITMAX + 1):
        iters = it
        _, rho, W = pieces(s * f, dtype)
        sw = np.sqrt(W)
        L = _factor(I + sw[:, None] * K * sw[None, :])
        b = W * (f - mean) + s * rho
        an = b - sw * _solve(L, _solve(L, sw * (K @ b)), trans=True)
        delta, nrm = np.max(np.abs(an - a)), np.max(np.abs(an))
        if delta <= TOL * max(1.0, nrm):
            a = an
            f = mean + K @ a
            psi = psi_of(a, f)
            trace.append(psi)
            converged = True
            halvings.append(0)
            break
        t = dtype(1)
        for h in range(HALVINGS + 1):
            at = a + t * (an - a)
            ft = mean + K @ at
            pt = psi_of(at, ft)
            if pt >= psi or h == HALVINGS:
                break
            t = t * dtype(0.5)
        a, f, psi = at, ft, pt
        trace.append(psi)
        halvings.append(h)
    _, rho, W = pieces(s * f, dtype)
    sw = np.sqrt(W)
    L = _factor(I + sw[:, None] * K * sw[None, :])
    nll = -(psi - np.sum(np.log(np.diag(L))))
    return {"f": f, "a": a, "W": W, "sw": sw, "L": L, "nll": nll, "psi": psi, "iters": iters, "converged": converged,
            "psi_trace": trace, "halvings": halvings, "g": s * rho}


def posterior(Ks, amp, mean, fit):
    """Latent mean and variance at the rows of Ks = K(X*, X): mean + Ks a, amp - |L^-1 W^1/2 Ks'|^2, in the fit's dtype."""
    dtype = fit["a"].dtype.type
    Ks = np.asarray(Ks, dtype=dtype)
    mu = dtype(mean) + Ks @ fit["a"]
    V = _solve(fit["L"], (Ks * fit["sw"][None, :]).T)
    return mu, dtype(amp) - np.sum(V * V, axis=0)


# ---- the 50-digit truth -------------------------------------------------------------------------------------------------------
def mp_mode(Kmp, labels, mean, f0):
    """Newton on F(f) = f - mean - K g(f) in DPS digits from the float64 mode f0 (J = I + K W).  Returns dict(f, a, W, nll) of mpf
    lists / values; a = g(f^), nll = -(psi - log det(B)/2)."""
    n = len(labels)
    s = [2 * int(v) - 1 for v in labels]
    mean = mpmath.mpf(float(mean))
    f = mpmath.matrix([mpmath.mpf(float(v)) for v in f0])
    for _ in range(12):
        P = [pieces_mp(s[i] * f[i]) for i in range(n)]
        g = mpmath.matrix([s[i] * P[i][1] for i in range(n)])
        F = f - mean - Kmp * g
        J = mpmath.eye(n) + Kmp * mpmath.diag([P[i][2] for i in range(n)])
        step = mpmath.lu_solve(J, F)
        f = f - step
        if max(abs(v) for v in step) <= mpmath.mpf(10) ** (-DPS + 8) * max(1, max(abs(v) for v in f)):
            break
    P = [pieces_mp(s[i] * f[i]) for i in range(n)]
    a = [s[i] * P[i][1] for i in range(n)]
    W = [P[i][2] for i in range(n)]
    sw = [mpmath.sqrt(w) for w in W]
    B = mpmath.eye(n) + mpmath.diag(sw) * Kmp * mpmath.diag(sw)
    psi = -mpmath.fsum(a[i] * (f[i] - mean) for i in range(n)) / 2 + mpmath.fsum(p[0] for p in P)
    nll = -(psi - mpmath.log(mpmath.det(B)) / 2)
    return {"f": list(f), "a": a, "W": W, "sw": sw, "B": B, "nll": nll}


def mp_posterior(Ksmp, amp, mean, sol):
    """mu = mean + k*' a and var = amp - (W^1/2 k*)' B^-1 (W^1/2 k*) at the rows of Ksmp, DPS digits."""
    n = len(sol["a"])
    mus, vs = [], []
    for r in range(Ksmp.rows):
        k = [Ksmp[r, j] for j in range(n)]
        mus.append(mpmath.mpf(float(mean)) + mpmath.fsum(k[j] * sol["a"][j] for j in range(n)))
        u = mpmath.matrix([sol["sw"][j] * k[j] for j in range(n)])
        x = mpmath.lu_solve(sol["B"], u)
        vs.append(mpmath.mpf(float(amp)) - mpmath.fsum(u[j] * x[j] for j in range(n)))
    return mus, vs


# ---- cases --------------------------------------------------------------------------------------------------------------------
def case_inputs(N, d, amp, mean, kern, labels, seed=0):
    """X in [0, 1]^d, lengthscales 0.3 sqrt(d) (squared: 0.09 d), 8 test rows, and the labels: 'mixed' (violated on one side of a
    tilted plane, at least one of each where N >= 2), 'zeros' or 'ones'."""
    rng = np.random.default_rng(1000 * N + 10 * d + seed)
    X = rng.random((N, d))
    Xs = rng.random((8, d))
    ls = np.full(d, 0.09 * d) * (1.0 + 0.25 * rng.random(d))
    if labels == "zeros":
        v = np.zeros(N)
    elif labels == "ones":
        v = np.ones(N)
    else:
        v = (X @ np.linspace(1.0, 2.0, d) > np.median(X @ np.linspace(1.0, 2.0, d))).astype(np.float64)
        if N >= 2 and v.min() == v.max():
            v[0] = 1.0 - v[0]
    return X, v, ls, float(amp), float(mean), Xs


# The issue's factors: N {1, 2, 12, 24}, d {1, 3, 6}, amp {1e-2, 1, 1e2, 1e4}, mean {-1, 0, 0.5}, both kernels, mixed / all-0 / all-1.
# Every (N, amp) pair appears (the pair that sets the conditioning and the tails reached); d, mean, kernel and labels cycle through them
# with periods 3, 3, 2, 3 against 16 pairs, so every value of every factor -- and every (amp, labels) and (amp, kernel) pair -- occurs.
def host_cases():
    out, k = [], 0
    for N in (1, 2, 12, 24):
        for amp in (1e-2, 1.0, 1e2, 1e4):
            out.append((N, (1, 3, 6)[k % 3], amp, (-1.0, 0.0, 0.5)[(k // 2) % 3], (SE, MATERN)[k % 2], ("mixed", "zeros", "ones")[(k + k // 4) % 3]))
            k += 1
    # ... and the one-class labels at the largest amplitude and N, both kernels
    out += [(24, 6, 1e4, 0.5, SE, "ones"), (24, 3, 1e4, -1.0, MATERN, "zeros"), (12, 1, 1e4, 0.0, MATERN, "mixed"), (24, 6, 1e2, 0.0, SE, "mixed")]
    return out


@functools.lru_cache(maxsize=None)
def solved_case(case):
    """One case solved three ways, once per process: the float64 restatement, the 50-digit truth, and the restatement's own errors
    (the yardsticks).  Returns dict(inputs, fit, truth (floats of the 50-digit values), err (f, a, W, mu, var, nll), scale)."""
    N, d, amp, mean, kern, labels = case
    X, v, ls, amp, mean, Xs = case_inputs(N, d, amp, mean, kern, labels)
    K = cov(X, X, ls, amp, kern)
    fit = laplace_fit(K, v, mean)
    mu, var = posterior(cov(Xs, X, ls, amp, kern), amp, mean, fit)
    with mpmath.workdps(DPS):
        sol = mp_mode(cov_mp(X, X, ls, amp, kern), v, mean, fit["f"])
        mus, vs = mp_posterior(cov_mp(Xs, X, ls, amp, kern), amp, mean, sol)
        truth = {"f": sol["f"], "a": sol["a"], "W": sol["W"], "mu": mus, "var": vs, "nll": [sol["nll"]]}
        got = {"f": fit["f"], "a": fit["a"], "W": fit["W"], "mu": mu, "var": var, "nll": [fit["nll"]]}
        err = {q: max(float(abs(mpmath.mpf(float(g)) - t)) for g, t in zip(got[q], truth[q])) for q in truth}
        tf = {q: np.array([float(t) for t in truth[q]]) for q in truth}
        lo = {q: np.array([float(t - mpmath.mpf(float(t))) for t in truth[q]]) for q in truth}
    return {"X": X, "v": v, "ls": ls, "amp": amp, "mean": mean, "Xs": Xs, "kern": kern, "fit": fit, "truth": tf, "truth_lo": lo, "err": err,
            "scale": {q: float(np.max(np.abs(tf[q]))) for q in tf}}


def bar(sol, q):
    """The project's bar for quantity q of a solved case: 8 x the float64 restatement's own error + 16 eps max|q|."""
    return 8.0 * sol["err"][q] + 16.0 * EPS * sol["scale"][q]


def errors_against(sol, q, got):
    """max |got - truth| with the truth held as a (hi, lo) pair."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    return float(np.max(np.abs((got - sol["truth"][q]) - sol["truth_lo"][q])))
