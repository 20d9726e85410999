"""Host-side references for tests/test_gpu_numerics.py: exact or 50-digit arithmetic (mpmath), the input constructors whose
float64 evaluation is exact, the error bars, and the exact invariances of the GP algebra.  No GPU needed here; the host tests
of these helpers are tests/test_exact_helpers.py."""
import math
from fractions import Fraction

import mpmath
import numpy as np
from scipy.linalg import lapack, solve_triangular

EPS = 2.0 ** -52
TINY = 2.0 ** -1022          # smallest normal double
SUB_BAR = 2.0 ** -1073       # absolute bar below TINY: two subnormal ulps


# ---- ulp measures -------------------------------------------------------------------------------------------------------
def mp_to_pair(v):
    """An mpf as (hi, lo) doubles with hi = round(v), lo = round(v - hi): about 106 correct bits where v is normal."""
    hi = float(v)
    lo = float(v - hi) if math.isfinite(hi) else 0.0
    return hi, lo


def pairs(values):
    hl = np.array([mp_to_pair(v) for v in values], dtype=np.float64).reshape(-1, 2)
    return hl[:, 0], hl[:, 1]


def ulp_of(hi):
    """The ulp of a double-rounded true value whose leading part is hi (normal range: 2^(e - 52) for 2^e <= |hi| < 2^(e+1))."""
    _, e = np.frexp(np.abs(hi))
    return np.ldexp(1.0, e - 53)


def ulp_errors(got, hi, lo):
    """|got - truth| in ulps of the truth where the truth is normal, NaN where it is not (those are judged by abs_errors)."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((got - hi) - lo) / ulp_of(hi)
    return np.where(np.abs(hi) >= TINY, err, np.nan)


def abs_errors(got, hi, lo):
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs((got - hi) - lo)


def within_bar(got, hi, lo, ulps, sub_bar=SUB_BAR):
    """(ok, worst ulp error over the normal truths, worst absolute error over the others)."""
    normal = np.abs(hi) >= TINY
    u = ulp_errors(got, hi, lo)
    a = abs_errors(got, hi, lo)
    wu = float(np.nanmax(u)) if normal.any() else 0.0
    wa = float(np.max(a[~normal])) if (~normal).any() else 0.0
    ok = bool(np.all(u[normal] <= ulps) and np.all(a[~normal] <= sub_bar))
    return ok, wu, wa


# ---- section A: points whose squared scaled distance to the origin is exact ------------------------------------------------
def _squares(S, d):
    """Non-negative integers k (length d) with sum k^2 == S, by greedy descent with a little backtracking; None if not found.
    d = 1 returns the nearest square instead (the caller reads the exact argument back from the coordinates)."""
    if d == 1:
        k = math.isqrt(S)
        if (k + 1) ** 2 - S < S - k * k:
            k += 1
        return [k]

    def rec(s, left):
        if s == 0:
            return [0] * left
        if left == 1:
            r = math.isqrt(s)
            return [r] if r * r == s else None
        top = math.isqrt(s)
        for k in range(top, max(-1, top - 8), -1):
            sub = rec(s - k * k, left - 1)
            if sub is not None:
                return [k] + sub
        return None

    return rec(S, d)


def exp_points(targets, d, j=0):
    """Rows X (len(targets) x d) with coordinates k * 2^-10 and the exact kernel argument of each against an observation at the
    origin under lenscale_sq = 4^j in every coordinate: arg = -sum(x^2) / 4^j / 2 (a Fraction), which float64 evaluates without
    rounding in any order.  A target that d coordinates cannot reach exactly gets the nearest reachable argument."""
    X = np.zeros((len(targets), d), dtype=np.float64)
    args = []
    for i, t in enumerate(targets):
        S = int(round(-2.0 * float(t) * 2.0 ** (20 + 2 * j)))
        ks = _squares(S, d)
        if ks is None:       # a sum of d >= 4 squares always exists; the greedy search may still miss it: step to a neighbour
            for s2 in range(S - 1, S - 64, -1):
                ks = _squares(s2, d)
                if ks is not None:
                    break
        X[i, :len(ks)] = np.ldexp(np.array(ks, dtype=np.float64), -10)
        args.append(exact_arg(X[i], j))
    return X, args


def exact_arg(x, j=0):
    """-sum(x^2) / 4^j / 2 as a Fraction, from the float64 coordinates themselves."""
    s = sum(Fraction(float(v)) ** 2 for v in x)
    return -s / Fraction(4) ** j / 2


def exp_arg_float64(x, j=0):
    """What the kernels compute for the argument: (x^2 / lenscale_sq) summed, halved, negated -- in float64."""
    w = 1.0 / 4.0 ** j
    s = 0.0
    for v in x:
        s += (v * v) * w
    return -0.5 * s


def exp_targets(dense=4096, seed=0):
    """The arguments section A covers: a dense sweep of [-1000, 0]; every table residue n & 127 at several exponents n >> 7
    (negative ones included); the subnormal range [-745, -708]; the clamp at -1000 and beyond it; the neighbourhood of 0."""
    rng = np.random.default_rng(seed)
    ln2_128 = math.log(2.0) / 128.0
    t = list(np.linspace(-1000.0, 0.0, dense))
    for hi in (0, -1, -3, -40, -200, -1000, -1400):          # n >> 7 = hi: n = 128 hi + j
        for jres in range(128):
            t.append(max(-1000.0, (128 * hi + jres) * ln2_128 + rng.uniform(-0.3, 0.3) * ln2_128))
    t += list(np.linspace(-745.0, -708.0, 512))
    t += list(rng.uniform(-1000.0, 0.0, 1024))
    t += [-1000.0, -1000.0 - 2.0 ** -20, -1001.0, -1100.0, -2.0 ** -20, -1e-3, -0.5]
    return [min(0.0, v) for v in t]


def special_exp_rows(d):
    """Rows whose arguments are -0.0 (the origin itself), -2^-1001 (about -1e-301: one coordinate 2^-500), exactly -1000 (when d
    >= 2 squares can reach 2000) and -1e4, with their exact arguments (lenscale_sq = 1)."""
    rows = [np.zeros(d)]
    x = np.zeros(d)
    x[0] = 2.0 ** -500
    rows.append(x)
    if d >= 2:
        x = np.zeros(d)
        x[0], x[1] = 40.0, 20.0         # 1600 + 400 = 2000
        rows.append(x)
    x = np.zeros(d)
    x[0] = math.sqrt(2e4)
    rows.append(x)
    X = np.array(rows)
    return X, [exact_arg(r, 0) for r in X]


def amp_exp_truth(amp, args, dps=40):
    """amp * exp(arg) for exact arguments (Fractions) as (hi, lo) pairs."""
    with mpmath.workdps(dps):
        e = [mpmath.exp(mpmath.mpf(a.numerator) / a.denominator) for a in args]
        return pairs([mpmath.mpf(amp) * v for v in e])


# ---- section B: activations ----------------------------------------------------------------------------------------------
def activation_inputs(seed=0):
    """Finite inputs of section B: +-0, +-subnormals, +-1e-8 ... 1e-300, a dense sweep of [-30, 30] and the neighbourhood of
    |x| = 22.5 (where tanh_fast4 clamps 2|x| at 45)."""
    rng = np.random.default_rng(seed)
    v = [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1060, -(2.0 ** -1060), 2.0 ** -1023, -(2.0 ** -1023), 2.0 ** -1022]
    tiny = 10.0 ** -np.arange(8, 301, dtype=np.float64)
    v += list(tiny) + list(-tiny)
    v += list(np.linspace(-30.0, 30.0, 12001))
    near = 22.5 + np.concatenate([np.linspace(-1e-3, 1e-3, 201), np.array([-2.0 ** -40, 2.0 ** -40, -2.0 ** -48])])
    v += list(near) + list(-near) + [np.nextafter(22.5, 0), np.nextafter(22.5, 30), 22.5, -22.5]
    v += list(rng.uniform(-30.0, 30.0, 2048)) + list(np.exp(rng.uniform(-20, 3.4, 1024)) * rng.choice([-1, 1], 1024))
    return np.array(v, dtype=np.float64)


def activation_truth(kind, x, dps=40):
    """(hi, lo) of tanh / sigmoid / relu at the doubles x, in mpmath."""
    with mpmath.workdps(dps):
        out = []
        for v in x:
            m = mpmath.mpf(float(v))
            if kind == "Tanh":
                out.append(mpmath.tanh(m))
            elif kind == "Sigmoid":
                out.append(1 / (1 + mpmath.exp(-m)))
            else:
                out.append(m if m > 0 else mpmath.mpf(0))
        return pairs(out)


def numpy_activation(kind, v):
    """The oracle's activations (oracle/blr.py), which fix the NaN / inf / signed-zero behaviour."""
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == "Tanh":
            return np.tanh(v)
        if kind == "Sigmoid":
            return 1.0 / (1.0 + np.exp(-v))
        return np.maximum(v, 0.0)


# ---- section C: GP regression in 50-digit arithmetic ----------------------------------------------------------------------
class Truth(object):
    __slots__ = ("nll", "mu", "var", "jitter")


def gp_truth(X, Y, lenscale_sq, amp, noise, mean, Xs, jitter=0.0, dps=50):
    """Textbook GP regression of the float64 inputs, evaluated at dps digits: NLL, posterior mean and latent variance at Xs
    (the same algebra as oracle/gp.py, with no rounding that matters).  K + (noise + jitter) I."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64).reshape(-1)
    N, d = X.shape
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        ls = [mpf(float(v)) for v in np.asarray(lenscale_sq, dtype=np.float64).ravel()]
        A, m = mpf(float(amp)), mpf(float(mean))
        Xm = [[mpf(float(v)) for v in r] for r in X]

        def k(a, b):
            return A * mpmath.exp(-sum((a[i] - b[i]) ** 2 / ls[i] for i in range(d)) / 2)

        K = mpmath.matrix(N, N)
        for i in range(N):
            for jj in range(i + 1):
                K[i, jj] = K[jj, i] = k(Xm[i], Xm[jj])
            K[i, i] += mpf(float(noise)) + mpf(float(jitter))
        L = mpmath.cholesky(K)
        r = mpmath.matrix([mpf(float(v)) - m for v in y])
        t = _fwd(L, r)
        alpha = _bwd(L, t)
        logdet = 2 * mpmath.fsum(mpmath.log(L[i, i]) for i in range(N))
        out = Truth()
        out.jitter = jitter
        out.nll = mpmath.fsum(r[i] * alpha[i] for i in range(N)) / 2 + logdet / 2 + N * mpmath.log(2 * mpmath.pi) / 2
        mu, var = [], []
        for row in Xs:
            zm = [mpf(float(v)) for v in row]
            ks = mpmath.matrix([k(zm, Xm[i]) for i in range(N)])
            v = _fwd(L, ks)
            mu.append(m + mpmath.fsum(ks[i] * alpha[i] for i in range(N)))
            var.append(A - mpmath.fsum(v[i] ** 2 for i in range(N)))
        out.mu, out.var = mu, var
        return out


def _fwd(L, b):
    n = L.rows
    x = mpmath.matrix(n, 1)
    for i in range(n):
        x[i] = (b[i] - mpmath.fsum(L[i, j] * x[j] for j in range(i))) / L[i, i]
    return x


def _bwd(L, b):
    n = L.rows
    x = mpmath.matrix(n, 1)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - mpmath.fsum(L[j, i] * x[j] for j in range(i + 1, n))) / L[i, i]
    return x


def lapack_fit(X, Y, lenscale_sq, amp, noise, mean, Xs, jitter=0.0, kscale=1.0):
    """oracle/gp.py's algebra on K + jitter I with a GIVEN jitter (the device's): (nll, mu, var), None if dpotrf fails.
    kscale != 1 multiplies the off-diagonal covariances by it: the same algebra on a K assembled a few ulp differently."""
    from oracle import gp
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(Y, dtype=np.float64).reshape(-1, 1)
    K = gp.ardse(X, None, lenscale_sq, amp)
    if kscale != 1.0:
        K *= kscale
        K[np.diag_indices(K.shape[0])] /= kscale
    K[np.diag_indices(K.shape[0])] += noise
    if jitter:
        K[np.diag_indices(K.shape[0])] += jitter
    L, info = lapack.dpotrf(K, lower=1, clean=1)
    if info != 0:
        return None
    r = y - mean
    alpha = solve_triangular(L, solve_triangular(L, r, lower=True), lower=True, trans="T")
    nll = float(0.5 * np.sum(r * alpha) + np.sum(np.log(np.diag(L))) + 0.5 * X.shape[0] * np.log(2.0 * np.pi))
    Ks = gp.ardse(Xs, X, lenscale_sq, amp)
    mu = mean + (Ks @ alpha)[:, 0]
    V = solve_triangular(L, Ks.T, lower=True)
    var = amp - np.einsum("ij,ij->j", V, V)
    return nll, mu, var


def grid_data(N, d, seed):
    """Observations on the grid k 2^-10 in [0, 1): under a lenscale_sq that is a power of 4 every squared scaled distance is
    exact in float64, on the host (oracle/gp.py's GEMM form) and on the device, so the host's K and the device's differ only
    by the exponential: <= 2 ulp on the device (section A), < 1 ulp in glibc."""
    rng = np.random.default_rng(seed)
    X = np.ldexp(rng.integers(0, 1024, (N, d)).astype(np.float64), -10)
    y = np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0]) + 0.05 * rng.normal(size=N)
    return X, ((y - y.mean()) / y.std()).reshape(-1, 1)


def jitter_schedule(max_eps, eps=1e-8, growth=1.1):
    """Every jitter utils/math.lua:159-218 can try on a K of Frobenius norm max_eps (the oracle's loop, value for value)."""
    out = []
    while not eps > max_eps:
        eps = eps * growth
        out.append(eps)
    return out


def min_pivot(K):
    """The smallest pivot of a right-looking Cholesky of K in float64 (the first non-positive one ends it)."""
    A = np.array(K, dtype=np.float64)
    n = A.shape[0]
    best = np.inf
    for j in range(n):
        p = A[j, j]
        best = min(best, p)
        if not p > 0.0:
            break
        c = A[j + 1:, j] / math.sqrt(p)
        A[j + 1:, j + 1:] -= np.outer(c, c)
    return best


def err_vs(got, truth):
    """max |got - truth| over a vector (truth: mpf values), in float64."""
    hi, lo = pairs(truth)
    return float(np.max(abs_errors(np.asarray(got, dtype=np.float64).ravel(), hi, lo)))


def gp_bar(err_oracle, scale, factor=8.0):
    """Section C's bar: as accurate as LAPACK doing the same algebra, up to a factor, plus 16 eps of the quantity's scale."""
    return factor * err_oracle + 16.0 * EPS * scale


def backward_errors(K, L, Linv, jitter=0.0):
    """||L L^T - (K + jitter I)||_F / ||K||_F and ||Linv L - I||_F, in long double."""
    Kl = np.asarray(K, dtype=np.longdouble).copy()
    Kl[np.diag_indices(Kl.shape[0])] += np.longdouble(jitter)
    Ll = np.tril(np.asarray(L, dtype=np.longdouble))
    r1 = float(np.linalg.norm((Ll @ Ll.T - Kl).astype(np.float64)) / np.linalg.norm(np.asarray(K, dtype=np.float64)))
    Il = np.tril(np.asarray(Linv, dtype=np.longdouble)) @ Ll
    Il[np.diag_indices(Il.shape[0])] -= 1
    return r1, float(np.linalg.norm(Il.astype(np.float64)))


# ---- section D: exact invariances -------------------------------------------------------------------------------------------
def scale_y(hyp, Y, k):
    """Y and mean by 2^k, amp and noise by 4^k."""
    h = dict(hyp, amp=math.ldexp(hyp["amp"], 2 * k), noise=math.ldexp(hyp["noise"], 2 * k), mean=math.ldexp(hyp["mean"], k))
    return h, np.ldexp(np.asarray(Y, dtype=np.float64), k)


def scale_x(hyp, X, j):
    """X (and the candidates) by 2^j, lenscale_sq by 4^j."""
    h = dict(hyp, lenscale_sq=np.ldexp(np.asarray(hyp["lenscale_sq"], dtype=np.float64), 2 * j))
    return h, np.ldexp(np.asarray(X, dtype=np.float64), j)
