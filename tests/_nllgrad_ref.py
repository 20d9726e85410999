"""The gradient of the GP regressor's negative log marginal likelihood (csrc/nll_grad.hip), stated three times on the host: in numpy
float64 the way the device forms it, in numpy.longdouble with a hand-written Cholesky (the truth for N > 24), and in mpmath at 50
digits with K formed in 50 digits from the float64 inputs (the truth for N <= 24).  Checked on the CPU by tests/test_nllgrad_host.py;
the yardsticks of tests/test_gpu_nllgrad.py come from here.

theta = [log lenscale_sq_1..d, log amp, log noise, mean];  K = Kf + (noise + jitter) I,  alpha = inv(K) (y - mean),
nll = 1/2 (y - mean)' alpha + sum log L_ii + N/2 log 2 pi,  Q = inv(K) - alpha alpha',  w = 1 / lenscale_sq,
    d/d log lenscale_sq_k = 1/4 sum_ij Q_ij g_ij (x_ik - x_jk)^2 w_k      g = -2 dk/dD: ARD-SE g = k, Matern-5/2 g = 5/3 amp (1 + s) exp(-s)
    d/d log amp           = 1/2 sum_ij Q_ij Kf_ij
    d/d log noise         = 1/2 noise tr Q          (a jitter is a constant: it is in K but not differentiated)
    d/d mean              = -sum_i alpha_i
Every form returns (nll, grad[d + 3], scale[d + 3]) with scale_k = 1/2 sum_ij |Q_ij dK_ij/dtheta_k| (mean: sum_i |alpha_i|): the size
of the terms a component is the sum of, which is what its rounding error is proportional to."""
import mpmath
import numpy as np

from _laplace_ref import MATERN, SE, cov_mp

DPS = 50
EPS = 2.0 ** -52


def _kg(D, amp, kern, dtype):
    """(k, g) from the distance D in dtype."""
    amp = dtype(amp)
    if kern == SE:
        k = amp * np.exp(-D / dtype(2))
        return k, k
    s = np.sqrt(dtype(5) * D)
    e = np.exp(-s)
    return amp * (dtype(1) + s + s * s / dtype(3)) * e, dtype(5) / dtype(3) * amp * (dtype(1) + s) * e


def _assemble(Q, alpha, Kf, G, X, w, noise, dtype):
    d = X.shape[1]
    grad, scale = np.zeros(d + 3, dtype=dtype), np.zeros(d + 3, dtype=dtype)
    QG = Q * G
    for k in range(d):
        diff = X[:, None, k] - X[None, :, k]          # on the raw observations, the square not expanded
        T = QG * (diff * diff) * w[k]
        grad[k], scale[k] = dtype(0.25) * T.sum(), dtype(0.25) * np.abs(T).sum()
    T = Q * Kf
    grad[d], scale[d] = dtype(0.5) * T.sum(), dtype(0.5) * np.abs(T).sum()
    dq = np.diag(Q)
    grad[d + 1], scale[d + 1] = dtype(0.5) * dtype(noise) * dq.sum(), dtype(0.5) * dtype(noise) * np.abs(dq).sum()
    grad[d + 2], scale[d + 2] = -alpha.sum(), np.abs(alpha).sum()
    return grad, scale


def nll_grad_f64(X, y, lenscale_sq, amp, noise, mean, kern, jitter=0.0):
    """numpy float64, the way the device forms it: the distance in the expanded form of utils/math.lua:65-111 (X^2 w + (Z^2 w)' -
    2 X (Z .* w)', clamped at 0), inv(K) = Linv' Linv from the explicit inverse of the Cholesky factor."""
    from scipy.linalg import cholesky, solve_triangular
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).ravel()
    N = X.shape[0]
    w = 1.0 / np.asarray(lenscale_sq, dtype=np.float64)
    xs = (X * X) @ w
    D = np.maximum((xs[:, None] + xs[None, :]) - 2.0 * (X @ (X * w).T), 0.0)
    Kf, G = _kg(D, amp, kern, np.float64)
    K = Kf + (noise + jitter) * np.eye(N)
    L = cholesky(K, lower=True)
    Linv = solve_triangular(L, np.eye(N), lower=True)
    r = y - mean
    alpha = Linv.T @ (Linv @ r)
    nll = 0.5 * float(r @ alpha) + float(np.log(np.diag(L)).sum()) + 0.5 * N * np.log(2.0 * np.pi)
    Q = Linv.T @ Linv - np.outer(alpha, alpha)
    grad, scale = _assemble(Q, alpha, Kf, G, X, w, noise, np.float64)
    return nll, grad, scale


def plain_factorisation_succeeds(X, lenscale_sq, amp, noise, kern):
    """Does the float64 restatement factor K without a jitter (where a case asks for noise == 0)?"""
    try:
        nll, g, _ = nll_grad_f64(X, np.zeros(len(X)), lenscale_sq, amp, noise, 0.0, kern)
        return bool(np.isfinite(nll) and np.isfinite(g).all())
    except Exception:
        return False


def chol_ld(A):
    """Hand-written lower Cholesky in numpy.longdouble (column by column; no LAPACK below float64)."""
    n = A.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % j)
        L[j, j] = np.sqrt(v[0])
        L[j + 1:, j] = v[1:] / L[j, j]
    return L


def tri_inv_ld(L):
    n = L.shape[0]
    Li = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        e = np.zeros(n, dtype=np.longdouble)
        e[i] = 1
        Li[i] = (e - L[i, :i] @ Li[:i]) / L[i, i]
    return Li


def nll_grad_ld(X, y, lenscale_sq, amp, noise, mean, kern, jitter=0.0):
    """numpy.longdouble, K in the difference form."""
    ld = np.longdouble
    X = np.asarray(X, dtype=ld)
    y = np.asarray(y, dtype=ld).ravel()
    N = X.shape[0]
    w = ld(1) / np.asarray(lenscale_sq, dtype=ld)
    diff = X[:, None, :] - X[None, :, :]
    D = np.sum(diff * diff * w, axis=2)
    Kf, G = _kg(D, amp, kern, ld)
    K = Kf + (ld(noise) + ld(jitter)) * np.eye(N, dtype=ld)
    L = chol_ld(K)
    Linv = tri_inv_ld(L)
    r = y - ld(mean)
    alpha = Linv.T @ (Linv @ r)
    nll = ld(0.5) * (r @ alpha) + np.log(np.diag(L)).sum() + ld(0.5) * N * np.log(ld(2) * np.pi)
    Q = Linv.T @ Linv - np.outer(alpha, alpha)
    grad, scale = _assemble(Q, alpha, Kf, G, X, w, noise, ld)
    return nll, grad, scale


def _mp_parts(X, y, lenscale_sq, amp, noise, mean, kern, jitter):
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    Kf = cov_mp(X, X, lenscale_sq, amp, kern)
    K = Kf.copy()
    for i in range(N):
        K[i, i] += mpmath.mpf(float(noise)) + mpmath.mpf(float(jitter))
    L = mpmath.cholesky(K)
    r = mpmath.matrix([mpmath.mpf(float(v)) - mpmath.mpf(float(mean)) for v in np.asarray(y, dtype=np.float64).ravel()])
    alpha = mpmath.cholesky_solve(K, r)
    nll = (r.T * alpha)[0] / 2 + mpmath.fsum(mpmath.log(L[i, i]) for i in range(N)) + mpmath.mpf(N) / 2 * mpmath.log(2 * mpmath.pi)
    return Kf, K, L, r, alpha, nll


def nll_mp(X, y, lenscale_sq, amp, noise, mean, kern, jitter=0.0):
    with mpmath.workdps(DPS):
        return _mp_parts(X, y, lenscale_sq, amp, noise, mean, kern, jitter)[5]


def nll_grad_mp(X, y, lenscale_sq, amp, noise, mean, kern, jitter=0.0):
    """mpmath at 50 digits; K formed in 50 digits from the float64 inputs (_laplace_ref.cov_mp).  Returns mpf values."""
    with mpmath.workdps(DPS):
        X = np.asarray(X, dtype=np.float64)
        N, d = X.shape
        Kf, K, L, r, alpha, nll = _mp_parts(X, y, lenscale_sq, amp, noise, mean, kern, jitter)
        Kinv = mpmath.inverse(K)
        w = [1 / mpmath.mpf(float(v)) for v in lenscale_sq]
        A = mpmath.mpf(float(amp))
        grad, scale = [mpmath.mpf(0)] * (d + 3), [mpmath.mpf(0)] * (d + 3)
        tl = [[] for _ in range(d)]
        ta = []
        for i in range(N):
            for j in range(N):
                q = Kinv[i, j] - alpha[i] * alpha[j]
                ta.append(q * Kf[i, j])
                if kern == SE:
                    g = Kf[i, j]
                else:
                    D = mpmath.fsum((mpmath.mpf(float(X[i, k])) - mpmath.mpf(float(X[j, k]))) ** 2 * w[k] for k in range(d))
                    s = mpmath.sqrt(5 * D)
                    g = mpmath.mpf(5) / 3 * A * (1 + s) * mpmath.exp(-s)
                for k in range(d):
                    df = mpmath.mpf(float(X[i, k])) - mpmath.mpf(float(X[j, k]))
                    tl[k].append(q * g * df * df * w[k])
        for k in range(d):
            grad[k], scale[k] = mpmath.fsum(tl[k]) / 4, mpmath.fsum(abs(t) for t in tl[k]) / 4
        grad[d], scale[d] = mpmath.fsum(ta) / 2, mpmath.fsum(abs(t) for t in ta) / 2
        dq = [Kinv[i, i] - alpha[i] * alpha[i] for i in range(N)]
        nz = mpmath.mpf(float(noise))
        grad[d + 1], scale[d + 1] = nz * mpmath.fsum(dq) / 2, nz * mpmath.fsum(abs(t) for t in dq) / 2
        grad[d + 2], scale[d + 2] = -mpmath.fsum(alpha), mpmath.fsum(abs(a) for a in alpha)
        return nll, grad, scale


def central_difference_mp(X, y, lenscale_sq, amp, noise, mean, kern, h=None):
    """The 50-digit central difference of the 50-digit nll in theta's coordinates (step 1e-15: truncation ~1e-30)."""
    with mpmath.workdps(DPS):
        h = mpmath.mpf(10) ** -15 if h is None else h
        d = len(lenscale_sq)
        theta = [mpmath.log(mpmath.mpf(float(v))) for v in lenscale_sq] + [mpmath.log(mpmath.mpf(float(amp))),
                                                                          mpmath.log(mpmath.mpf(float(noise))) if noise > 0 else None,
                                                                          mpmath.mpf(float(mean))]

        def f(t):
            X64 = np.asarray(X, dtype=np.float64)
            N = X64.shape[0]
            ls = [mpmath.exp(v) for v in t[:d]]
            A, nz, m = mpmath.exp(t[d]), (mpmath.exp(t[d + 1]) if t[d + 1] is not None else mpmath.mpf(0)), t[d + 2]
            K = mpmath.matrix(N, N)
            for i in range(N):
                for j in range(N):
                    D = mpmath.fsum((mpmath.mpf(float(X64[i, k])) - mpmath.mpf(float(X64[j, k]))) ** 2 / ls[k] for k in range(d))
                    if kern == SE:
                        K[i, j] = A * mpmath.exp(-D / 2)
                    else:
                        s = mpmath.sqrt(5 * D)
                        K[i, j] = A * (1 + s + s * s / 3) * mpmath.exp(-s)
                K[i, i] += nz
            L = mpmath.cholesky(K)
            r = mpmath.matrix([mpmath.mpf(float(v)) - m for v in np.asarray(y, dtype=np.float64).ravel()])
            a = mpmath.cholesky_solve(K, r)
            return (r.T * a)[0] / 2 + mpmath.fsum(mpmath.log(L[i, i]) for i in range(N)) + mpmath.mpf(N) / 2 * mpmath.log(2 * mpmath.pi)

        out = []
        for k in range(d + 3):
            if theta[k] is None:
                out.append(mpmath.mpf(0))
                continue
            tp, tm = list(theta), list(theta)
            tp[k], tm[k] = theta[k] + h, theta[k] - h
            out.append((f(tp) - f(tm)) / (2 * h))
        return out


def ld_to_mp(x):
    """A numpy.longdouble as an mpf, exactly (two float64 pieces: 64 significant bits fit in 53 + 53)."""
    x = np.longdouble(x)
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - np.longdouble(hi)))


def problem(N, d, seed, amp=1.0, noise_rel=1e-2, mean=0.5, ls_scale=1.0):
    """Observations in the unit cube, responses a draw-like smooth function scaled to the amplitude; hypers around them."""
    rng = np.random.default_rng([seed, N, d])
    X = rng.random((N, d))
    y = mean + np.sqrt(amp) * (np.sin(3.0 * X.sum(axis=1) / np.sqrt(d)) + 0.3 * rng.standard_normal(N))
    ls = ls_scale * (d / 8.0) * (0.6 + 0.8 * rng.random(d))
    return X, y, {"lenscale_sq": ls, "amp": float(amp), "noise": float(noise_rel * amp), "mean": float(mean)}


def bar(err64, scale):
    """The project's bar per component: 8 x the float64 restatement's own error + 16 eps x scale."""
    return 8.0 * np.asarray(err64, dtype=np.float64) + 16.0 * EPS * np.asarray(scale, dtype=np.float64)
