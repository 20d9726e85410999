"""References for Thompson sampling on the Bayesian-linear head (tests/test_blr_ts_host.py, tests/test_gpu_blr_ts.py).  No GPU needed
here.  A path of b7_blr_ts_nominate is f_j(x) = mean_s + phi(x)' w_j with w_j = m_s + L_s^-T eps_j, s = j mod S; this module restates

  * eps_j: the library's counter normal (tests/_ts_ref.py: counter_normal / counter_key) on the stream 2^32 + j, counter k;
  * the weights GIVEN the device's own L^-1, m and eps, in double-double (tests/_blr_ref.py: error-free products, exact sums), with
    the project's bar for such a triangular product: 8 x numpy float64's own error on the same operands + 16 eps sum |L^-1| |eps|;
  * the paths GIVEN the device's own weights, as _blr_ref.exact_mean_rows / mean_bar judge the head's mean;
  * the nominees by _ts_ref.nominees_ref;
  * the covariance of the two candidate maps eps -> L^-T eps and eps -> L^-1 eps at 50 digits (the transpose's guard)."""
import mpmath
import numpy as np

import _blr_ref as B
import _exact as E
import _ts_ref as T

STREAM = 1 << 32          # blr_ts.hip: BLR_TS_STREAM; _ts_ref's streams are 0 (the basis) and 1 + j (path j)
DRAW_ULPS = 4.0           # what tests/test_gpu_ts.py holds b7_ts_last_draws' weight and eps to against the numpy restatement
nominees_ref = T.nominees_ref


def eps_ref(seed, path, z):
    """eps_j[k], k < z: a function of (seed, j, k) alone."""
    return T.counter_normal(T.counter_key(seed, STREAM + path), np.arange(z, dtype=np.uint64))


def weights_host(Linv, m, eps):
    """m + L^-T eps in float64 (numpy): the yardstick of the bar."""
    return np.asarray(m, dtype=np.float64).ravel() + np.tril(Linv).T @ np.asarray(eps, dtype=np.float64)


class WeightRef(object):
    __slots__ = ("hi", "lo", "bar", "e_np")


def weights_exact(Linv, m, eps):
    """w_k = m_k + sum_{i >= k} Linv[i][k] eps[i] from the float64 values themselves, as (hi, lo); bar_k = 8 e_np + 16 eps_mach
    sum_i |Linv[i][k]| |eps_i|, e_np numpy's own worst error over the components."""
    Linv = np.tril(np.asarray(Linv, dtype=np.float64))
    m, eps = np.asarray(m, dtype=np.float64).ravel(), np.asarray(eps, dtype=np.float64).ravel()
    z = len(m)
    P, Er = B._two_prod(Linv, eps[:, None])                 # P[i][k] + Er[i][k] = Linv[i][k] eps[i]
    out = [B._dd_sum(list(P[k:, k]) + list(Er[k:, k]) + [float(m[k])]) for k in range(z)]
    r = WeightRef()
    r.hi, r.lo = np.array([o[0] for o in out]), np.array([o[1] for o in out])
    r.e_np = float(np.max(E.abs_errors(weights_host(Linv, m, eps), r.hi, r.lo)))
    r.bar = 8.0 * r.e_np + 16.0 * E.EPS * np.abs(P).sum(0)
    return r


def judge_weights(ref, w):
    """error / bar per component."""
    return E.abs_errors(np.asarray(w, dtype=np.float64).ravel(), ref.hi, ref.lo) / ref.bar


def judge_paths(W, means, Phi, P):
    """error / _blr_ref.mean_bar of the paths P (rows x q) against mean_j + Phi w_j evaluated exactly from the given weights W (z x q)."""
    W, Phi, P = np.asarray(W, dtype=np.float64), np.asarray(Phi, dtype=np.float64), np.asarray(P, dtype=np.float64)
    z = W.shape[0]
    out = np.empty(P.shape)
    for j in range(W.shape[1]):
        hi, lo, ab = B.exact_mean_rows(W[:, j], Phi, means[j])
        out[:, j] = E.abs_errors(P[:, j], hi, lo) / B.mean_bar(z, means[j], ab)
    return out


def map_covariances(A, dps=50):
    """(inv(A), L^-T L^-1, L^-1 L^-T) as mpmath matrices at dps digits, A = L L' (A: float64 entries taken as exact)."""
    with mpmath.workdps(dps):
        z = A.shape[0]
        Am = mpmath.matrix([[mpmath.mpf(float(A[i, j])) for j in range(z)] for i in range(z)])
        L = mpmath.cholesky(Am)
        Li = mpmath.matrix([list(E._fwd(L, mpmath.matrix([1 if i == k else 0 for i in range(z)]))) for k in range(z)]).T
        with mpmath.workdps(2 * dps):
            Ainv = mpmath.inverse(Am)
        return Ainv, Li.T * Li, Li * Li.T


def rel_distance(X, Y, dps=50):
    """max |X - Y| / max |Y| over the entries, as a float."""
    with mpmath.workdps(dps + 10):
        n = X.rows
        return float(max(abs(X[i, j] - Y[i, j]) for i in range(n) for j in range(n)) / max(abs(Y[i, j]) for i in range(n) for j in range(n)))
