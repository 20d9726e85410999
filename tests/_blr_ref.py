"""Host-side references for tests/test_gpu_blr.py: the Bayesian-linear head of models/dngo.lua in 50-digit arithmetic (mpmath),
oracle/blr.py's algebra in float64 as the yardstick of the bars, the exact evaluation of what the mean and variance kernels are
GIVEN (the downloaded L^-1 and weights), and input constructors whose features, Gram matrix and right-hand side are exact in
float64.  No GPU needed here; the host tests of these helpers are tests/test_blr_host.py."""
import math

import mpmath
import numpy as np
from scipy.linalg import lapack, solve_triangular

import _exact as E

U = 2.0 ** -53               # unit roundoff of float64
X_BITS, W_BITS, B_BITS, Y_BITS = 10, 3, 4, 8
Z_BITS = X_BITS + W_BITS     # every dyadic feature is an integer multiple of 2^-13


# ---- inputs whose features are exact in float64 ----------------------------------------------------------------------------
def dyadic_relu_net(d, z, seed):
    """One nn.Linear(d, z) + ReLU with weights k 2^-3 and biases k 2^-4, k an integer in [-8, 8]: (weights, biases) as the
    basis entry points take them."""
    rng = np.random.default_rng(seed)
    W = np.ldexp(rng.integers(-8, 9, (z, d)).astype(np.float64), -W_BITS)
    b = np.ldexp(rng.integers(-8, 9, z).astype(np.float64), -B_BITS)
    return [W], [b]


def dyadic_points(N, d, seed):
    """N points with coordinates k 2^-10, k an integer in [0, 1024)."""
    rng = np.random.default_rng(seed)
    return np.ldexp(rng.integers(0, 1 << X_BITS, (N, d)).astype(np.float64), -X_BITS)


def dyadic_responses(X, seed):
    """A smooth function of X plus noise, rounded to multiples of 2^-8 (so that Z'(y - mean) is exact for a dyadic mean)."""
    rng = np.random.default_rng(seed)
    y = np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0]) + 0.05 * rng.normal(size=X.shape[0])
    return np.ldexp(np.rint(np.ldexp(y, Y_BITS)), -Y_BITS).reshape(-1, 1)


def _ints(a, bits):
    """a 2^bits as int64; a must be an integer multiple of 2^-bits."""
    s = np.ldexp(np.asarray(a, dtype=np.float64), bits)
    i = s.astype(np.int64)
    assert np.array_equal(i.astype(np.float64), s), "not a multiple of 2^-%d" % bits
    return i


def dyadic_features_int(X, W, b):
    """relu(X W' + b) 2^13 in integer arithmetic: every product is a multiple of 2^-13 below 2^3, every sum of d of them and a
    bias is exact in float64 in any order, fused or not -- so every basis kernel must return exactly this."""
    pre = _ints(X, X_BITS) @ _ints(W[0], W_BITS).T + (_ints(b[0], B_BITS) << (Z_BITS - B_BITS))
    return np.maximum(pre, 0)


def dyadic_features(X, W, b):
    return np.ldexp(dyadic_features_int(X, W, b).astype(np.float64), -Z_BITS)


def int_gram(Z):
    """Z'Z 2^26 of dyadic features as an int64 matrix (exact: entries below N 2^32)."""
    Zi = _ints(Z, Z_BITS)
    return Zi.T @ Zi


def _pow2(v):
    return v > 0 and math.frexp(v)[0] == 0.5


def exact_head(Z, y, alpha, beta, mean):
    """A = beta Z'Z + alpha I and q = Z' beta (y - mean) of dyadic features and responses under alpha, beta powers of two and a
    dyadic mean: integers on a common power-of-two scale, below 2^53, so the float64 arrays returned hold them EXACTLY."""
    assert _pow2(alpha) and _pow2(beta)
    G = int_gram(Z)
    ea = int(math.log2(alpha)) - int(math.log2(beta)) + 2 * Z_BITS            # alpha / beta in units of 2^-26
    assert ea >= 0
    Ai = G + (np.int64(1) << ea) * np.eye(G.shape[0], dtype=np.int64)
    qi = _ints(Z, Z_BITS).T @ _ints(np.asarray(y, dtype=np.float64).ravel() - mean, Y_BITS)
    assert int(np.abs(Ai).max()) < 2 ** 53 and int(np.abs(qi).max()) < 2 ** 53
    return (np.ldexp(Ai.astype(np.float64), int(math.log2(beta)) - 2 * Z_BITS),
            np.ldexp(qi.astype(np.float64), int(math.log2(beta)) - Z_BITS - Y_BITS))


def pivot_case(d=3, z=8, N=64, seed=5):
    """Test g's head: a dyadic net whose first two features are the constant 1/2 (zero weights, bias 1/2), N = 64 observations, so
    g = sum z_i^2 = 16 = 4^2; with beta = 1 and alpha = 2^-200, A_11 = A_21 = A_22 round to 16, sqrt(16) is exact and the second
    pivot is 16 - 4 * 4 = 0 in any float64 Cholesky."""
    W, b = dyadic_relu_net(d, z, seed)
    W[0][:2] = 0.0
    b[0][:2] = 0.5
    X = dyadic_points(N, d, seed + 1)
    return W, b, X, dyadic_responses(X, seed + 2), 2.0 ** -200, 1.0


# The shapes of tests/test_gpu_blr.py (and of the host tests of the bars).  Small heads (z <= 64, a live 50-digit truth): the edges
# of the 64-observation chunk and of the 16-wide tiles of G; (10, 64) has N < z and rests on alpha alone.  Wide heads: backward
# errors only, under hypers that make A and q exact in float64 (exact_head).
D = 3
SMALL_CASES = [(1, 1), (63, 16), (64, 17), (65, 48), (65, 49), (129, 63), (129, 64), (10, 64), (200, 50)]
WIDE_CASES = [(15, 65), (16, 128), (17, 129), (300, 200), (300, 256), (10, 200)]
SMALL_HYP = (0.37, 83.0, 0.11)            # alpha, beta, mean: nothing dyadic about them
WIDE_HYP = (2.0 ** -4, 2.0 ** 6, 2.0 ** -2)


class Problem(object):
    __slots__ = ("N", "z", "W", "b", "X", "Y", "Xg", "Z0", "Z1")


def problem(N, z, M, d=D):
    """The dyadic net, observations, responses and M candidate rows of one (N, z), with their exact features."""
    p = Problem()
    p.N, p.z = N, z
    p.W, p.b = dyadic_relu_net(d, z, 1000 * N + z)
    p.X, p.Xg = dyadic_points(N, d, 7 * N + z), dyadic_points(M, d, 11 * N + z + 1)
    p.Y = dyadic_responses(p.X, 13 * N + z)
    p.Z0, p.Z1 = dyadic_features(p.X, p.W, p.b), dyadic_features(p.Xg, p.W, p.b)
    return p


# ---- 50-digit truth --------------------------------------------------------------------------------------------------------
class BlrTruth(object):
    __slots__ = ("A", "m", "nll", "mu", "var", "raw")


def _exact_gram_mp(Z0):
    """Z0'Z0 of float64 features as exact integers over a common power of two (Python ints): (G, shift), Z0'Z0 = G 2^-shift."""
    rat = [[float(v).as_integer_ratio() for v in r] for r in Z0]
    k = max(d.bit_length() - 1 for r in rat for _, d in r)
    Zi = np.array([[n << (k - (d.bit_length() - 1)) for n, d in r] for r in rat], dtype=object)
    return Zi.T @ Zi, 2 * k


def blr_truth(Z0, y, alpha, beta, mean, Z1_rows, dps=50):
    """The head of the float64 inputs, taken as exact, at dps digits: A = beta Z0'Z0 + alpha I, m = A^-1 Z0' beta (y - mean), the
    evidence -log p(y | alpha, beta) of Bishop 3.82 / 3.86 as blr_fit_core states it, and mu_j = mean + phi_j . m,
    var_j = 1/beta + phi_j' A^-1 phi_j for the rows of Z1_rows.  Values as (hi, lo) pairs; .A is A rounded to float64 (for
    condition numbers), .raw the mpf values (m, nll, mu, var)."""
    Z0 = np.asarray(Z0, dtype=np.float64)
    yv = np.asarray(y, dtype=np.float64).ravel()
    N, z = Z0.shape
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        al, be, mn = mpf(float(alpha)), mpf(float(beta)), mpf(float(mean))
        G, shift = _exact_gram_mp(Z0)
        A = mpmath.matrix(z, z)
        for i in range(z):
            for j in range(i + 1):
                A[i, j] = A[j, i] = be * mpmath.ldexp(mpf(int(G[i, j])), -shift)
            A[i, i] += al
        r = [mpf(float(v)) - mn for v in yv]
        Zm = [[mpf(float(v)) for v in row] for row in Z0]
        q = mpmath.matrix([be * mpmath.fsum(Zm[i][k] * r[i] for i in range(N)) for k in range(z)])
        L = mpmath.cholesky(A)
        m = E._bwd(L, E._fwd(L, q))
        logdet = 2 * mpmath.fsum(mpmath.log(L[i, i]) for i in range(z))
        Em = be * mpmath.fsum(v * v for v in r) / 2 - mpmath.fsum(q[k] * m[k] for k in range(z)) / 2
        nll = -(z * mpmath.log(al) / 2 + N * mpmath.log(be) / 2 - Em - logdet / 2 - N * mpmath.log(2 * mpmath.pi) / 2)
        mu, var = [], []
        for row in np.asarray(Z1_rows, dtype=np.float64).reshape(-1, z):
            phi = mpmath.matrix([mpf(float(v)) for v in row])
            v = E._fwd(L, phi)
            mu.append(mn + mpmath.fsum(phi[k] * m[k] for k in range(z)))
            var.append(1 / be + mpmath.fsum(v[k] ** 2 for k in range(z)))
        t = BlrTruth()
        t.raw = ([m[k] for k in range(z)], nll, mu, var)
        t.m, t.nll, t.mu, t.var = E.pairs(t.raw[0]), E.pairs([nll]), E.pairs(mu), E.pairs(var)
        t.A = np.array([[float(A[i, j]) for j in range(z)] for i in range(z)])
        return t


def lapack_blr(Z0, y, alpha, beta, mean, Z1_rows):
    """oracle/blr.py's algebra in float64 on the same inputs: {"m", "nll", "mu", "var"}.  Its error against blr_truth is the
    yardstick of E.gp_bar."""
    from oracle import blr
    f = blr.fit(Z0, y, alpha, beta, mean)
    mu, var = blr.predict(f, np.asarray(Z1_rows, dtype=np.float64).reshape(-1, np.asarray(Z0).shape[1]))
    return {"m": f["m"], "nll": float(f["nll"]), "mu": mu[:, 0], "var": var}


def err_pairs(got, pair):
    """max |got - truth| against a (hi, lo) pair of arrays."""
    return float(np.max(E.abs_errors(np.asarray(got, dtype=np.float64).ravel(), pair[0], pair[1])))


# ---- heads too wide for a live truth: backward errors -----------------------------------------------------------------------
def lapack_head(A, q):
    """The library's algebra in LAPACK: A = L L' (dpotrf), L^-1 by forward substitution on the identity (dtrtrs, as
    test_factors_at_the_corners_have_lapack_sized_backward_errors forms its yardstick), m = L^-T (L^-1 q) -- the weights through the
    explicit inverse, as the device forms them (launch_trtri + launch_alpha), not through two triangular solves: the residual of
    the weights is then of order cond(L) eps on either side, and LAPACK doing the same algebra is the fair yardstick of it.
    Not dtrtri: its column sweep makes the LEFT residual X L - I, the one backward_errors measures, componentwise small (Higham,
    Accuracy and Stability, ch. 14), 3 to 6 times below what substitution on the identity or any blocked inversion leaves on these
    heads; the device's inverse sits within 1.1 x of dtrtrs's on every wide head and up to 6.8 x above dtrtri's."""
    L, info = lapack.dpotrf(A, lower=1, clean=1)
    assert info == 0
    Li = np.tril(solve_triangular(L, np.eye(L.shape[0]), lower=True))
    return L, Li, Li.T @ (Li @ q)


def solve_residual(A, m, q):
    """||A m - q|| / (||A|| ||m|| + ||q||) in long double (A and q exact in float64: exact_head)."""
    Al, ml, ql = (np.asarray(v, dtype=np.longdouble) for v in (A, np.ravel(m), np.ravel(q)))
    r = Al @ ml - ql
    return float(np.linalg.norm(r.astype(np.float64)) /
                 (np.linalg.norm(np.asarray(A, dtype=np.float64)) * np.linalg.norm(ml.astype(np.float64))
                  + np.linalg.norm(ql.astype(np.float64))))


# ---- exact evaluation of what the mean and variance kernels are given ------------------------------------------------------------
def _two_prod(a, b):
    """a b = p + e exactly (Dekker / Veltkamp; no overflow, e exact while |a b| >= 2^-969)."""
    p = a * b
    c = 134217729.0
    ah = c * a
    ah = ah - (ah - a)
    al = a - ah
    bh = c * b
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_sum(terms):
    """The exact sum of float64 terms as a (hi, lo) pair: hi correctly rounded (math.fsum), lo the rounded remainder."""
    terms = list(terms)
    hi = math.fsum(terms)
    return hi, math.fsum(terms + [-hi])


def exact_mean_rows(m, Phi, mean):
    """mean + phi . m for every row phi of Phi, from the float64 values themselves: (hi, lo), and sum |phi_k m_k| per row."""
    m = np.asarray(m, dtype=np.float64).ravel()
    Phi = np.asarray(Phi, dtype=np.float64)
    P, Er = _two_prod(Phi, m[None, :])
    out = [_dd_sum(list(P[j]) + list(Er[j]) + [float(mean)]) for j in range(Phi.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.abs(P).sum(1)


def exact_var_rows(Linv, Phi, invbeta):
    """invbeta + |Linv phi|^2 for every row phi, from the float64 values themselves (Linv lower triangular, invbeta the ROUNDED
    1/beta the kernel is handed): (hi, lo) pairs good to about 2^-100 relative."""
    Linv = np.tril(np.asarray(Linv, dtype=np.float64))
    Phi = np.asarray(Phi, dtype=np.float64)
    z = Linv.shape[0]
    hi, lo = np.empty(Phi.shape[0]), np.empty(Phi.shape[0])
    for j, phi in enumerate(Phi):
        P, Er = _two_prod(Linv, phi[None, :])
        v = [_dd_sum(list(P[i, :i + 1]) + list(Er[i, :i + 1])) for i in range(z)]
        vh, vl = np.array([t[0] for t in v]), np.array([t[1] for t in v])
        sq, sqe = _two_prod(vh, vh)
        hi[j], lo[j] = _dd_sum(list(sq) + list(sqe) + list(2.0 * vh * vl) + list(vl * vl) + [float(invbeta)])
    return hi, lo


def mean_bar(z, mean, abs_sum):
    """(z + 2) 2^-53 (|mean| + sum |phi_k m_k|), absolute: z products and z additions (the mean's included) in any order, fused or
    not -- the classical bound of a dot product of z + 1 terms."""
    return (z + 2) * U * (abs(mean) + abs_sum)


def var_bar(z, var_hi):
    """(z + 4) 2^-53 var, absolute: the sum of z non-negative terms v_i^2 (each a rounded or fused square) and one addition of the
    rounded 1/beta, in any order, errs by at most that.  The terms v_i = (Linv phi)_i are themselves rounded dot products; their
    share is not in the bar, which therefore also holds them to far less than their worst case (z 2^-53 sum_k |Linv_ik phi_k|
    each) -- tests/test_blr_host.py shows that numpy's own matrix product of the same operands stays within this bar (at
    most half of it) on every shape the GPU tests use."""
    return (z + 4) * U * var_hi
