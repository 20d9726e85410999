"""Host-side reference for tests/test_gpu_post_exact.py: what the posterior kernels (ksx_kernel + post_kernel_w4 / post_kernel_w4t /
post_small_kernel, and the fused kpost_small_kernel) must return for one candidate row x*, GIVEN the device's own L^-1 and alpha
(gp_download) and the float64 inputs taken as exact:

    k_i = cov(x*, x_i)                  the TRUE covariance entries, as (hi, lo) pairs from 50-digit arithmetic on an exact argument
    var = amp (+ noise) - |Linv k|^2    evaluated exactly (error-free products, double-double sums with an a-posteriori bound)
    mu  = mean + k . alpha              likewise

and the bars: a rounding term, E.gp_bar of numpy's own float64 error on the same operands, plus a first-order K* term that carries the
suite's per-entry covariance bars and the rounding of the argument as the device forms it (arg_gamma).  Nothing in a bar comes from
the device's output.  Also here: the case lists, the inputs, the judged rows and a float64 restatement of the device algebra, which
tests/test_post_exact_host.py uses to show that the bars can be met, are not vacuous, and catch seven kinds of wrong kernel.
No GPU needed."""
import math

import mpmath
import numpy as np
from scipy.linalg import lapack, solve_triangular

import _exact as E
from _blr_ref import _dd_sum, _two_prod

U = 2.0 ** -53
MI355X_CUS = 256                 # compute units of the machine the host tests size their grids for (device_info() on the GPU)
WORKSPACE_DEFAULT = 4 << 30      # b7_ctx::ks_bytes as a context starts
CAP = 1e-9                       # every bar / scale stays below this: four orders inside the 1e-5 of the parity tests
REF_GOOD = 2.0 ** -90            # what the exact evaluation promises, relative to its scale (asserted row by row)

SE, MATERN = "ardse", "ardmatern52"
# Test a: the general route on the default library (N, d, kernel) -- the smallest shapes at which each variance kernel instance
# and each slab class of the walk can go wrong.
CASES_A = [(64, 33, SE), (65, 40, MATERN), (129, 6, SE), (257, 3, MATERN), (400, 33, SE), (640, 17, SE), (700, 6, MATERN),
           (300, 65, SE)]
# Test b: the fused small-N posterior; and the same sizes through the general path of the diagnostic build.
CASES_B = [(63, 1, SE), (64, 6, MATERN), (65, 17, SE), (100, 32, MATERN), (128, 6, SE)]
CASES_B_GENERAL = [(100, 6, MATERN), (128, 6, SE)]
# Test c: S fits side by side (N, d, kernel, S, large grid?)
CASES_C = [(100, 6, SE, 3, False), (256, 6, MATERN, 4, True), (300, 6, SE, 4, True)]
CASE_D = (400, 33, SE)

FIXED_ROWS = (0, 1, 15, 16, 63, 64, 127, 128, 255, 256, 257)
OBS_COPIED = (0, 31, 32, 63, 64, 127, 128, 255, 256)      # and N - 1
OBS_PLACES = FIXED_ROWS[1:]                                  # the grid rows that hold them, in that order


def npad_of(N):
    return 64 if N <= 64 else -(-N // 128) * 128


def dpad_of(d):
    return 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 48 if d <= 48 else 64 if d <= 64 else 96


def m_small():
    return 4 * 256 + 13


def m_large(cus, S=1):
    """The smallest ragged grid with rows / 256 * S >= cus: 256 cus / S + 77 (65 613 on an MI355X at S = 1)."""
    return 256 * (-(-cus // S)) + 77


def chunk_rows(workspace_bytes, Npad, M):
    """predict_chunk of gp_api.hip: candidate rows per pass of the chunked posterior."""
    chunk = max(workspace_bytes // (8 * Npad) // 256 * 256, 256)
    return min(chunk, -(-M // 256) * 256)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def case_inputs(N, d, seed=None):
    """X uniform in [0, 1)^d, y a smooth function of X plus noise, lenscale_sq = d/8 (1 +- 0.3) per dimension, noise = 1e-3 amp."""
    rng = np.random.default_rng(1000 * N + d if seed is None else seed)
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(1) / math.sqrt(d)) + 0.3 * np.cos(7.0 * X[:, 0]) + 0.05 * rng.normal(size=N)
    y = (y - y.mean()) / y.std()
    amp, mean = 1.7, 0.3
    hyp = {"lenscale_sq": d / 8.0 * (1.0 + 0.3 * (2.0 * rng.random(d) - 1.0)), "amp": amp, "noise": 1e-3 * amp, "mean": mean}
    return X, (math.sqrt(amp) * y + mean).reshape(-1, 1), hyp


def hyper_samples(hyp, S):
    """The S hyper samples of test c: lengthscales and amplitude move, noise stays 1e-3 amp."""
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.25 * s), amp=hyp["amp"] * (1.0 + 0.1 * s),
                 noise=1e-3 * hyp["amp"] * (1.0 + 0.1 * s)) for s in range(S)]


def make_grid(M, X, seed=None):
    """M seeded uniform rows; rows OBS_PLACES are overwritten by observations OBS_COPIED and N - 1 (those below N), so that single
    columns of K* carry amp itself.  make_grid(M1, ...) is the head of make_grid(M2, ...) for M1 < M2 >= 258 only through
    slicing: take the larger grid and cut it."""
    N, d = X.shape
    rng = np.random.default_rng(7 * N + d if seed is None else seed)
    G = rng.random((M, d))
    obs = sorted({j for j in OBS_COPIED + (N - 1,) if j < N})
    for place, j in zip(OBS_PLACES, obs):
        G[place] = X[j]
    return G


def judged_rows(M, chunk=None, seed=0):
    """The rows a case is judged on: FIXED_ROWS, the last three rows (of the ragged final tile), both sides of every chunk boundary
    and 24 seeded random rows."""
    rows = {r for r in FIXED_ROWS if r < M} | {r for r in (M - 3, M - 2, M - 1) if r >= 0}
    if chunk:
        for c in range(chunk, M, chunk):
            rows |= {c - 1, c}
    rng = np.random.default_rng(seed + M)
    rows |= set(int(r) for r in rng.choice(M, min(24, M), replace=False))
    return np.array(sorted(rows), dtype=np.int64)


# ---- the true covariance entries ---------------------------------------------------------------------------------------------------
def _to_ints(a):
    """A float64 array as Python integers over a common power of two: (n, q) with a = n 2^-q exactly."""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = np.ldexp(m, 53).astype(np.int64)
    ee = e.astype(np.int64) - 53
    nz = mi != 0
    q = max(int(-ee[nz].min()), 0) if nz.any() else 0
    sh = np.where(nz, ee + q, 0).astype(object)
    return mi.astype(object) * (2 ** sh), q


FRAC_BITS = 200


def exact_args(Xs, X, lenscale_sq):
    """arg = -1/2 sum_k (x*_k - x_ik)^2 / lenscale_sq_k of the float64 values, in rational arithmetic: integers T (rows x N, an
    object array) and a shift with arg = -T 2^-shift, each term floored at 2^-(FRAC_BITS + 2 q): an absolute error below 2^-200."""
    R, N, d = len(Xs), len(X), X.shape[1]
    ints, q = _to_ints(np.concatenate([np.asarray(Xs, dtype=np.float64), np.asarray(X, dtype=np.float64)]))
    xs, xo = ints[:R], ints[R:]
    num = np.empty(d, dtype=object)
    den = np.empty(d, dtype=object)
    for k, v in enumerate(np.asarray(lenscale_sq, dtype=np.float64).ravel()):
        a, b = float(v).as_integer_ratio()
        num[k], den[k] = a, b << FRAC_BITS
    T = np.empty((R, N), dtype=object)
    for r in range(R):
        df = xo - xs[r][None, :]
        T[r] = ((df * df * den[None, :]) // num[None, :]).sum(axis=1)
    return T, 2 * q + FRAC_BITS + 1


class Cov(object):
    __slots__ = ("hi", "lo", "g", "s")


def true_cov_rows(Xs, X, lenscale_sq, amp, kernel, dps=50):
    """k_i = cov(x*, x_i) per row x* of Xs: (hi, lo) pairs of amp exp(arg) (ARD-SE) or amp (1 + s + s^2/3) exp(-s), s = sqrt(-10 arg)
    (Matern-5/2), at dps digits on exact_args' argument; g = |dk/darg| (k itself; (5/3) amp (1 + s) exp(-s): cov_grad_nonpos4) and
    s (zeros for ARD-SE) in float64."""
    T, shift = exact_args(Xs, X, lenscale_sq)
    out = Cov()
    out.hi, out.lo, out.g, out.s = (np.empty(T.shape) for _ in range(4))
    with mpmath.workdps(dps):
        A = mpmath.mpf(float(amp))
        for r in range(T.shape[0]):
            for i in range(T.shape[1]):
                arg = mpmath.ldexp(mpmath.mpf(-T[r, i]), -shift)
                if kernel == SE:
                    k = A * mpmath.exp(arg)
                    g, s = k, 0.0
                else:
                    s = mpmath.sqrt(-10 * arg)
                    e = A * mpmath.exp(-s)
                    k = (1 + s + s * s / 3) * e
                    g = 5 * (1 + s) * e / 3
                out.hi[r, i], out.lo[r, i] = E.mp_to_pair(k)
                out.g[r, i], out.s[r, i] = float(g), float(s)
    return out


# ---- the bars -------------------------------------------------------------------------------------------------------------------
def arg_gamma(dpad):
    """gamma_n = n u / (1 - n u), n = dpad + 4: the relative rounding bound, term by term, of the argument as the device forms it,
        arg_dev = (c - xs/2) - zs/2          (ksx_walk.h: arg4; kpost_small_kernel states the same line)
    against the exact -1/2 sum_k (x_k - z_k)^2 / l_k = sum_k x_k z_k / l_k - 1/2 sum_k x_k^2 / l_k - 1/2 sum_k z_k^2 / l_k.  Counting
    the roundings on any one term of each sum:
      c     w_k = fl(1 / l_k) and zsc_k = fl(z_k w_k) (prep_obs_kernel; gp_small_body.h): 2.  The MFMA chain over dpad k-steps is a
            fused multiply-add per term, started at 0: the first term meets dpad roundings, later ones fewer (padding terms are
            exact zeros): dpad.  The two subtractions each round a quantity that contains c: 2.         dpad + 4
      xs/2  w_k: 1; fl(x_k^2): 1; its product with w_k: 1; `s += t` over dpad terms started at 0 (0 + t is exact): dpad - 1;
            the halving is exact; two subtractions: 2.  A compiler that contracts the product into an fma rounds less. dpad + 4
      zs/2  the same sum, in one subtraction only.                                                                    dpad + 3
    so |arg_dev - arg| <= gamma_(dpad+4) (sum_k |x_k zsc_k| + xs/2 + zs/2) (Higham, Accuracy and Stability, lemma 3.1: a product of
    n factors (1 + delta_i), |delta_i| <= u, is 1 + theta with |theta| <= gamma_n).  The clamp min(arg_dev, 0) moves arg_dev
    towards the exact argument, which is never positive."""
    n = dpad + 4
    return n * U / (1.0 - n * U)


def arg_bound(Xs, X, lenscale_sq):
    """delta_a (rows x N): arg_gamma (sum_k |x*_k zsc_ik| + xs/2 + zs/2), the magnitudes in float64."""
    Xs, X = np.asarray(Xs, dtype=np.float64), np.asarray(X, dtype=np.float64)
    w = 1.0 / np.asarray(lenscale_sq, dtype=np.float64).ravel()
    mag = np.abs(Xs) @ np.abs(X * w).T + (0.5 * ((Xs * Xs) @ w))[:, None] + (0.5 * ((X * X) @ w))[None, :]
    return arg_gamma(dpad_of(X.shape[1])) * mag


def cov_entry_bar(k, s, kernel):
    """B_cov: what the suite already asserts for one covariance entry formed from an exact argument -- 4 ulp of the true value for
    ARD-SE (tests/test_gpu_numerics.py, section A), (4 + s) ulp for Matern-5/2 (tests/_matern_ref.py: within_matern_bar); below the
    normal range 2^-1073 absolute (plus the Matern's relative s term)."""
    k = np.abs(k)
    normal = k >= E.TINY
    ulps = 4.0 + (s if kernel == MATERN else 0.0)
    sub = E.SUB_BAR + (s * E.EPS * k if kernel == MATERN else 0.0)
    return np.where(normal, ulps * E.ulp_of(np.where(normal, k, 1.0)), sub)


def kstar_bound(cov, delta_a, kernel):
    """delta_k_i = B_cov + g_i delta_a_i, to first order in delta_a.  B_cov is taken at the value the device's own argument can
    reach, |k_i| + g_i delta_a_i (it may lie in the next binade)."""
    shift = cov.g * delta_a
    return cov_entry_bar(np.abs(cov.hi) + shift, cov.s, kernel) + shift


# ---- the exact posterior of float64 operands ---------------------------------------------------------------------------------
def _two_sum(a, b):
    """a + b = s + e exactly (Knuth)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _dd_tree(hi, lo):
    """The sum over the last axis of double-double terms (hi, lo), pairwise: (hi, lo, levels).  Each level errs by at most
    3 u^2 (|a| + |b|) per addition (the low parts' sum and its addition to the exact error term round; the two_sums do not), so the
    whole tree by at most levels 2^-104 sum |hi|."""
    levels = 0
    while hi.shape[-1] > 1:
        if hi.shape[-1] & 1:
            pad = np.zeros(hi.shape[:-1] + (1,))
            hi, lo = np.concatenate([hi, pad], -1), np.concatenate([lo, pad], -1)
        s, e = _two_sum(hi[..., 0::2], hi[..., 1::2])
        hi, lo = _two_sum(s, e + (lo[..., 0::2] + lo[..., 1::2]))
        levels += 1
    return hi[..., 0], lo[..., 0], levels


class Post(object):
    __slots__ = ("mu", "var", "scale_m", "scale_v", "v", "ref_err_v", "ref_err_m")


def exact_post_rows(Linv, alpha, k_hi, k_lo, amp, add, mean):
    """var = amp + add - |Linv k|^2 and mu = mean + k . alpha for k = k_hi + k_lo, row by row, from the float64 values themselves.
    The products Linv_ji k_hi_i are split without error (_two_prod), Linv_ji k_lo_i is rounded (2^-106 of the term), v_j is their
    double-double tree sum, v_j^2 is expanded without error, and the final sums are exact (_dd_sum).  What is not exact is bounded
    a posteriori, per row: ref_err_v = sum_j 2 |v_j| (levels + 2) 2^-104 sum_i |Linv_ji k_i| + 2^-103 |v|^2, asserted below
    REF_GOOD (amp + add + |v|^2).  Returns (hi, lo) pairs, the scales amp + add + |v|^2 and |mean| + sum |k_i alpha_i|, and |v|."""
    Linv = np.tril(np.asarray(Linv, dtype=np.float64))
    al = np.asarray(alpha, dtype=np.float64).ravel()
    R = k_hi.shape[0]
    out = Post()
    out.mu, out.var = (np.empty(R), np.empty(R)), (np.empty(R), np.empty(R))
    out.scale_m, out.scale_v, out.ref_err_v, out.ref_err_m = (np.empty(R) for _ in range(4))
    out.v = np.empty((R, Linv.shape[0]))
    for r in range(R):
        P, Er = _two_prod(Linv, k_hi[r][None, :])
        vh, vl, levels = _dd_tree(P, Er + Linv * k_lo[r][None, :])
        dv = (levels + 2) * 2.0 ** -104 * np.abs(P).sum(1)
        sq, sqe = _two_prod(vh, vh)
        terms = [float(amp), float(add)] + (-sq).tolist() + (-sqe).tolist() + (-2.0 * vh * vl).tolist() + (-(vl * vl)).tolist()
        out.var[0][r], out.var[1][r] = _dd_sum(terms)
        vv = float(sq.sum())
        out.scale_v[r] = abs(amp) + abs(add) + vv
        out.ref_err_v[r] = float((2.0 * np.abs(vh) * dv).sum()) + 2.0 ** -103 * vv
        out.v[r] = vh
        Pm, Em = _two_prod(k_hi[r], al)
        Lm = k_lo[r] * al
        out.mu[0][r], out.mu[1][r] = _dd_sum([float(mean)] + Pm.tolist() + Em.tolist() + Lm.tolist())
        out.scale_m[r] = abs(mean) + float(np.abs(Pm).sum())
        out.ref_err_m[r] = 2.0 ** -105 * float(np.abs(Pm).sum())
    assert np.all(out.ref_err_v <= REF_GOOD * out.scale_v) and np.all(out.ref_err_m <= REF_GOOD * out.scale_m), \
        "the reference is not good to 2^-90: %.3g, %.3g" % (float(np.max(out.ref_err_v / out.scale_v)),
                                                            float(np.max(out.ref_err_m / out.scale_m)))
    return out


def mp_post_rows(Linv, alpha, k_hi, k_lo, amp, add, mean, dps=50):
    """The same formula in plain dps-digit arithmetic: (mu, var) as lists of mpf."""
    Linv = np.tril(np.asarray(Linv, dtype=np.float64))
    al = np.asarray(alpha, dtype=np.float64).ravel()
    n = Linv.shape[0]
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        mu, var = [], []
        for r in range(k_hi.shape[0]):
            k = [mpf(float(k_hi[r, i])) + mpf(float(k_lo[r, i])) for i in range(n)]
            v = [mpmath.fsum(mpf(float(Linv[j, i])) * k[i] for i in range(j + 1)) for j in range(n)]
            var.append(mpf(float(amp)) + mpf(float(add)) - mpmath.fsum(x * x for x in v))
            mu.append(mpf(float(mean)) + mpmath.fsum(k[i] * mpf(float(al[i])) for i in range(n)))
    return mu, var


def numpy_post(Ks, Linv, alpha, amp, add, mean):
    """The float64 evaluation of the same operands: mean + Ks alpha, (amp - colsumsq(Linv Ks')) + add (the kernels' statement)."""
    V = Ks @ np.tril(np.asarray(Linv, dtype=np.float64)).T
    return mean + Ks @ np.asarray(alpha, dtype=np.float64).ravel(), (amp - (V * V).sum(1)) + add


class Ref(object):
    __slots__ = ("rows", "cov", "post", "bar_m", "bar_v", "share_m", "share_v", "e_np_m", "e_np_v", "with_noise")

    def pick(self, rows):
        """Positions in this reference of the grid rows `rows`."""
        pos = np.searchsorted(self.rows, rows)
        assert np.array_equal(self.rows[pos], rows)
        return pos


def reference(X, hyp, kernel, Linv, alpha, G, rows, with_noise=False, cov=None):
    """The reference and the bars of grid rows `rows` (sorted) of G under one fit.  bar = E.gp_bar(e_np, scale) + K* term per row,
    absolute: e_np is the worst error over these rows of numpy's float64 evaluation of the same operands (k_hi, Linv, alpha)
    against the exact value -- the yardstick is the reference's error, never the device's --, scale_v = amp (+ noise) + |v|^2,
    scale_m = |mean| + sum |k_i alpha_i|, and the K* term is, to first order in delta_k,
        variance  sum_j 2 |v_j| sum_i |Linv_ji| delta_k_i,        mean  sum_i |alpha_i| delta_k_i         (kstar_bound)."""
    ls, amp, mean = hyp["lenscale_sq"], hyp["amp"], hyp["mean"]
    add = hyp["noise"] if with_noise else 0.0
    N = X.shape[0]
    Linv = np.tril(np.asarray(Linv, dtype=np.float64)[:N, :N])
    al = np.asarray(alpha, dtype=np.float64).ravel()[:N]
    Xs = G[rows]
    ref = Ref()
    ref.rows, ref.with_noise = np.asarray(rows, dtype=np.int64), with_noise
    ref.cov = true_cov_rows(Xs, X, ls, amp, kernel) if cov is None else cov
    ref.post = exact_post_rows(Linv, al, ref.cov.hi, ref.cov.lo, amp, add, mean)
    mu_np, var_np = numpy_post(ref.cov.hi, Linv, al, amp, add, mean)
    ref.e_np_m = float(np.max(E.abs_errors(mu_np, *ref.post.mu)))
    ref.e_np_v = float(np.max(E.abs_errors(var_np, *ref.post.var)))
    dk = kstar_bound(ref.cov, arg_bound(Xs, X, ls), kernel)
    ks_m = dk @ np.abs(al)
    ks_v = 2.0 * np.einsum("rj,rj->r", np.abs(ref.post.v), dk @ np.abs(Linv).T)
    ref.bar_m = E.gp_bar(ref.e_np_m, ref.post.scale_m) + ks_m
    ref.bar_v = E.gp_bar(ref.e_np_v, ref.post.scale_v) + ks_v
    ref.share_m, ref.share_v = ks_m / ref.bar_m, ks_v / ref.bar_v
    return ref


def judge(ref, rows, mu, var):
    """error / bar of the device's (or a restatement's) mu and var at grid rows `rows`, per row: (mean ratios, variance ratios)."""
    pos = ref.pick(rows)
    mu, var = np.asarray(mu, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
    em = E.abs_errors(mu, ref.post.mu[0][pos], ref.post.mu[1][pos])
    ev = E.abs_errors(var, ref.post.var[0][pos], ref.post.var[1][pos])
    return em / ref.bar_m[pos], ev / ref.bar_v[pos]


def within(ratios):
    """Every row inside its bar (a NaN is outside)."""
    return bool(np.all(ratios <= 1.0))


# ---- the device algebra restated in float64 (host tests) -----------------------------------------------------------------------
def device_kstar(Xs, X, lenscale_sq, amp, kernel):
    """K(X*, X) as the device forms it, in numpy: w = 1 / l, zsc = X w, c = X* zsc', arg = min((c - xs/2) - zs/2, 0), then the
    covariance function through np.exp (and np.sqrt)."""
    Xs, X = np.asarray(Xs, dtype=np.float64), np.asarray(X, dtype=np.float64)
    w = 1.0 / np.asarray(lenscale_sq, dtype=np.float64).ravel()
    hq, hk = 0.5 * ((Xs * Xs) @ w), 0.5 * ((X * X) @ w)
    arg = np.minimum(((Xs @ (X * w).T) - hq[:, None]) - hk[None, :], 0.0)
    if kernel == SE:
        return amp * np.exp(arg)
    s = np.sqrt(-10.0 * arg)
    return amp * (1.0 + s * (1.0 + s / 3.0)) * np.exp(-s)


def host_fit(X, Y, hyp, kernel):
    """K by device_kstar with amp + noise on the diagonal, L by LAPACK (no jitter: info must be 0), L^-1 by substitution on the
    identity, alpha = L^-T (L^-1 (y - mean)): (L, Linv, alpha, cond(K))."""
    K = device_kstar(X, X, hyp["lenscale_sq"], hyp["amp"], kernel)
    K[np.diag_indices(len(X))] = hyp["amp"] + hyp["noise"]
    L, info = lapack.dpotrf(K, lower=1, clean=1)
    assert info == 0, "LAPACK needs jitter: info %d" % info
    Linv = np.tril(solve_triangular(L, np.eye(len(X)), lower=True))
    return L, Linv, Linv.T @ (Linv @ (np.asarray(Y, dtype=np.float64).ravel() - hyp["mean"])), float(np.linalg.cond(K))


def all_cases(cus=MI355X_CUS):
    """Every (name, N, d, kernel, hyp, [M, ...]) of the GPU file, once per distinct fit."""
    out = []
    for N, d, kern in CASES_A:
        out.append(("a", N, d, kern, case_inputs(N, d)[2], [m_small(), m_large(cus)]))
    for N, d, kern in CASES_B + CASES_B_GENERAL[:1]:
        out.append(("b", N, d, kern, case_inputs(N, d)[2], [m_small()]))
    for N, d, kern, S, large in CASES_C:
        for s, h in enumerate(hyper_samples(case_inputs(N, d)[2], S)):
            out.append(("c%d" % s, N, d, kern, h, [m_large(cus, 4) if large else m_small()]))
    return out


def case_rows(Ms, chunks=None):
    """The grid (its size) and the judged rows of a case run at the grid sizes Ms: every smaller grid is the head of the largest."""
    rows = [judged_rows(M, None if chunks is None else chunks[i]) for i, M in enumerate(Ms)]
    return max(Ms), rows, np.unique(np.concatenate(rows))
