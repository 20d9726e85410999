"""References for Thompson sampling (tests/test_ts_host.py, tests/test_gpu_ts.py).  No GPU needed here.

  * the library's counter generator (bot7_amd/csrc/counter_rng.h: splitmix64 -> Box-Muller) and b7_ts_nominate's counter layout,
    restated in numpy: draws(seed, path, ...) is what b7_ts_last_draws must return;
  * paths_ref: the pathwise posterior sample f_j(x) = m + phi(x)' w_j + K(x, X) inv(K) (y - m - Phi(X) w_j - eps_j) in float64 with
    np.linalg.solve on K;
  * rff_exact: cos(X Omega' + phase) W at 50 digits.  The inputs are doubles, hence exact rationals: both products are exact
    integer arithmetic (Python ints), only the cosine itself is mpmath's (its fixed-point kernel, 60 digits); the result is rounded once, to a
    (hi, lo) pair of doubles."""
from fractions import Fraction

import mpmath
import numpy as np
from mpmath.libmp import libelefun

DPS = 50
G = np.uint64(0x9E3779B97F4A7C15)
TWO_M53 = 1.1102230246251565404e-16
TWO_PI = 6.283185307179586476925
BASIS_STRIDE, CHI_OFF, PHASE_OFF, EPS_OFF = 128, 96, 101, 4096


# ---- the generator --------------------------------------------------------------------------------------------------------------
def splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _hashes(key, ctr):
    ctr = np.asarray(ctr, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = splitmix64(np.uint64(key) + G * (np.uint64(2) * ctr + np.uint64(1)))
        b = splitmix64(np.uint64(key) + G * (np.uint64(2) * ctr + np.uint64(2)))
    return a, b


def counter_normal(key, ctr):
    a, b = _hashes(key, ctr)
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * TWO_M53
    u2 = (b >> np.uint64(11)).astype(np.float64) * TWO_M53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI * u2)


def counter_uniform(key, ctr):
    a, _ = _hashes(key, ctr)
    return (a >> np.uint64(11)).astype(np.float64) * TWO_M53


def counter_key(seed, stream):
    return splitmix64(splitmix64(np.uint64(seed)) ^ np.uint64(stream))


def basis(seed, F, d, lenscale_sq, kernel="ardse"):
    """(omega F x d, phase F): stream 0 of the seed; feature f owns the counters 128 f .. 128 f + 127."""
    key = counter_key(seed, 0)
    f = np.arange(F, dtype=np.uint64)[:, None] * np.uint64(BASIS_STRIDE)
    z = counter_normal(key, f + np.arange(d, dtype=np.uint64)[None, :])
    if kernel == "ardmatern52":
        g = counter_normal(key, f + np.uint64(CHI_OFF) + np.arange(5, dtype=np.uint64)[None, :])
        u = np.zeros(F)
        for i in range(5):
            u = u + g[:, i] * g[:, i]
        z = z * np.sqrt(5.0 / u)[:, None]
    inv_ls = 1.0 / np.sqrt(np.asarray(lenscale_sq, dtype=np.float64).ravel())
    phase = TWO_PI * counter_uniform(key, f.ravel() + np.uint64(PHASE_OFF))
    return z * inv_ls[None, :], phase


def draws(seed, path, F, d, N, lenscale_sq, noise, kernel="ardse"):
    """Path `path`'s draws under its hyper sample's lengthscales and noise, as b7_ts_last_draws returns them."""
    omega, phase = basis(seed, F, d, lenscale_sq, kernel)
    key = counter_key(seed, 1 + path)
    weight = counter_normal(key, np.arange(F, dtype=np.uint64))
    eps = np.sqrt(noise) * counter_normal(key, np.uint64(EPS_OFF) + np.arange(N, dtype=np.uint64))
    return {"omega": omega, "phase": phase, "weight": weight, "eps": eps}


def ulps(got, want):
    """|got - want| in units of the last place of want."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


# ---- the paths ------------------------------------------------------------------------------------------------------------------
def cov(X, Z, lenscale_sq, amp, kernel="ardse"):
    X, Z = np.atleast_2d(np.asarray(X, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    w = 1.0 / np.asarray(lenscale_sq, dtype=np.float64).ravel()
    D = np.zeros((len(X), len(Z)))
    for k in range(X.shape[1]):
        D += (X[:, k][:, None] - Z[:, k][None, :]) ** 2 * w[k]
    if kernel == "ardse":
        return amp * np.exp(-0.5 * D)
    s = np.sqrt(5.0 * D)
    return amp * (1.0 + s + s * s / 3.0) * np.exp(-s)


def features(X, omega, phase, amp):
    return np.sqrt(2.0 * amp / len(phase)) * np.cos(np.asarray(X, dtype=np.float64) @ omega.T + phase[None, :])


def paths_ref(X, y, Xs, hyp, kernel, draws_, jitter=0.0, want_v=False):
    """The q = len(draws_) sample paths over Xs (M x q).  hyp: one hyper sample, or a list of S of them (path j is drawn under
    hyp[j mod S]).  jitter: what the factorisation put on K's diagonal beside the noise (one value, or one per hyper sample);
    eps keeps the hyper sample's own noise."""
    X, Xs, y = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
    hyps = hyp if isinstance(hyp, (list, tuple)) else [hyp]
    jit = np.broadcast_to(np.asarray(jitter, dtype=np.float64), (len(hyps),))
    out, vs = np.empty((len(Xs), len(draws_))), []
    for j, dr in enumerate(draws_):
        h, s = hyps[j % len(hyps)], j % len(hyps)
        K = cov(X, X, h["lenscale_sq"], h["amp"], kernel) + (h["noise"] + max(float(jit[s]), 0.0)) * np.eye(len(X))
        r = y - h["mean"] - features(X, dr["omega"], dr["phase"], h["amp"]) @ dr["weight"] - dr["eps"]
        v = np.linalg.solve(K, r)
        out[:, j] = h["mean"] + features(Xs, dr["omega"], dr["phase"], h["amp"]) @ dr["weight"] + cov(Xs, X, h["lenscale_sq"], h["amp"], kernel) @ v
        vs.append(v)
    return (out, vs) if want_v else out


def nominees_ref(paths):
    """The rule of b7_ts_nominate on a reference: paths in order, each its first minimum over the rows not taken earlier, a NaN
    never winning.  Returns 0-based rows."""
    taken = []
    for j in range(paths.shape[1]):
        col = np.where(np.isnan(paths[:, j]), np.inf, paths[:, j]).copy()
        col[taken] = np.inf
        free = [i for i in range(len(col)) if i not in taken]
        taken.append(int(np.argmin(col)) if np.isfinite(col[free]).any() else free[0])
    return taken


# ---- cos(X Omega' + phase) W at 50 digits ------------------------------------------------------------------------------------
def _fixed(a):
    """A float64 array as (object array of Python ints, k) with a = ints / 2^k exactly."""
    a = np.asarray(a, dtype=np.float64)
    fr = [Fraction(float(v)) for v in a.ravel()]
    k = max(f.denominator.bit_length() - 1 for f in fr)
    ints = np.array([f.numerator * ((1 << k) // f.denominator) for f in fr], dtype=object).reshape(a.shape)
    return ints, k


COS_BITS = 200


def rff_exact(X, omega, phase, W):
    """(hi, lo): hi + lo = cos(X omega' + phase) W to ~1e-48 relative to sum |W| (50-digit cosines of exact arguments, exact
    sums), M1 x q each."""
    Xi, kx = _fixed(X)
    Oi, ko = _fixed(omega)
    Pi, kp = _fixed(phase)
    Wi, kw = _fixed(W)
    if kp < kx + ko:
        Pi, kp = Pi * (1 << (kx + ko - kp)), kx + ko
    args = Xi.dot(Oi.T) * (1 << (kp - kx - ko)) + Pi[None, :]          # exact, over 2^kp
    # 50-digit cosines in fixed point (mpmath's own integer kernel, COS_BITS + 32 bits of working precision: ~1e-60 absolute)
    wp = COS_BITS + 32
    pi2 = libelefun.pi_fixed(wp - 1)
    fix = (lambda a: a << (wp - kp)) if wp >= kp else (lambda a: a >> (kp - wp))
    cosi = np.array([libelefun.cos_sin_fixed(fix(int(a)), wp, pi2)[0] >> 32 for a in args.ravel()], dtype=object).reshape(args.shape)
    tot = cosi.dot(Wi)                                                  # over 2^(COS_BITS + kw)
    hi = np.empty(tot.shape)
    lo = np.empty(tot.shape)
    for idx, t in np.ndenumerate(tot):
        fr = Fraction(int(t), 1 << (COS_BITS + kw))
        h = float(fr)
        hi[idx], lo[idx] = h, float(fr - Fraction(h))
    return hi, lo


def err_vs_exact(got, hi, lo):
    """max |got - (hi + lo)|, the subtraction of hi being exact where it matters (Sterbenz)."""
    return float(np.max(np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)))
