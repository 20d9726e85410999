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
        free = np.ones(len(col), dtype=bool)
        free[taken] = False
        taken.append(int(np.argmin(col)) if np.isfinite(col[free]).any() else int(np.flatnonzero(free)[0]))
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


# ---- the paths held to exact arithmetic (tests/test_ts_exact_host.py, tests/test_gpu_ts_exact.py) ---------------------------------
# What rff_kernel and the mean kernels must return for one grid row x and one path j, GIVEN the device's own alpha column of the
# pseudo-response fit (diagnostic build: b7dbg_ts_alpha) and its own draws, the float64 inputs taken as exact:
#     f_j(x) = [m + sum_i k(x, x_i) alpha_ij] + [sum_f W'_fj cos(omega_f . x + phase_f)],   W'_fj = fl(sqrt(2 amp / F) weight_jf)
# k as (hi, lo) pairs from 50 digits on an exact argument (_post_ref.true_cov_rows), error-free products, exact sums; the prior term
# by rff_exact.  The bar per row, nothing of it from the device's output:
#     gp_bar(e_np, scale_m)            e_np: numpy float64's own error on m + k_hi . alpha over the judged rows
#   + sum_i |alpha_i| dk_i             _post_ref.kstar_bound: the suite's per-entry covariance bars and the argument's counted roundings
#   + 16 e_rff + 1e-15 sum_f |W'_f|    test_gpu_ts.rff_check's bar; e_rff: numpy's error on cos(X omega' + phase) W' over the judged rows
#   + 2 u |f_j(x)|                     the final add base + acc (one rounding; 2 u leaves room for the value's own rounding to a double)
# and scale = |m| + sum_i |k_i alpha_i| + sum_f |W'_f|; bar / scale <= CAP on every judged row.
import functools  # noqa: E402

import _exact as E  # noqa: E402
import _post_ref as PR  # noqa: E402
from _blr_ref import _dd_sum, _two_prod  # noqa: E402

U = 2.0 ** -53
CAP = PR.CAP
SEED = 20261
EXACT_ND = [(5, 3), (64, 9), (65, 33), (129, 65), (300, 6)]          # rff dpad 8 / 16 / 64 / 96 / 8, Npad 64 / 64 / 128 / 256 / 384
EXACT_SQ = [(1, 1), (1, 16), (3, 5), (3, 16)]                          # qs == 1 alone; 16; 2, 2, 1; 6, 5, 5
EXACT_FM = [(16, 7), (256, 1037), (16, 1037), (256, 7)]
KERNELS = [PR.SE, PR.MATERN]


def exact_cases():
    """(N, d, kernel, S, q, F, M): every (N, d) x kernel x (S, q); (F, M) rotates so that each of its four pairs meets every
    (N, d), every kernel and every (S, q)."""
    out = []
    for a, (N, d) in enumerate(EXACT_ND):
        for b, kern in enumerate(KERNELS):
            for c, (S, q) in enumerate(EXACT_SQ):
                F, M = EXACT_FM[(a + b + c) % 4]
                out.append((N, d, kern, S, min(q, M), F, M))
    return out


def packed_weights(weight, amp, F):
    """W' = fl(scale weight), scale = sqrt(2 amp / F) as the host forms it: rff_pack_kernel's single rounding."""
    return np.sqrt(2.0 * amp / F) * np.asarray(weight, dtype=np.float64)


def case_problem(N, d, S, M):
    """Inputs, hyper samples, grid and judged rows of one case (_post_ref's constructors)."""
    X, Y, hyp = PR.case_inputs(N, d)
    return X, Y, PR.hyper_samples(hyp, S), PR.make_grid(max(M, 258), X)[:M], PR.judged_rows(M)


@functools.lru_cache(maxsize=None)
def case_cov(N, d, kern, M, s):
    """true_cov_rows of a case's judged rows under hyper sample s, once (sample s is the same whatever S >= s + 1 is)."""
    X, _, hyps, G, rows = case_problem(N, d, s + 1, M)
    return PR.true_cov_rows(G[rows], X, hyps[s]["lenscale_sq"], hyps[s]["amp"], kern)


class PathRef(object):
    __slots__ = ("hi", "lo", "bar", "scale", "e_np", "e_rff", "ks_share", "rows")


def paths_exact(X, Xs, hyps, kernel, draws_, alphas, covs=None):
    """Reference, bars and scales (rows x q) of the q = len(draws_) paths at the rows Xs.  hyps: the S hyper samples; alphas[s]: the
    N x qs alpha columns of sample s (column p belongs to path s + S p); covs[s] (optional): true_cov_rows of Xs under sample s."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    S, q, R = len(hyps), len(draws_), len(Xs)
    ref = PathRef()
    ref.hi, ref.lo, ref.bar, ref.scale, ref.ks_share = (np.empty((R, q)) for _ in range(5))
    ref.e_np, ref.e_rff = np.empty(q), np.empty(q)
    for s in range(min(S, q)):
        h = hyps[s]
        cov = covs[s] if covs is not None else PR.true_cov_rows(Xs, X, h["lenscale_sq"], h["amp"], kernel)
        dk = PR.kstar_bound(cov, PR.arg_bound(Xs, X, h["lenscale_sq"]), kernel)
        js = list(range(s, q, S))
        F = len(draws_[s]["phase"])
        Wp = np.stack([packed_weights(draws_[j]["weight"], h["amp"], F) for j in js], axis=1)
        rh, rl = rff_exact(Xs, draws_[s]["omega"], draws_[s]["phase"], Wp)
        r_np = np.cos(Xs @ draws_[s]["omega"].T + draws_[s]["phase"][None, :]) @ Wp
        for p, j in enumerate(js):
            al = np.asarray(alphas[s], dtype=np.float64)[:, p]
            Pm, Em = _two_prod(cov.hi, al[None, :])
            Lm = cov.lo * al[None, :]
            gp = [_dd_sum([float(h["mean"])] + Pm[r].tolist() + Em[r].tolist() + Lm[r].tolist()) for r in range(R)]
            gh, gl = np.array([g[0] for g in gp]), np.array([g[1] for g in gp])
            scale_m = abs(h["mean"]) + np.abs(Pm).sum(1)
            e_np = float(np.max(E.abs_errors(h["mean"] + cov.hi @ al, gh, gl)))
            e_rff = float(np.max(E.abs_errors(r_np[:, p], rh[:, p], rl[:, p])))
            tot = [_dd_sum([gh[r], gl[r], rh[r, p], rl[r, p]]) for r in range(R)]
            ref.hi[:, j], ref.lo[:, j] = [t[0] for t in tot], [t[1] for t in tot]
            sw = float(np.abs(Wp[:, p]).sum())
            ks = dk @ np.abs(al)
            ref.bar[:, j] = E.gp_bar(e_np, scale_m) + ks + (16.0 * e_rff + 1e-15 * sw) + 2.0 * U * np.abs(ref.hi[:, j])
            ref.scale[:, j] = scale_m + sw
            ref.ks_share[:, j] = ks / ref.bar[:, j]
            ref.e_np[j], ref.e_rff[j] = e_np, e_rff
    return ref


def judge_paths(ref, P):
    """error / bar of paths P (rows x q) against the reference, entry by entry."""
    return E.abs_errors(np.asarray(P, dtype=np.float64), ref.hi, ref.lo) / ref.bar


def identity_residual(P_obs, draws_, alphas, y, hyps, jitter, K_norms):
    """max_i |paths(x_i) + eps_i + (noise + jitter) alpha_i - y_i| per path, and its bound 64 N 2^-53 ||K||_inf max |alpha|
    (test_gpu_ts.test_path_identity_on_the_device).  P_obs: N x q, the paths at the observations; K_norms[s]: ||K_s||_inf."""
    S, q, N = len(hyps), len(draws_), len(y)
    y = np.asarray(y, dtype=np.float64).ravel()
    res, bound = np.empty(q), np.empty(q)
    for j in range(q):
        s, p = j % S, j // S
        al = np.asarray(alphas[s], dtype=np.float64)[:, p]
        res[j] = np.abs(P_obs[:, j] + draws_[j]["eps"] + (hyps[s]["noise"] + max(float(jitter[s]), 0.0)) * al - y).max()
        bound[j] = 64.0 * N * U * K_norms[s] * np.abs(al).max()
    return res, bound


# ---- the device algebra restated in float64 (host tests) -------------------------------------------------------------------------
def host_alphas(X, y, hyps, kernel, draws_, jitter=None):
    """alphas[s] (N x qs) as the device makes them, in float64 with LAPACK: the pseudo-responses (y - Phi w') - eps, K by the
    expansion formula with noise (+ jitter) on the diagonal."""
    from scipy.linalg import cho_factor, cho_solve
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64).ravel()
    S, q = len(hyps), len(draws_)
    out = []
    for s in range(min(S, q)):
        h = hyps[s]
        js = list(range(s, q, S))
        F = len(draws_[s]["phase"])
        Wp = np.stack([packed_weights(draws_[j]["weight"], h["amp"], F) for j in js], axis=1)
        phiw = np.cos(X @ draws_[s]["omega"].T + draws_[s]["phase"][None, :]) @ Wp
        ycols = (y[:, None] - phiw) - np.stack([draws_[j]["eps"] for j in js], axis=1)
        K = PR.device_kstar(X, X, h["lenscale_sq"], h["amp"], kernel)
        K[np.diag_indices(len(X))] = h["amp"] + h["noise"] + (0.0 if jitter is None else max(float(jitter[s]), 0.0))
        out.append(cho_solve(cho_factor(K, lower=True), ycols - h["mean"]))
    return out


def paths_host(X, Xs, hyps, kernel, draws_, alphas, wrong=None, Xs_next=None, tail=None):
    """The float64 restatement of the nomination's path arithmetic at the rows Xs: (m + K* alpha) + cos(Xs omega' + phase) W',
    column s + S p.  wrong names one way a kernel goes wrong (tests/test_ts_exact_host.py): ("slab", start, width), ("swap", s, p),
    ("layout",), ("chunk", c), ("base", ) with tail the mask of the rows in the last ragged 16-row tile, ("hql",) with Xs_next the
    neighbouring queries."""
    X, Xs = np.asarray(X, dtype=np.float64), np.asarray(Xs, dtype=np.float64)
    S, q = len(hyps), len(draws_)
    kind = wrong[0] if wrong else None
    out = np.full((len(Xs), q), np.nan)
    for s in range(min(S, q)):
        h = hyps[s]
        js = list(range(s, q, S))
        F = len(draws_[s]["phase"])
        Ks = PR.device_kstar(Xs, X, h["lenscale_sq"], h["amp"], kernel)
        if kind == "hql":
            w = 1.0 / np.asarray(h["lenscale_sq"], dtype=np.float64).ravel()
            hq, hk = 0.5 * ((Xs_next * Xs_next) @ w), 0.5 * ((X * X) @ w)
            arg = np.minimum(((Xs @ (X * w).T) - hq[:, None]) - hk[None, :], 0.0)
            sq = np.sqrt(-10.0 * arg)
            Ks = h["amp"] * np.exp(arg) if kernel == PR.SE else h["amp"] * (1.0 + sq * (1.0 + sq / 3.0)) * np.exp(-sq)
        if kind == "slab":
            Ks[:, wrong[1]:wrong[1] + wrong[2]] = 0.0
        al = np.array(alphas[s], dtype=np.float64)
        if kind == "swap" and wrong[1] == s:
            al[:, [wrong[2], wrong[2] + 1]] = al[:, [wrong[2] + 1, wrong[2]]]
        Wp = np.stack([packed_weights(draws_[j]["weight"], h["amp"], F) for j in js], axis=1)
        C = np.cos(Xs @ draws_[s]["omega"].T + draws_[s]["phase"][None, :])
        if kind == "chunk":
            C[:, 16 * wrong[1]:16 * wrong[1] + 16] = 0.0
        base = h["mean"] + Ks @ al
        if kind == "base":
            base[tail] = 0.0
        val = base + C @ Wp
        for p, j in enumerate(js):
            out[:, (p + len(js) * s) if kind == "layout" else j] = val[:, p]
    return out
