"""References for the off-grid refinement (b7_eval_nominate_refine, b7_gp_grad_at, b7_score_grad_compute; tests/test_refine_host.py,
tests/test_gpu_refine.py).  No GPU needed here.

  * the posterior and its gradient in float64 numpy, in the device's L^-1 form (fit64, post_grad64);
  * the score's value and gradient per kind and the marginal over the S samples (score_value_grad64): EI / CB values through the
    oracle's arithmetic (oracle/cport.py), LogEI's through tests/_logei_ref.logei_np;
  * one ladder step as pure functions (ladder_candidates, ladder_decide) and the whole ascent on top of them (refine_run);
  * the truth: the same quantities at 50 digits (mpmath) for N <= 64, in numpy longdouble above, by one hand-written Cholesky
    (post_grad_truth), and the score's value and gradient at 50 digits (score_value_grad_mp).

With D_i = sum_c (x_c - X_ic)^2 / l2_c, k_i = k(x, X_i), dk_i/dx_c = -g_i (x_c - X_ic) / l2_c (ARD-SE: g = k; Matern-5/2: g = (5/3) amp (1 + s)
exp(-s), s = sqrt(5 D)), V = inv(L) k*, W = inv(L)' V:   mu = m + k* . alpha,  var = amp - |V|^2,  dmu_c = sum_i alpha_i dk_i/dx_c,
dvar_c = -2 sum_i W_i dk_i/dx_c,  dsigma = dvar / (2 sigma)."""
import math

import mpmath
import numpy as np
from scipy import special
from scipy.linalg import solve_triangular

import _logei_ref as LR

DPS = 50
EPS = 2.0 ** -52
NOT_RUN, FLAT, CONVERGED, MOVED = 1, 2, 4, 8
ETA_FLOOR = 2.0 ** -40


# ---- float64: the device's algebra ------------------------------------------------------------------------------------------------
def cov64(D, amp, kernel):
    """(k, g) from the scaled squared distances D."""
    if kernel == "ardse":
        k = amp * np.exp(-0.5 * D)
        return k, k
    s = np.sqrt(5.0 * D)
    e = np.exp(-s)
    return amp * (1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * amp * (1.0 + s) * e


def fit64(X, y, hyp, kernel="ardse", jitter=0.0):
    X = np.asarray(X, dtype=np.float64)
    w = 1.0 / np.asarray(hyp["lenscale_sq"], dtype=np.float64)
    D = np.zeros((len(X), len(X)))
    for c in range(X.shape[1]):                 # (no N x N x d intermediate)
        D += (X[:, None, c] - X[None, :, c]) ** 2 * w[c]
    K, _ = cov64(D, hyp["amp"], kernel)
    K[np.diag_indices(len(X))] += hyp["noise"] + jitter
    L = np.linalg.cholesky(K)
    Linv = solve_triangular(L, np.eye(len(X)), lower=True)
    r = np.asarray(y, dtype=np.float64).ravel() - hyp["mean"]
    return {"X": X, "w": w, "amp": hyp["amp"], "mean": hyp["mean"], "Linv": Linv, "alpha": Linv.T @ (Linv @ r), "kernel": kernel}


def post_grad64(f, xs):
    """mu[P], var[P], dmu[P][d], dvar[P][d] at the rows of xs."""
    xs = np.atleast_2d(np.asarray(xs, dtype=np.float64))
    diff = xs[:, None, :] - f["X"][None, :, :]
    k, g = cov64(np.einsum("pic,c->pi", diff * diff, f["w"]), f["amp"], f["kernel"])
    V = f["Linv"] @ k.T
    W = f["Linv"].T @ V
    dk = -(g[:, :, None] * diff) * f["w"]
    return (f["mean"] + k @ f["alpha"], f["amp"] - np.einsum("ip,ip->p", V, V), np.einsum("i,pic->pc", f["alpha"], dk),
            -2.0 * np.einsum("ip,pic->pc", W, dk))


def _erf_as(x):
    """A&S 7.1.26 as the scores evaluate it (utils/math.lua:261-288)."""
    t = 1.0 / (np.abs(x) * 0.3275911 + 1.0)
    r = ((((1.061405429 * t + -1.453152027) * t + 1.421413741) * t + -0.284496736) * t + 0.254829592) * t
    return (1.0 - r * np.exp(-(x * x))) * np.where(x >= 0.0, 1.0, -1.0)


def score_coef64(kind, mu, var, spec):
    """(dv/dmu, dv/dsigma) of one sample's score at every row."""
    sigma = np.sqrt(var)
    if kind == "cb":
        sg = 1.0 if spec.get("sign", -1.0) > 0.0 else -1.0
        kap = spec.get("tradeoff", 1.0)
        return np.full_like(mu, sg), np.full_like(mu, sg * (kap if spec.get("upper") else -kap))
    z = ((spec["fmin"] - mu) - spec.get("tradeoff", 0.0)) / sigma
    if kind == "ei":
        return -(_erf_as(z * 0.70710678118654746) + 1.0) * 0.5, np.exp(-0.5 * z * z) * 0.3989422804014327
    with np.errstate(all="ignore"):
        R = LR.SQRT_PI_2 * special.erfcx(-z * LR.SQRT1_2)          # Phi / phi
        ph = np.where(z < 0.0, 1.0 / (1.0 + z * R), (1.0 / R) / (z + 1.0 / R))
        Ph = np.where(z < 0.0, R * ph, 1.0 / (z + 1.0 / R))
    return -Ph / sigma, ph / sigma


def score_value64(kind, mu, var, spec):
    """One sample's score at every row, in the arithmetic the grid's score has."""
    if kind == "logei":
        return LR.logei_np(mu, var, spec["fmin"], spec.get("tradeoff", 0.0))
    from oracle import cport
    mu, var = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
    if kind == "ei":
        return cport.ei(mu, var, [spec["fmin"]], spec.get("tradeoff", 0.0))
    return cport.cb(mu, var, spec.get("tradeoff", 1.0), bool(spec.get("upper")), spec.get("sign", -1.0))


def score_value_grad64(kind, mu, var, dmu, dvar, spec):
    """The marginal value [P] and gradient [P][d] from S samples' mu / var [S][P] and gradients [S][P][d]."""
    mu, var, dmu, dvar = (np.asarray(a, dtype=np.float64) for a in (mu, var, dmu, dvar))
    S = mu.shape[0]
    vals, grads = [], []
    for s in range(S):
        cm, cs = score_coef64(kind, mu[s], var[s], spec)
        with np.errstate(all="ignore"):
            vals.append(score_value64(kind, mu[s], var[s], spec))
            grads.append(cm[:, None] * dmu[s] + cs[:, None] * (dvar[s] / (2.0 * np.sqrt(var[s]))[:, None]))
    if kind == "logei":
        a = np.full(mu.shape[1], -np.inf)
        for s in range(S):
            a = LR.logaddexp_np(a, vals[s])
        with np.errstate(all="ignore"):
            G = sum(np.exp(vals[s] - a)[:, None] * grads[s] for s in range(S))
        return a + (-math.log(float(S))), G
    a = np.zeros(mu.shape[1])
    for s in range(S):
        a = a + vals[s]
    return a / float(S), sum(grads) / float(S)


def value_grad64(fits, kind, spec, xs):
    """The marginal acquisition and its gradient at the rows of xs under the S fits."""
    parts = [post_grad64(f, xs) for f in fits]
    return score_value_grad64(kind, *(np.stack([p[i] for p in parts]) for i in range(4)), spec)


# ---- the ladder ------------------------------------------------------------------------------------------------------------------
def ladder_candidates(x, g, eta, lo, hi):
    """The four rungs' points (4 x d), or None when the start is flat (max |g (hi - lo)| zero or not finite)."""
    b = hi - lo
    gt = g * b
    with np.errstate(all="ignore"):
        m = np.max(np.abs(gt))
    if not (m > 0.0 and np.isfinite(m)):
        return None
    r = gt / m
    return np.stack([np.minimum(np.maximum(x + ((eta * 4.0 ** -k) * r) * b, lo), hi) for k in range(4)])


def ladder_decide(v, eta, cand_vals):
    """(rung taken or -1, new value, new eta, converged) from a start's value, its step and the four rungs' values: the highest
    value wins, the lowest rung on ties, never a NaN; it must be strictly above v; eta <- min(1, 4 t_k) or eta / 256."""
    kb, bv = -1, None
    for k in range(4):
        c = cand_vals[k]
        if c == c and (kb < 0 or c > bv):
            kb, bv = k, c
    if kb >= 0 and bv > v:
        eta_new = min(1.0, 4.0 * (eta * 4.0 ** -kb))
        return kb, bv, eta_new, eta_new < ETA_FLOOR
    eta_new = eta / 256.0
    return -1, v, eta_new, eta_new < ETA_FLOOR


def refine_run(value_grad, starts, iters, eta0, lo, hi, grid_scores=None):
    """The whole ascent in float64: value_grad(xs) -> (values, gradients).  -> dict(x P x d, val P, status P, val0 P, winner)."""
    starts = np.asarray(starts, dtype=np.float64)
    P, d = starts.shape
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,))
    x = starts.copy()
    v, g = value_grad(x)
    v, g = np.array(v), np.array(g)
    status = np.where(np.isfinite(v), 0, NOT_RUN)
    if grid_scores is not None:
        status = np.where(np.isnan(np.asarray(grid_scores)), NOT_RUN, status)
    eta, val0 = np.full(P, float(eta0)), v.copy()
    for _ in range(iters):
        for p in range(P):
            if status[p] & (NOT_RUN | CONVERGED):
                continue
            cand = ladder_candidates(x[p], g[p], eta[p], lo, hi)
            if cand is None:
                status[p] |= FLAT
                continue
            cv, cg = value_grad(cand)
            k, v[p], eta[p], conv = ladder_decide(v[p], eta[p], cv)
            if k >= 0:
                x[p], g[p] = cand[k], cg[k]
                status[p] |= MOVED
            if conv:
                status[p] |= CONVERGED
    win = 0
    if np.any(status & MOVED):
        ok = [p for p in range(P) if not (status[p] & NOT_RUN) and np.isfinite(v[p])]
        if ok:
            win = max(ok, key=lambda p: (v[p], -p))
    return {"x": x, "val": v, "status": status, "val0": val0, "winner": win}


def th_top(acc, P):
    """TH's max applied P times, the earlier winners left out: the first NaN wins, else the largest value, ties to the lowest row."""
    acc = np.asarray(acc, dtype=np.float64)
    left, out = np.ones(acc.size, dtype=bool), []
    for _ in range(P):
        idx = np.flatnonzero(left)
        a = acc[idx]
        nan = np.flatnonzero(np.isnan(a))
        j = idx[nan[0]] if nan.size else idx[int(np.argmax(a))]
        out.append(int(j))
        left[j] = False
    return out


# ---- the truth --------------------------------------------------------------------------------------------------------------------
def _backend(N):
    """Arithmetic of the truth: mpmath objects (call inside workdps) for N <= 64, numpy longdouble above."""
    if N <= 64:
        conv = lambda a: np.array([mpmath.mpf(float(v)) for v in np.ravel(a)], dtype=object).reshape(np.shape(a))
        return conv, np.frompyfunc(mpmath.exp, 1, 1), np.frompyfunc(mpmath.sqrt, 1, 1)
    return (lambda a: np.asarray(a, dtype=np.longdouble)), np.exp, np.sqrt


def _chol(A, sqrt):
    n = A.shape[0]
    L = A.copy()
    for j in range(n):
        L[j, j] = sqrt(L[j, j] - (L[j, :j] @ L[j, :j] if j else 0))
        if j + 1 < n:
            L[j + 1:, j] = (L[j + 1:, j] - (L[j + 1:, :j] @ L[j, :j] if j else 0)) / L[j, j]
        L[j, j + 1:] = L[j, j + 1:] * 0
    return L


def _fwd(L, B):
    X = B.copy()
    for i in range(L.shape[0]):
        X[i] = (B[i] - (L[i, :i] @ X[:i] if i else 0)) / L[i, i]
    return X


def _bwd(L, B):
    X = B.copy()
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        X[i] = (B[i] - (L[i + 1:, i] @ X[i + 1:] if i + 1 < n else 0)) / L[i, i]
    return X


def _cov_t(D, amp, kernel, exp, sqrt):
    if kernel == "ardse":
        k = amp * exp(-D / 2)
        return k, k
    s = sqrt(5 * D)
    e = exp(-s)
    return amp * (1 + s + s * s / 3) * e, amp * 5 * (1 + s) * e / 3


def post_grad_truth(X, y, hyp, xs, kernel="ardse", jitter=0.0):
    """(mu, var, dmu, dvar) at the rows of xs (at most a handful) as arrays of the truth's arithmetic."""
    X, xs = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(xs, dtype=np.float64))
    N = X.shape[0]
    with mpmath.workdps(DPS):
        conv, exp, sqrt = _backend(N)
        Xt, xt, ls = conv(X), conv(xs), conv(np.asarray(hyp["lenscale_sq"], dtype=np.float64))
        amp, mean = conv([hyp["amp"]])[0], conv([hyp["mean"]])[0]
        D = 0
        for c in range(X.shape[1]):             # (no N x N x d intermediate)
            dc = Xt[:, None, c] - Xt[None, :, c]
            D = D + dc * dc / ls[c]
        K, _ = _cov_t(D, amp, kernel, exp, sqrt)
        for i in range(N):
            K[i, i] = K[i, i] + conv([hyp["noise"]])[0] + conv([jitter])[0]
        L = _chol(K, sqrt)
        r = conv(np.asarray(y, dtype=np.float64).ravel()) - mean
        alpha = _bwd(L, _fwd(L, r.reshape(N, 1))).reshape(N)
        diff = xt[:, None, :] - Xt[None, :, :]
        k, g = _cov_t((diff * diff / ls).sum(-1), amp, kernel, exp, sqrt)       # P x N
        V = _fwd(L, k.T.copy())
        W = _bwd(L, V)
        dk = -(g[:, :, None] * diff) / ls                                     # P x N x d
        mu = mean + k @ alpha
        var = amp - (V * V).sum(0)
        dmu = (alpha[None, :, None] * dk).sum(1)
        dvar = -2 * (W.T[:, :, None] * dk).sum(1)
        return mu, var, dmu, dvar


def err_vs_truth(got, truth):
    """max |got - truth| with the difference taken in the truth's arithmetic."""
    with mpmath.workdps(DPS):
        truth = np.asarray(truth)
        if truth.dtype == object:
            g = np.array([mpmath.mpf(float(v)) for v in np.ravel(got)], dtype=object)
            return float(max(abs(a - b) for a, b in zip(g, truth.ravel())))
        return float(np.max(np.abs(np.asarray(got, dtype=np.longdouble).ravel() - truth.ravel())))


def truth_to_float(t):
    with mpmath.workdps(DPS):
        return np.array([float(v) for v in np.ravel(t)], dtype=np.float64).reshape(np.shape(t))


# ---- the score at 50 digits -----------------------------------------------------------------------------------------------------
def _erf_as_mp(x):
    t = 1 / (abs(x) * mpmath.mpf(0.3275911) + 1)
    c = [mpmath.mpf(v) for v in (1.061405429, -1.453152027, 1.421413741, -0.284496736, 0.254829592)]
    r = ((((c[0] * t + c[1]) * t + c[2]) * t + c[3]) * t + c[4]) * t
    return (1 - r * mpmath.exp(-x * x)) * (1 if x >= 0 else -1)


def _to_mp(v):
    """A float, a longdouble (split exactly into two doubles) or an mpf as an mpf."""
    if isinstance(v, mpmath.mpf):
        return v
    if isinstance(v, np.longdouble):
        hi = float(v)
        return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))
    return mpmath.mpf(float(v))


def score_value_grad_mp(kind, mu, var, dmu, dvar, spec):
    """The marginal value and gradient of score_value_grad64 at 50 digits on the exact values of the inputs (floats, or the truth's
    own mpf / longdouble arrays).  EI is the score's own definition -- A&S's Phi (its constants as the doubles they are), the exact
    phi --, LogEI the exact log EI."""
    mu, var, dmu, dvar = (np.asarray(a) for a in (mu, var, dmu, dvar))
    S, P, d = dmu.shape
    with mpmath.workdps(DPS):
        mpf = _to_mp
        vals, grads = [], []
        for j in range(P):
            vs, gs = [], []
            for s in range(S):
                m, sig = mpf(mu[s, j]), mpmath.sqrt(mpf(var[s, j]))
                if kind == "cb":
                    sg = 1 if spec.get("sign", -1.0) > 0.0 else -1
                    kap = mpf(spec.get("tradeoff", 1.0)) * (1 if spec.get("upper") else -1)
                    v, cm, cs = sg * (m + kap * sig), mpmath.mpf(sg), sg * kap
                else:
                    z = (mpf(spec["fmin"]) - m - mpf(spec.get("tradeoff", 0.0))) / sig
                    pdf = mpmath.exp(-z * z / 2) / mpmath.sqrt(2 * mpmath.pi)
                    if kind == "ei":
                        cdf = (_erf_as_mp(z * mpf(0.70710678118654746)) + 1) / 2
                        pdf_s = mpmath.exp(-z * z / 2) * mpf(0.3989422804014327)
                        v = (mpf(spec["fmin"]) - m - mpf(spec.get("tradeoff", 0.0))) * cdf + sig * pdf_s
                        v, cm, cs = max(v, mpmath.mpf(0)), -cdf, pdf_s
                    else:
                        cdf = mpmath.erfc(-z / mpmath.sqrt(2)) / 2
                        h = pdf + z * cdf
                        v, cm, cs = mpmath.log(sig * h), -(cdf / h) / sig, (pdf / h) / sig
                vs.append(v)
                gs.append([cm * mpf(dmu[s, j, c]) + cs * mpf(dvar[s, j, c]) / (2 * sig) for c in range(d)])
            if kind == "logei":
                top = max(vs)
                wts = [mpmath.exp(v - top) for v in vs]
                tot = sum(wts)
                vals.append(top + mpmath.log(tot / S))
                grads.append([sum(wts[s] * gs[s][c] for s in range(S)) / tot for c in range(d)])
            else:
                vals.append(sum(vs) / S)
                grads.append([sum(gs[s][c] for s in range(S)) / S for c in range(d)])
        return np.array(vals, dtype=object), np.array(grads, dtype=object)
