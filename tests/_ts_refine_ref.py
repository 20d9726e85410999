"""References for the refinement of Thompson nominees on their own sample paths (b7_ts_nominate_refine, b7_ts_path_grad_at;
tests/test_ts_refine_host.py, tests/test_gpu_ts_refine.py).  No GPU needed here.

  * value_grad64: a path's value and gradient in float64, the value built on _ts_ref.cov / features, with the scales the bars use;
  * value_grad_mp: the same at 50 digits (mpmath), the float64 inputs taken as exact;
  * starts_ref: the start selection as a numpy stable argsort;
  * descend: the whole descent in float64, _refine_ref.refine_run on the negated path.

  f_j(x)     = m + sum_f W[f] cos(omega[f] . x + phase[f]) + sum_i v[i] k(x, X_i)               W = sqrt(2 amp / F) weight
  df_j/dx_c  = -sum_f W[f] sin(omega[f] . x + phase[f]) omega[f][c] - w_c sum_i v[i] g_i (x_c - X_ic)
with w = 1 / lenscale_sq and g the radial factor of _refine_ref.cov64 (ARD-SE: k; Matern-5/2: (5/3) amp (1 + s) exp(-s))."""
import mpmath
import numpy as np

import _refine_ref as RR
import _ts_ref as TR

DPS = 50


def value_grad64(X, hyp, kernel, dr, v, xs, want_scale=False):
    """(val P, grad P x d[, scale_val P, scale_grad P]) of one path at the rows of xs.  dr: its draws (omega, phase, weight), v: its
    update weights.  The scales are the sums of the absolute values of the terms: |m| + sum |W| + sum |v_i k_i|, and per point the
    largest over c of sum_f |W_f sin_f omega_fc| + sum_i |v_i g_i (x_c - X_ic) w_c|."""
    X, xs = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(xs, dtype=np.float64))
    v = np.asarray(v, dtype=np.float64).ravel()
    w = 1.0 / np.asarray(hyp["lenscale_sq"], dtype=np.float64).ravel()
    F = len(dr["phase"])
    Wp = TR.packed_weights(dr["weight"], hyp["amp"], F)
    arg = xs @ dr["omega"].T + dr["phase"][None, :]
    diff = xs[:, None, :] - X[None, :, :]
    k, g = RR.cov64(np.einsum("pic,c->pi", diff * diff, w), hyp["amp"], kernel)
    val = hyp["mean"] + TR.features(xs, dr["omega"], dr["phase"], hyp["amp"]) @ dr["weight"] + TR.cov(xs, X, hyp["lenscale_sq"], hyp["amp"], kernel) @ v
    sw = np.sin(arg) * Wp[None, :]
    grad = -(sw @ dr["omega"]) - np.einsum("pi,pic->pc", g * v[None, :], diff) * w[None, :]
    if not want_scale:
        return val, grad
    sv = abs(hyp["mean"]) + np.abs(Wp).sum() + np.abs(k) @ np.abs(v)
    sg = (np.abs(sw) @ np.abs(dr["omega"]) + np.einsum("pi,pic->pc", np.abs(g * v[None, :]), np.abs(diff)) * w[None, :]).max(axis=1)
    return val, grad, sv, sg


def value_grad_mp(X, hyp, kernel, dr, v, xs):
    """(val P, grad P x d) as object arrays of mpf at DPS digits; W is the double sqrt(2 amp / F) weight, as the library packs it."""
    X, xs = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(xs, dtype=np.float64))
    N, d = X.shape
    F = len(dr["phase"])
    Wp = TR.packed_weights(dr["weight"], hyp["amp"], F)
    with mpmath.workdps(DPS):
        mp = lambda a: [mpmath.mpf(float(t)) for t in np.ravel(a)]
        ls, amp, mean = mp(hyp["lenscale_sq"]), mpmath.mpf(float(hyp["amp"])), mpmath.mpf(float(hyp["mean"]))
        om, ph, W, vv = [mp(r) for r in dr["omega"]], mp(dr["phase"]), mp(Wp), mp(v)
        Xm = [mp(r) for r in X]
        vals, grads = [], []
        for row in xs:
            x = mp(row)
            val, grad = mean, [mpmath.mpf(0)] * d
            for f in range(F):
                a = sum(om[f][c] * x[c] for c in range(d)) + ph[f]
                val = val + W[f] * mpmath.cos(a)
                ws = W[f] * mpmath.sin(a)
                grad = [grad[c] - ws * om[f][c] for c in range(d)]
            for i in range(N):
                D = sum((x[c] - Xm[i][c]) ** 2 / ls[c] for c in range(d))
                if kernel == "ardse":
                    k = amp * mpmath.exp(-D / 2)
                    g = k
                else:
                    s = mpmath.sqrt(5 * D)
                    e = mpmath.exp(-s)
                    k, g = amp * (1 + s + s * s / 3) * e, amp * 5 * (1 + s) * e / 3
                val = val + vv[i] * k
                grad = [grad[c] - vv[i] * g * (x[c] - Xm[i][c]) / ls[c] for c in range(d)]
            vals.append(val)
            grads.append(grad)
        return np.array(vals, dtype=object), np.array(grads, dtype=object)


def starts_ref(paths, nominees, P):
    """Path j's P starts as 0-based rows (q x P; -1 where no row is left): its nominee, then the P - 1 rows of lowest f_j among the
    rows that are none of the q nominees, ascending by (value, row) -- a stable argsort --, a NaN never chosen."""
    paths = np.asarray(paths, dtype=np.float64)
    q = paths.shape[1]
    out = np.full((q, P), -1, dtype=np.int64)
    barred = np.zeros(len(paths), dtype=bool)
    barred[np.asarray(nominees, dtype=np.int64)] = True
    for j in range(q):
        out[j, 0] = nominees[j]
        order = np.argsort(paths[:, j], kind="stable")
        order = order[~np.isnan(paths[order, j]) & ~barred[order]][:P - 1]
        out[j, 1:1 + len(order)] = order
    return out


def descend(value_grad, starts_x, iters, eta0, lo, hi):
    """_refine_ref.refine_run on -f: value_grad(xs) -> (f, df).  The result's val / val0 are the PATH's values (lower is better)."""
    def neg(xs):
        f, g = value_grad(xs)
        return -np.asarray(f), -np.asarray(g)
    out = RR.refine_run(neg, starts_x, iters, eta0, lo, hi)
    out["val"], out["val0"] = -out["val"], -out["val0"]
    return out
