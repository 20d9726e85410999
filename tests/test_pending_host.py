"""The references of tests/_pending_ref.py against each other, without a GPU: 50 digits against LAPACK against the long-double
restatements and their derived bars; the recovery of a fantasy factor from draws whose normals are off by 4 ulp; the jitter cases'
cost in schedule steps; the append chain's restatement and its refusal rule at the named corners."""
import math

import mpmath
import numpy as np
import pytest
from scipy.linalg import lapack, solve_triangular

import _exact as E
import _pending_ref as R


def _small_case(N, P, seed):
    rng = np.random.default_rng(seed)
    d = 1 if N == 2 else 2
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.05 * rng.normal(size=N)
    Y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    return X, Y, rng.random((P, d))


@pytest.mark.parametrize("N,P", [(2, 1), (2, 3), (16, 1), (16, 3)])
def test_cov_truth_against_gp_truth_lapack_and_the_long_double_restatement(N, P):
    """gp_cov_truth's diagonal and mean are _exact.gp_truth's; LAPACK (lapack_cov) and the long-double restatement on LAPACK's own
    inverse factor (cov_ref_bar, mean_ref_bar) are within gp_bar of LAPACK's error of the 50 digits, at the three hypers of A.3."""
    X, Y, Xp = _small_case(N, P, seed=N + P)
    for h in R.box_hyps(X, Y, seed=N):
        K = R.host_K(X, h)
        jit = 0.0
        for jit in [0.0] + E.jitter_schedule(float(np.linalg.norm(K))):
            if R.lapack_cov(X, Y, h, Xp, jitter=jit) is not None:
                break
        mu_t, cov_t = R.gp_cov_truth(X, Y, h, Xp, jitter=jit)
        t = E.gp_truth(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xp, jitter=jit)
        assert all(abs(a - b) <= mpmath.mpf(10) ** -40 * (1 + abs(b)) for a, b in zip(mu_t, t.mu))
        assert all(abs(cov_t[p, p] - t.var[p]) <= mpmath.mpf(10) ** -40 * h["amp"] for p in range(P))
        orcs = [R.lapack_cov(X, Y, h, Xp, jitter=jit, kscale=ks) for ks in (1.0, 1.0 - E.EPS, 1.0 + E.EPS)]
        orcs = [o for o in orcs if o is not None]
        e_mu = max(E.err_vs(o[0], mu_t) for o in orcs)
        e_cov = max(E.err_vs(o[1], R.mp_flat(cov_t)) for o in orcs)
        Kj = K.copy()
        Kj[np.diag_indices(N)] += jit
        L, Li = R.lapack_factors(Kj)
        from oracle import gp
        Kp, Kpp = gp.ardse(Xp, X, h["lenscale_sq"], h["amp"]), gp.ardse(Xp, None, h["lenscale_sq"], h["amp"])
        ref, bar = R.cov_ref_bar(Kp, Kpp, Li, R.npad(N))
        assert E.err_vs(ref.astype(np.float64), R.mp_flat(cov_t)) <= E.gp_bar(e_cov, h["amp"])
        r = Y - h["mean"]
        a_ref, _ = R.alpha_ref_bar(Li, r, R.npad(N))
        m_ref, _ = R.mean_ref_bar(Kp, a_ref, h["mean"], R.npad(N))
        assert E.err_vs(m_ref[:, 0].astype(np.float64), mu_t) <= E.gp_bar(e_mu, math.sqrt(h["amp"]) + abs(h["mean"]))


@pytest.mark.parametrize("N,c,d", [(1, 2, 1), (65, 65, 6), (257, 3, 6)])
def test_derived_bars_hold_for_float64_products_and_catch_a_dropped_term(N, c, d):
    """float64 numpy's Linv' (Linv r) and mean + K* alpha are inside the derived bars of their long-double references (worst ratio
    printed); dropping the last term of either product, or its last 4-wide slice, is not."""
    X, Yc = R.multi_data(N, d, c, seed=N)
    h = R.grid_hyp(d)
    L, Li = R.lapack_factors(R.host_K(X, h))
    r = Yc - h["mean"]
    ref, bar = R.alpha_ref_bar(Li, r, R.npad(N))
    got = Li.T @ (Li @ r)
    ratio = np.abs(got - ref).astype(np.float64) / bar
    assert ratio.max() <= 1.0
    Xs = R.grid_points(129, d, seed=5)
    from oracle import gp
    Ks = gp.ardse(Xs, X, h["lenscale_sq"], h["amp"])
    mref, mbar = R.mean_ref_bar(Ks, got, h["mean"], R.npad(N))
    mu = h["mean"] + Ks @ got
    assert (np.abs(mu - mref).astype(np.float64) / mbar).max() <= 1.0
    print("N %d c %d: alpha %.3f of its bar, mean %.3f" % (N, c, ratio.max(), (np.abs(mu - mref).astype(np.float64) / mbar).max()))
    if N >= 65:
        lo = N - 4
        wrong = h["mean"] + Ks[:, :lo] @ got[:lo]
        assert (np.abs(wrong - mref).astype(np.float64) / mbar).max() > 1.0
        wrong_a = Li[:lo].T @ (Li[:lo] @ r)
        assert (np.abs(wrong_a - ref).astype(np.float64) / bar).max() > 1.0


def _synthetic(P, n, seed, jitter=0.0):
    rng = np.random.default_rng(P)
    A = rng.normal(size=(P, P + 3))
    S = A @ A.T / (P + 3)
    Lp = np.linalg.cholesky(S + jitter * np.eye(P))
    mu = rng.normal(size=P)
    Z = R.fantasy_normals(seed, P, n)
    Zp = Z * (1.0 + R.DRAW_ULP * E.EPS * rng.choice([-1.0, 1.0], size=Z.shape))     # every normal off by 4 ulp
    return S, Lp, mu, Z, mu[:, None] + Lp @ Zp


@pytest.mark.parametrize("P", [2, 8, 64])
def test_factor_recovery_from_draws_with_normals_off_by_four_ulp(P):
    """recover_factor on synthetic (Lp, Z) pairs, n = 4 P, a seed >= 2^63: cond(Z) < 4, the strict upper triangle and L_est - Lp
    inside Delta, L_est L_est' = S inside the bar of C.2, a jitter recovered to 1e-3; a factor with a filled upper triangle and
    the layout s P + k are far outside."""
    n, seed = 4 * P, 2 ** 63 + 12345
    S, Lp, mu, Z, Y = _synthetic(P, n, seed)
    L_est, delta, cond = R.recover_factor(Y, mu, Z)
    assert cond < 4.0
    up = float(np.linalg.norm(np.triu(L_est, 1)))
    err = float(np.linalg.norm(L_est - Lp))
    print("P %d: cond(Z) %.2f, upper %.3g, error %.3g, Delta %.3g, ||S|| %.3g" % (P, cond, up, err, delta, np.linalg.norm(S)))
    assert up <= delta and err <= delta
    assert np.linalg.norm(L_est @ L_est.T - S) <= 8 * E.EPS * np.linalg.norm(S) + 2 * np.linalg.norm(L_est) * delta
    # a jittered factor: j is the mean diagonal of L_est L_est' - S
    j = R.fantasy_schedule()[3]
    S, Lp, mu, Z, Y = _synthetic(P, n, seed, jitter=j)
    L_est, delta, _ = R.recover_factor(Y, mu, Z)
    j_est = float(np.mean(np.diag(L_est @ L_est.T - S)))
    assert R.match_schedule(j_est) == 3
    assert np.linalg.norm(L_est @ L_est.T - (S + j * np.eye(P))) <= 8 * E.EPS * np.linalg.norm(S) + 2 * np.linalg.norm(L_est) * delta
    # the breaks: an upper triangle that is read, and the transposed counter layout
    full = Lp + np.triu(Lp.T, 1) * 1e-9
    Lw, dw, _ = R.recover_factor(mu[:, None] + full @ Z, mu, Z)
    assert np.linalg.norm(np.triu(Lw, 1)) > dw
    Zt = R.T.counter_normal(np.uint64(seed), np.arange(n, dtype=np.uint64)[None, :] * np.uint64(P) + np.arange(P, dtype=np.uint64)[:, None])
    Lw, dw, _ = R.recover_factor(mu[:, None] + Lp @ Zt, mu, Z)
    assert np.linalg.norm(np.triu(Lw, 1)) > dw


def test_fantasy_layout_depends_on_n():
    """z(k, s) = counter_normal(seed, k n + s): n = 8 and n = 16 share row 0 and differ in every later row."""
    a, b = R.fantasy_normals(7, 3, 8), R.fantasy_normals(7, 3, 16)
    assert np.array_equal(a[0], b[0, :8]) and not np.array_equal(a[1:], b[1:, :8])
    assert np.array_equal(a[1], b[0, 8:])


def test_jitter_cases_cost_lapack_fewer_than_twenty_schedule_steps():
    for name, X, Y, h, Xp in R.jitter_cases():
        assert R.lapack_factors(R.host_K(X, h)) is not None, "the fit itself must not need jitter"
        _, S = R.lapack_cov(X, Y, h, Xp)
        S = np.tril(S) + np.tril(S, -1).T
        steps = 0
        sched = R.fantasy_schedule()
        while True:
            Sj = S + (sched[steps - 1] if steps else 0.0) * np.eye(len(S))
            if lapack.dpotrf(Sj, lower=1, clean=1)[1] == 0:
                break
            steps += 1
        print("%s: LAPACK needs %d schedule steps, min pivot %.3g" % (name, steps, E.min_pivot(S)))
        assert steps < 20
        assert abs(E.min_pivot(S)) <= len(S) * E.EPS * np.linalg.norm(S) or steps > 0


chain_hypers = R.chain_hypers


@pytest.mark.parametrize("n0,N,d", R.CHAINS)
def test_restated_append_chain_against_lapack(n0, N, d):
    """The float64 restatement of the chain n0 -> N at the eight covariance corners and the interior point: where it runs to the
    end its factors are finite and its backward errors are printed beside LAPACK's; where it refuses a step, l2 <= tol there and
    LAPACK's smallest pivot on the extended matrix is within n eps ||K|| of zero or the matrix has cond > 1e10."""
    X, Y = E.grid_data(N, d, seed=N)
    done = 0
    for i, h in enumerate(chain_hypers(X, Y)):
        K = R.host_K(X, h)
        ch = R.append_chain(K, n0)
        if ch is None:
            print("(%d -> %d, %d) hyper %d: dpotrf fails at n0" % (n0, N, d, i))
            continue
        L, Li, n_end, steps = ch
        assert np.isfinite(L).all() and np.isfinite(Li).all()
        if n_end < N:
            n, ok, l2, tol = steps[-1]
            Kn = K[:n + 1, :n + 1]
            assert not ok and not l2 > tol
            assert np.linalg.cond(Kn) > 1e10 or abs(E.min_pivot(Kn)) <= (n + 1) * E.EPS * np.linalg.norm(Kn)
            print("(%d -> %d, %d) hyper %d: refused at n = %d, l2 %.3g tol %.3g cond %.2g" % (n0, N, d, i, n, l2, tol, np.linalg.cond(Kn)))
            continue
        yard, rs, la = R.chain_yardstick(K, n0)
        assert rs is not None
        if la is not None:
            print("(%d -> %d, %d) hyper %d: factor %.3g (LAPACK %.3g, x%.2f), inverse %.3g (LAPACK %.3g, x%.2f)"
                  % (n0, N, d, i, rs[0], la[0], rs[0] / la[0], rs[1], la[1], rs[1] / la[1]))
        done += 1
    assert done >= 5, "the restated chain must reach the end at the well-conditioned hypers"


def test_refusal_rule_at_the_named_corners():
    """(N, d) = (128, 1) from n0 = 8: the restatement refuses at corners 2 and 3 (large lenscale_sq, low noise), before the end, and
    accepts every step at the interior point; an exact duplicate of an observation under noise 0 is refused."""
    X, Y = E.grid_data(128, 1, seed=128)
    hyps = chain_hypers(X, Y)
    for i in (2, 3):
        ch = R.append_chain(R.host_K(X, hyps[i]), 8)
        assert ch is not None and ch[2] < 128, (i, ch and ch[2])
        n, ok, l2, tol = ch[3][-1]
        print("corner %d: refused at n = %d (l2 %.3g, tol %.3g)" % (i, n, l2, tol))
        assert abs(l2) <= 2 * tol or l2 < 0
    assert R.append_chain(R.host_K(X, hyps[8]), 8)[2] == 128
    X, Y = E.grid_data(40, 2, seed=40)
    h = dict(R.grid_hyp(2, j=-2), noise=0.0)
    X[39] = X[5]
    ch = R.append_chain(R.host_K(X, h), 39)
    assert ch[2] == 39 and not ch[3][-1][1]


@pytest.mark.parametrize("noise", [0.0, 1e-8])
def test_near_duplicates_are_accepted_cleanly_or_refused(noise):
    """A row at distance 2^-k (k in 10, 20, 26, 30) from an observation: the restated step either refuses or yields a finite row
    whose factors meet 4 x LAPACK's backward errors + K_GAP."""
    X0, Y = E.grid_data(41, 2, seed=41)
    h = dict(R.grid_hyp(2, j=-2), noise=noise)
    for k in (10, 20, 26, 30):
        X = X0.copy()
        X[40] = X[5]
        X[40, 0] += 2.0 ** -k
        K = R.host_K(X, h)
        ch = R.append_chain(K, 40)
        if ch is None:
            continue
        L, Li, n_end, steps = ch
        print("noise %g k %d: %s, l2 %.3g tol %.3g" % (noise, k, "accepted" if n_end == 41 else "refused", steps[-1][2], steps[-1][3]))
        if n_end == 41:
            assert np.isfinite(Li).all()
            la = R.lapack_factors(K)
            if la is not None:
                g, o = E.backward_errors(K, L, Li), E.backward_errors(K, *la)
                assert g[0] <= 4 * o[0] + R.K_GAP and g[1] <= 4 * o[1], (g, o)


def test_long_double_refit_against_50_digits():
    """D.2's truth (ld_cholesky, ld_solve_lower, ld_posterior on the host's K) against 50 digits on that same K at N = 24, d = 6,
    the interior hyper, with LAPACK's error on it beside."""
    from oracle import gp
    N, d = 24, 6
    X, Y = E.grid_data(N, d, seed=N)
    h = R.interior_hyp(d)
    Xs = R.grid_points(9, d, seed=2)
    K, Ks = R.host_K(X, h), gp.ardse(Xs, X, h["lenscale_sq"], h["amp"])
    L = R.ld_cholesky(K)
    res = np.tril(L @ L.T - K.astype(np.longdouble))          # the factor reads the lower triangle (the host's K is symmetric to 1 ulp)
    assert float(np.max(np.abs(res.astype(np.float64)))) <= 2.0 ** -60 * N * np.abs(K).max()
    B = np.random.default_rng(0).normal(size=(N, 3))
    assert float(np.max(np.abs((L @ R.ld_solve_lower(L, B) - B).astype(np.float64)))) <= 2.0 ** -60 * N * np.linalg.cond(K)
    # 50 digits on the SAME float64 K and K* (E.gp_truth would form its own K, exactly: the difference would measure the K entries)
    mu, var = R.ld_posterior(K, Ks, Y - h["mean"], h["mean"], h["amp"])
    with mpmath.workdps(50):
        Km = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(i + 1):
                Km[i, j] = Km[j, i] = mpmath.mpf(float(K[i, j]))
        Lm = mpmath.cholesky(Km)
        tm = E._fwd(Lm, mpmath.matrix([mpmath.mpf(float(v)) - mpmath.mpf(h["mean"]) for v in Y[:, 0]]))
        mu_t, var_t = [], []
        for row in Ks:
            v = E._fwd(Lm, mpmath.matrix([mpmath.mpf(float(x)) for x in row]))
            mu_t.append(mpmath.mpf(h["mean"]) + mpmath.fsum(v[i] * tm[i] for i in range(N)))
            var_t.append(mpmath.mpf(h["amp"]) - mpmath.fsum(v[i] ** 2 for i in range(N)))
    Ll, _ = R.lapack_factors(np.tril(K) + np.tril(K, -1).T)
    V = solve_triangular(Ll, Ks.T, lower=True)
    o_mu = E.err_vs(h["mean"] + V.T @ solve_triangular(Ll, Y[:, 0] - h["mean"], lower=True), mu_t)
    o_var = E.err_vs(h["amp"] - np.einsum("ij,ij->j", V, V), var_t)
    e_mu, e_var = E.err_vs(mu[:, 0].astype(np.float64), mu_t), E.err_vs(var.astype(np.float64), var_t)
    print("long double refit: mean %.3g (LAPACK %.3g), variance %.3g (LAPACK %.3g)" % (e_mu, o_mu, e_var, o_var))
    # long double carries 11 more bits than LAPACK's float64; rounded to float64 for the comparison, its error is one rounding of
    # the value (2^-53 of its size) plus at most 2^-8 of LAPACK's (a factor 8 left for the two algorithms' constants)
    assert e_mu <= 2.0 ** -53 * (abs(h["mean"]) + math.sqrt(h["amp"]) * 4) + 2.0 ** -8 * o_mu
    assert e_var <= 2.0 ** -53 * h["amp"] + 2.0 ** -8 * o_var
