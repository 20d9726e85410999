"""The kriging-believer algebra without a GPU: the rank-one variance downdate (include/bot7hip.h, b7_eval_nominate_batch) equals
a refit with the believed points appended at their own posterior means -- in float64 against numpy / scipy, and at 50 digits
against tests/_exact.py's GP -- and the posterior mean does not move."""
import mpmath
import numpy as np
import pytest

import _believer_ref as R
import _exact as E


def _problem(N, d, M, S, seed):
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(N)
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.3, 1.5, d) * d / 4.0, "amp": amp * rng.uniform(0.7, 1.4), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.1 * rng.standard_normal()} for _ in range(S)]
    return X, y, Xc, hyps


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("N,d,M", [(24, 3, 97), (60, 6, 131)])
def test_downdate_equals_refit_float64(N, d, M, kernel):
    X, y, Xc, hyps = _problem(N, d, M, 2, seed=N + d)
    rows = [5, 40, 41, 96]
    for h in hyps:
        b = R.Believer(X, y, Xc, h, kernel)
        mu0 = b.mu.copy()
        for j, r in enumerate(rows):
            b.believe(r)
            mu, var = R.refit(X, y, Xc, h, kernel, rows[:j + 1])
            # the refit's own rounding: an (N + j)-point solve at condition amp / noise = 100 .. 200
            assert np.max(np.abs(var - b.var)) <= 1e-11 * h["amp"]
            assert np.max(np.abs(mu - mu0)) <= 1e-11 * max(1.0, np.max(np.abs(mu0)))   # the mean is unchanged by the lie
            assert np.all(b.var > 0.0) and np.all(b.var <= b.p.var + 1e-15)            # a downdate never adds variance
        # a believed row keeps var noise / (var + noise) of its variance at its own downdate; later ones only lower it
        assert b.var[rows[-1]] <= h["noise"]


def test_downdate_equals_refit_50_digits():
    """One shape at 50 digits (tests/_exact.py's gp_truth): the float64 recurrence against the exact refit."""
    N, d, M = 7, 2, 6
    X, y, Xc, hyps = _problem(N, d, M, 1, seed=3)
    h = hyps[0]
    rows = [1, 4]
    b = R.Believer(X, y, Xc, h, "ardse")
    Xa, ya = X, y
    t0 = E.gp_truth(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xc)
    for r in rows:
        t = E.gp_truth(Xa, ya, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xc)
        Xa, ya = np.vstack([Xa, Xc[r]]), np.append(ya, float(t.mu[r]))   # the lie, rounded to a double
        b.believe(r)
    t = E.gp_truth(Xa, ya, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xc)
    with mpmath.workdps(50):
        dv = max(abs(mpmath.mpf(float(v)) - tv) for v, tv in zip(b.var, t.var))
        dm = max(abs(tm - tm0) for tm, tm0 in zip(t.mu, t0.mu))
    assert float(dv) <= 1e-12 * h["amp"]
    assert float(dm) <= 1e-13          # unchanged up to the rounding of the believed values to doubles


def test_greedy_sequences_agree_and_exclude():
    X, y, Xc, hyps = _problem(24, 3, 211, 3, seed=11)
    for kind, spec in (("ei", {"fmin": float(y.min())}), ("cb", {"tradeoff": 1.0}), ("logei", {"fmin": float(y.min())})):
        pa, sa, ga, _ = R.greedy(X, y, Xc, hyps, "ardse", 4, kind, "downdate", **spec)
        pb, sb, gb, _ = R.greedy(X, y, Xc, hyps, "ardse", 4, kind, "refit", **spec)
        assert pa == pb and len(set(pa)) == 4
        for a, b_ in zip(sa, sb):
            assert np.max(np.abs(a - b_) / np.maximum(1.0, np.abs(b_))) <= 1e-9


# ---- the 50-digit truth of the believer (tests/_believer_ref.believer_truth) and the float64 restatements against it ------------
ROWS16 = [5, 40, 41, 58, 0, 17, 33, 9, 26, 50, 3, 12, 47, 21, 36, 59]


@pytest.fixture(scope="module")
def truth16():
    """One 16-pick sequence (N = 24, d = 3, 60 candidates, every candidate a probe) under both kernels, the truth after every pick."""
    X, y, Xc, hyps = _problem(24, 3, 60, 1, seed=5)
    out = {}
    for kernel in ("ardse", "ardmatern52"):
        out[kernel] = R.believer_truth(X, y, Xc, hyps[0], kernel, ROWS16, range(60), after=range(17))
    return X, y, Xc, hyps[0], out


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
def test_recurrence_and_refit_agree_with_the_truth_over_16_picks(truth16, kernel):
    """Bar after j picks: 8 (N + j) eps amp, 4.4e-14 amp at j = 1 and 7.1e-14 amp at j = 16.  The variance is amp less a sum of
    n = N + j squares that add up to at most amp, each the outcome of a substitution of at most n terms against a factor whose
    entries carry sums of at most n terms: n eps amp where every stage's rounding adds up linearly, and the factor 8 (gp_bar's)
    for the stages -- K's entries, the factor, the substitution, the squares and their sum.  The worst case of the theory,
    the condition number (N + j) amp / noise = 4e3 times eps, is 8.2e-13 amp and is left far above: a stable float64 solve at
    this conditioning does not come near it, and a restatement that did would be no reference for a device held to a few
    1e-15 amp.  The truth's mean never moves: the believed values add nothing to inv(L) (y - mean), exactly."""
    X, y, Xc, h, truths = truth16
    t = truths[kernel]
    b = R.Believer(X, y, Xc, h, kernel)
    worst_b = worst_r = 0.0
    for j in range(1, 17):
        bar = 8.0 * (24 + j) * E.EPS * h["amp"]
        b.believe(ROWS16[j - 1])
        mu, var = R.refit(X, y, Xc, h, kernel, ROWS16[:j])
        eb, er = R.err_vs_truth(b.var, t[j][1]), R.err_vs_truth(var, t[j][1])
        worst_b, worst_r = max(worst_b, eb), max(worst_r, er)
        assert eb <= bar and er <= bar, (j, eb / h["amp"], er / h["amp"], bar / h["amp"])
        assert R.err_vs_truth(mu, t[j][0]) <= bar / h["amp"] * max(1.0, np.max(np.abs(mu)))
        with mpmath.workdps(50):
            assert max(abs(a - c) for a, c in zip(t[j][0], t[0][0])) < mpmath.mpf(10) ** -40
            assert all(a < c for a, c in zip(t[j][1], t[j - 1][1]))              # every downdate lowers every variance
            assert t[j][1][ROWS16[j - 1]] <= h["noise"]
    print("%s, 16 picks: recurrence %.3e amp, refit %.3e amp off the truth (bar %.3e amp at pick 1, %.3e amp at pick 16)" %
          (kernel, worst_b / h["amp"], worst_r / h["amp"], 8.0 * 25 * E.EPS, 8.0 * 40 * E.EPS))


def test_truth_is_the_textbook_gp_of_the_augmented_data(truth16):
    """believer_truth's leading-block factor against tests/_exact.gp_truth (mpmath.cholesky) on the data with the believed rows
    appended at the truth's own means, rounded to doubles: equal up to that rounding."""
    X, y, Xc, h, truths = truth16
    t = truths["ardse"]
    rows = ROWS16[:3]
    Xa, ya = np.vstack([X, Xc[rows]]), np.append(y, [float(t[0][0][r]) for r in rows])
    g = E.gp_truth(Xa, ya, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xc)
    with mpmath.workdps(50):
        assert max(abs(a - c) for a, c in zip(g.var, t[3][1])) < mpmath.mpf(10) ** -40
        assert max(abs(a - c) for a, c in zip(g.mu, t[3][0])) < 1e-13


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
def test_truth_with_jitter_is_the_truth_with_noise_plus_jitter(kernel):
    """noise = 2^-7 amp-free and jitter = 2^-20: their float64 sum is exact, so the two truths are the same numbers."""
    X, y, Xc, hyps = _problem(12, 2, 9, 1, seed=8)
    h = dict(hyps[0], noise=2.0 ** -7)
    jit = 2.0 ** -20
    a = R.believer_truth(X, y, Xc, h, kernel, [2, 7, 4], range(9), after=(0, 1, 3), jitter=jit)
    b = R.believer_truth(X, y, Xc, dict(h, noise=h["noise"] + jit), kernel, [2, 7, 4], range(9), after=(0, 1, 3))
    c = R.believer_truth(X, y, Xc, h, kernel, [2, 7, 4], range(9), after=(0, 1, 3))
    with mpmath.workdps(50):
        for j in (0, 1, 3):
            for k in (0, 1):
                assert max(abs(u - v) for u, v in zip(a[j][k], b[j][k])) < mpmath.mpf(10) ** -45
            assert max(abs(u - v) for u, v in zip(a[j][1], c[j][1])) > 1e-9      # ... and the jitter is not simply dropped
