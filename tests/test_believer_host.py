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
