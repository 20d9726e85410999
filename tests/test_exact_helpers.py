"""The host references of tests/test_gpu_numerics.py checked on the host (no GPU): the 50-digit GP against the oracle, the
exactness of the argument constructors, the invariances on the oracle itself, and the bars."""
import math

import numpy as np
import pytest

import _exact as E
from oracle import cport, gp


def _problem(N=16, d=2, M=32, seed=3):
    rng = np.random.default_rng(seed)
    X, Xs = rng.random((N, d)), rng.random((M, d))
    Y = np.sin(3.0 * X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, 1))
    hyp = {"lenscale_sq": np.full(d, 0.3), "amp": 1.3, "noise": 1e-2, "mean": 0.1}
    return X, Y, Xs, hyp


def test_mp_gp_agrees_with_the_oracle_on_a_well_conditioned_problem():
    X, Y, Xs, hyp = _problem()
    t = E.gp_truth(X, Y, Xs=Xs, **hyp)
    f = gp.fit(X, Y, **hyp)
    mu, var = gp.predict(f, Xs)
    assert abs(float(t.nll) - f.nll[0]) <= 1e-13 * abs(f.nll[0])
    assert E.err_vs(mu[:, 0], t.mu) <= 1e-13 * np.abs(mu).max()
    assert E.err_vs(var, t.var) <= 1e-13 * hyp["amp"]
    nll, mu2, var2 = E.lapack_fit(X, Y, Xs=Xs, **hyp)      # the oracle's algebra with a given jitter (here none): the oracle
    assert nll == pytest.approx(f.nll[0], rel=1e-15) and np.array_equal(mu2, mu[:, 0]) and np.array_equal(var2, var)


@pytest.mark.parametrize("d", [1, 6, 32])
@pytest.mark.parametrize("j", [0, 2, -1])
def test_exp_argument_constructors_are_exact_in_float64(d, j):
    targets = E.exp_targets(dense=512)
    X, args = E.exp_points(targets, d, j)
    assert np.all(np.abs(X * 1024.0 - np.round(X * 1024.0)) == 0)
    for x, a, t in zip(X, args, targets):
        assert E.exp_arg_float64(x, j) == a          # float64 evaluation equals the exact (Fraction) argument
        if d >= 6:
            assert abs(float(a) - t) <= 2.0 ** (-20 - 2 * j) * 64   # and the target is reached (d >= 4: sums of squares)
    Xs, sargs = E.special_exp_rows(d)
    for x, a in zip(Xs[:-1], sargs[:-1]):
        assert E.exp_arg_float64(x, 0) == a
    assert sargs[0] == 0 and sargs[1] == -E.Fraction(1, 2 ** 1001) and (d < 2 or sargs[2] == -1000)


@pytest.mark.parametrize("ls", [4.0 ** -3, 4.0 ** 6])
def test_grid_data_distances_are_exact_in_the_oracle(ls):
    X, _ = E.grid_data(40, 6, seed=1)
    D = gp.pdist(X, None, np.full(6, ls))
    for a in range(40):
        for b in range(40):
            exact = sum((E.Fraction(float(X[a, k])) - E.Fraction(float(X[b, k]))) ** 2 for k in range(6)) / E.Fraction(ls)
            assert E.Fraction(float(D[a, b])) == exact


def test_exp_targets_cover_every_residue_and_the_subnormal_range():
    t = np.array(E.exp_targets())
    n = np.rint(t * 128 / math.log(2.0)).astype(np.int64)
    for hi in (-1, -3, -40, -200):
        assert set((n[(n >> 7) == hi] & 127).tolist()) == set(range(128))
    assert ((t > -745) & (t < -708)).sum() >= 400 and (t == -1000).any() and (t < -1000).sum() >= 3
    assert t.max() <= 0


def test_truth_and_bars_accept_the_exact_value_and_reject_32_ulp():
    X, args = E.exp_points(E.exp_targets(dense=256), 6, 0)
    for amp in (2.0 ** -40, 1e-3, 3.0, 2.0 ** 40):
        hi, lo = E.amp_exp_truth(amp, args)
        ok, wu, wa = E.within_bar(hi, hi, lo, 4)
        assert ok and wu <= 0.5 and wa <= 2.0 ** -1074
        normal = np.abs(hi) >= E.TINY
        bad = hi.copy()
        bad[normal] += 32 * E.ulp_of(hi[normal])
        assert not E.within_bar(bad, hi, lo, 4)[0]
    xs = E.activation_inputs()
    for kind in ("Tanh", "Sigmoid", "ReLU"):
        hi, lo = E.activation_truth(kind, xs)
        ref = E.numpy_activation(kind, xs)
        ok, wu, _ = E.within_bar(ref, hi, lo, 4)
        assert ok, (kind, wu)
        bad = ref.copy()
        i = np.abs(hi) >= E.TINY
        bad[i] += 32 * E.ulp_of(hi[i])
        assert not E.within_bar(bad, hi, lo, 6)[0]
    assert np.isnan(E.numpy_activation("ReLU", np.array([np.nan])))[0]


def test_gp_bar_accepts_the_oracle_and_rejects_32_ulp():
    X, Y, Xs, hyp = _problem(N=16, d=2)
    t = E.gp_truth(X, Y, Xs=Xs, **hyp)
    nll, mu, var = E.lapack_fit(X, Y, Xs=Xs, **hyp)
    for got, truth, scale in ((np.array([nll]), [t.nll], abs(nll)), (mu, t.mu, math.sqrt(hyp["amp"]) + abs(hyp["mean"])),
                              (var, t.var, hyp["amp"])):
        e_o = E.err_vs(got, truth)
        assert e_o <= E.gp_bar(e_o, scale)
        # against a reference as good as the correctly rounded truth, 32 ulp of the scale is outside the bar
        hi, _ = E.pairs(truth)
        bar = E.gp_bar(E.err_vs(hi, truth), scale)
        assert E.err_vs(hi, truth) <= bar and E.err_vs(hi + 32 * E.ulp_of(np.full_like(hi, scale)), truth) > bar


def test_jitter_schedule_and_min_pivot():
    K = np.ones((4, 4))
    sched = E.jitter_schedule(np.linalg.norm(K))
    L, jit, info = gp.chol_jitter(K)
    assert jit in sched and info != 0
    assert abs(E.min_pivot(K)) <= 4 * E.EPS * np.linalg.norm(K)
    assert E.min_pivot(np.eye(3) * 2.0) == 2.0


def _oracle_all(X, Y, Xs, h, fmin):
    f = gp.fit(X, Y, **h)
    mu, var = gp.predict(f, Xs)
    return f, mu, var, cport.ei(mu, var, [fmin]), cport.cb(mu, var)


@pytest.mark.parametrize("k", [-20, -3, 5, 20])
def test_oracle_obeys_the_y_scaling_relation_bit_for_bit(k):
    X, Y, Xs, hyp = _problem(N=24, d=3, M=200)
    f, mu, var, ei, cb = _oracle_all(X, Y, Xs, hyp, float(Y.min()))
    h2, Y2 = E.scale_y(hyp, Y, k)
    f2, mu2, var2, ei2, cb2 = _oracle_all(X, Y2, Xs, h2, float(Y2.min()))
    assert f.jitter == 0 and f2.jitter == 0
    assert np.array_equal(f2.L, np.ldexp(f.L, k)) and np.array_equal(f2.alpha, np.ldexp(f.alpha, -k))
    assert np.array_equal(mu2, np.ldexp(mu, k)) and np.array_equal(var2, np.ldexp(var, 2 * k))
    assert np.array_equal(ei2, np.ldexp(ei, k)) and np.array_equal(cb2, np.ldexp(cb, k))
    assert cport.argmax_first(ei2)[0] == cport.argmax_first(ei)[0]
    shift = f2.nll[0] - f.nll[0]
    assert abs(shift - 24 * k * math.log(2.0)) <= 8 * E.EPS * max(abs(f.nll[0]), abs(f2.nll[0]))


@pytest.mark.parametrize("j", [-4, 3])
def test_oracle_obeys_the_x_scaling_relation_bit_for_bit(j):
    X, Y, Xs, hyp = _problem(N=24, d=3, M=200)
    f, mu, var, ei, cb = _oracle_all(X, Y, Xs, hyp, float(Y.min()))
    h2, X2 = E.scale_x(hyp, X, j)
    _, Xs2 = E.scale_x(hyp, Xs, j)
    f2, mu2, var2, ei2, cb2 = _oracle_all(X2, Y, Xs2, h2, float(Y.min()))
    for a, b in ((f.L, f2.L), (f.alpha, f2.alpha), (f.nll, f2.nll), (mu, mu2), (var, var2), (ei, ei2), (cb, cb2)):
        assert np.array_equal(a, b)


def test_oracle_obeys_the_permutation_relation_bit_for_bit():
    X, Y, Xs, hyp = _problem(N=24, d=3, M=1000)
    f = gp.fit(X, Y, **hyp)
    perm = np.random.default_rng(5).permutation(1000)[::-1]
    mu, var = gp.predict(f, Xs)
    mu2, var2 = gp.predict(f, Xs[perm])
    ei, ei2 = cport.ei(mu, var, [float(Y.min())]), cport.ei(mu2, var2, [float(Y.min())])
    # row-wise kernels give position-independent bits; numpy's matrix products may not, so compare to rounding here and
    # leave the bit-for-bit statement to the device, whose kernels are row-wise by construction
    assert np.allclose(mu2, mu[perm], rtol=4 * E.EPS, atol=0) and np.allclose(var2, var[perm], rtol=1e-12, atol=0)
    assert perm[cport.argmax_first(ei2)[0] - 1] == cport.argmax_first(ei)[0] - 1
