"""Host tests of tests/_blr_ref.py, the references of tests/test_gpu_blr.py.  No GPU: float64 numpy stands in for the device where
a bar is checked, so that every bar is shown to admit an honest float64 evaluation before a kernel is held to it."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import _blr_ref as R
import _exact as E


def _numpy_head(p, alpha, beta, mean):
    """The head in plain float64 numpy, arranged as the device arranges it: L, L^-1, m = L^-T (L^-1 q)."""
    A = beta * (p.Z0.T @ p.Z0) + alpha * np.eye(p.z)
    q = p.Z0.T @ (beta * (p.Y.ravel() - mean))
    return R.lapack_head(A, q)


def test_truth_agrees_with_itself_at_50_and_80_digits():
    p = R.problem(65, 48, 8)
    a, b = (R.blr_truth(p.Z0, p.Y, *R.SMALL_HYP, p.Z1, dps=dps) for dps in (50, 80))
    with mpmath.workdps(80):
        for va, vb in zip([a.raw[1]] + a.raw[0] + a.raw[2] + a.raw[3], [b.raw[1]] + b.raw[0] + b.raw[2] + b.raw[3]):
            assert abs(va - vb) <= mpmath.mpf(10) ** -38 * abs(vb)


@pytest.mark.parametrize("N,z", [(63, 16), (65, 49), (10, 64), (200, 50)])
def test_truth_agrees_with_lapack_to_cond_eps(N, z):
    p = R.problem(N, z, 16)
    al, be, mn = R.SMALL_HYP
    t, o = R.blr_truth(p.Z0, p.Y, al, be, mn, p.Z1), R.lapack_blr(p.Z0, p.Y, al, be, mn, p.Z1)
    cond = np.linalg.cond(t.A)
    assert 1e4 < cond < 1e9
    m = t.m[0]
    assert np.linalg.norm(E.abs_errors(o["m"], *t.m)) <= cond * E.EPS * np.linalg.norm(m)
    assert R.err_pairs(o["mu"], t.mu) <= cond * E.EPS * (abs(mn) + np.abs(p.Z1 * m).sum(1).max())
    assert R.err_pairs(o["var"], t.var) <= cond * E.EPS * t.var[0].max()
    assert R.err_pairs([o["nll"]], t.nll) <= cond * E.EPS * abs(t.nll[0][0])


def test_dyadic_features_are_the_same_bits_in_every_order():
    p = R.problem(80, 50, 300)
    W, b = p.W[0], p.b[0]
    for X, Z in ((p.X, p.Z0), (p.Xg, p.Z1)):
        assert np.array_equal(np.maximum(X @ W.T + b, 0.0), Z)
        assert np.array_equal(np.maximum((W @ X.T).T + b, 0.0), Z)
        assert np.array_equal(np.maximum((W[:, ::-1] @ X[:, ::-1].T).T + b, 0.0), Z)
        fs = np.array([[max(math.fsum([W[k, i] * x[i] for i in range(R.D)] + [b[k]]), 0.0) for k in range(p.z)] for x in X[:40]])
        assert np.array_equal(fs, Z[:40])
    dead = (p.Z0 == 0.0).all(0)
    assert dead.any() and not dead.all()       # A_ii = alpha exactly on the dead ones: an edge the GPU tests keep


def test_int64_gram_and_exact_head_equal_fractions():
    p = R.problem(20, 6, 4)
    al, be, mn = R.WIDE_HYP
    ZF = [[Fraction(float(v)) for v in row] for row in p.Z0]
    GF = [[sum(ZF[n][i] * ZF[n][j] for n in range(p.N)) for j in range(p.z)] for i in range(p.z)]
    G = R.int_gram(p.Z0)
    assert all(Fraction(int(G[i, j]), 1 << (2 * R.Z_BITS)) == GF[i][j] for i in range(p.z) for j in range(p.z))
    A, q = R.exact_head(p.Z0, p.Y, al, be, mn)
    for i in range(p.z):
        assert Fraction(float(q[i])) == Fraction(be) * sum(ZF[n][i] * (Fraction(float(p.Y[n, 0])) - Fraction(mn)) for n in range(p.N))
        for j in range(p.z):
            assert Fraction(float(A[i, j])) == Fraction(be) * GF[i][j] + (Fraction(al) if i == j else 0)


def test_the_pivot_construction_has_a_zero_second_pivot():
    W, b, X, Y, alpha, beta = R.pivot_case()
    Z0 = R.dyadic_features(X, W, b)
    assert np.array_equal(Z0[:, 0], Z0[:, 1]) and float(Z0[:, 0] @ Z0[:, 0]) == 16.0
    A = beta * (Z0.T @ Z0) + alpha * np.eye(Z0.shape[1])
    assert A[0, 0] == A[1, 0] == A[1, 1] == 16.0
    assert E.min_pivot(A) == 0.0
    # with S heads: beta = 4 keeps every step exact as well (A_11 = 64, sqrt 8, 64 - 8 * 8 = 0)
    assert E.min_pivot(4.0 * (Z0.T @ Z0) + alpha * np.eye(Z0.shape[1])) == 0.0


@pytest.mark.parametrize("N,z", R.SMALL_CASES + R.WIDE_CASES)
def test_numpy_stays_within_the_exact_evaluation_bars(N, z):
    """The reference alone must pass its own bars: numpy's matrix products of the head's L^-1 and m over the features, against
    the exact evaluation of the same operands."""
    small = (N, z) in R.SMALL_CASES
    p = R.problem(N, z, 300 if small else 64)
    al, be, mn = R.SMALL_HYP if small else R.WIDE_HYP
    if small:
        L, Li, m = _numpy_head(p, al, be, mn)
    else:
        L, Li, m = R.lapack_head(*R.exact_head(p.Z0, p.Y, al, be, mn))
    invbeta = 1.0 / be
    var = invbeta + ((p.Z1 @ Li.T) ** 2).sum(1)
    hi, lo = R.exact_var_rows(Li, p.Z1, invbeta)
    rv = float((E.abs_errors(var, hi, lo) / R.var_bar(z, hi)).max())
    mu = mn + p.Z1 @ m
    mh, ml, ab = R.exact_mean_rows(m, p.Z1, mn)
    rm = float((E.abs_errors(mu, mh, ml) / R.mean_bar(z, mn, ab)).max())
    print("N %d z %d: numpy error / bar: variance %.3f, mean %.3f" % (N, z, rv, rm))
    assert rv <= 1.0 and rm <= 1.0
    assert (var >= invbeta).all()


def test_exact_evaluation_equals_fractions():
    p = R.problem(17, 5, 3)
    _, Li, m = _numpy_head(p, *R.SMALL_HYP)
    invbeta, mn = 1.0 / R.SMALL_HYP[1], R.SMALL_HYP[2]
    hi, lo = R.exact_var_rows(Li, p.Z1, invbeta)
    mh, ml, _ = R.exact_mean_rows(m, p.Z1, mn)
    for j, phi in enumerate(p.Z1):
        v = [sum(Fraction(float(Li[i, k])) * Fraction(float(phi[k])) for k in range(i + 1)) for i in range(p.z)]
        want = Fraction(invbeta) + sum(x * x for x in v)
        assert hi[j] == float(want) and abs(Fraction(float(hi[j])) + Fraction(float(lo[j])) - want) <= want * Fraction(1, 2 ** 100)
        want = Fraction(mn) + sum(Fraction(float(phi[k])) * Fraction(float(m[k])) for k in range(p.z))
        assert mh[j] == float(want) and abs(Fraction(float(mh[j])) + Fraction(float(ml[j])) - want) <= abs(want) * Fraction(1, 2 ** 100)
