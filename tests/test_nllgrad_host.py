"""CPU checks of the likelihood gradient's three host statements (tests/_nllgrad_ref.py), of the library's bounded L-BFGS
(b7_lbfgsb_minimize through a ctypes callback) and of the new surface (header, Lua cdef, bindings, build list, model refusals).
Nothing here needs a GPU: the optimiser is host code of the library."""
import os
import re

import mpmath
import numpy as np
import pytest

import _nllgrad_ref as R
from _nllgrad_ref import MATERN, SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNS = (SE, MATERN)

# The margin by which the library's result may sit above scipy's L-BFGS-B from the same start.  Both stop on a projected gradient of
# 1e-5 (ours relative to max(1, |f|), scipy's pgtol absolute) and scipy also on a relative decrease below 2.2e-9 (factr = 1e7), so two
# correct runs end within a stopping tolerance's worth of value of the same minimum, not on the same bits.  Measured over the cases
# below and the two GP fits of tests/test_gpu_nllgrad.py: the largest excess of ours over scipy's was 1.1e-10 max(1, |f|) (the GP fit at
# N = 150: 4.3e-9 at f = -38.7; the bounded quadratic 2.5e-11; the Rosenbrock cases are negative: ours is lower).  The margin is that
# figure with one decimal order of head room for another libm or BLAS under scipy, and it is below half of scipy's own
# relative-decrease tolerance: an end point a hundred times further from the minimum than today's fails.
SCIPY_MARGIN = 1e-9


def _margin(f):
    return SCIPY_MARGIN * max(1.0, abs(f))


# ---- 1. the three statements of the gradient ------------------------------------------------------------------------------------
def _kappa_bound(N, h):
    """An upper bound of cond(K): lambda_max <= N amp + noise (Gershgorin, |k| <= amp), lambda_min >= noise."""
    return (N * h["amp"] + h["noise"]) / h["noise"]


_MP = {}


def _truth(N, d, kern, seed=3):
    key = (N, d, kern, seed)
    if key not in _MP:
        X, y, h = R.problem(N, d, seed)
        _MP[key] = (X, y, h, R.nll_grad_mp(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern))
    return _MP[key]


@pytest.mark.parametrize("kern", KERNS)
@pytest.mark.parametrize("N", [1, 2, 12, 24])
def test_float64_form_against_50_digits(N, kern):
    """A backward-stable factorisation and inverse leave errors of a small multiple of N eps cond(K) relative to the size of the
    terms summed: each component is held to 8 N eps cond_bound x scale (scale: the 50-digit sum of the absolute terms), the value
    to the same multiple of its own terms."""
    X, y, h, (nll, grad, scale) = _truth(N, 3, kern)
    v, g, s64 = R.nll_grad_f64(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern)
    bound = 8.0 * N * R.EPS * _kappa_bound(N, h)
    worst = 0.0
    for k in range(len(grad)):
        err, lim = abs(float(mpmath.mpf(float(g[k])) - grad[k])), bound * float(scale[k])
        worst = max(worst, err / lim if lim > 0 else (0.0 if err == 0 else np.inf))
        assert err <= lim, (N, kern, k, err, lim)
        assert abs(s64[k] - float(scale[k])) <= 1e-6 * float(scale[k]) + 1e-300
    assert abs(float(mpmath.mpf(v) - nll)) <= bound * (abs(float(nll)) + N)
    print("f64 vs 50 digits N=%d %s worst err/bound %.3g" % (N, kern, worst))


@pytest.mark.parametrize("kern", KERNS)
def test_longdouble_form_against_50_digits(kern):
    """The same bound with the long double's unit roundoff (2^-63 on x86; where long double is double, double's)."""
    N = 24
    X, y, h, (nll, grad, scale) = _truth(N, 3, kern)
    v, g, _ = R.nll_grad_ld(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern)
    bound = 8.0 * N * float(np.finfo(np.longdouble).eps) / 2 * _kappa_bound(N, h)
    worst = 0.0
    for k in range(len(grad)):
        with mpmath.workdps(R.DPS):
            err = abs(float(R.ld_to_mp(g[k]) - grad[k]))
        lim = bound * float(scale[k])
        worst = max(worst, err / lim)
        assert err <= lim, (kern, k, err, lim)
    print("longdouble vs 50 digits %s worst err/bound %.3g" % (kern, worst))


@pytest.mark.parametrize("kern", KERNS)
def test_50_digit_form_against_a_central_difference(kern):
    """(nll(theta + h e_k) - nll(theta - h e_k)) / 2h at h = 1e-15 in 50 digits: truncation h^2 nll'''/6 ~ 1e-30 x the terms, rounding
    1e-50 / h = 1e-35 x them; held to 1e-24 x scale.  This is what checks the 1/4 and the 1/2."""
    N, d = 6, 2
    X, y, h = R.problem(N, d, 11)
    _, grad, scale = R.nll_grad_mp(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern)
    cd = R.central_difference_mp(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern)
    worst = 0.0
    for k in range(d + 3):
        err = abs(grad[k] - cd[k])
        worst = max(worst, float(err / scale[k]))
        assert err <= mpmath.mpf(10) ** -24 * scale[k], (kern, k, grad[k], cd[k])
    print("50 digits vs central difference %s worst err/scale %.3g" % (kern, worst))


def test_noise_zero_component_and_jitter_constant():
    """noise == 0: the noise component is exactly 0 in every form; a jitter enters K but is not differentiated."""
    X, y, h = R.problem(12, 2, 5)
    _, g, _ = R.nll_grad_f64(X, y, h["lenscale_sq"], h["amp"], 0.0, h["mean"], SE, jitter=1e-3)
    assert g[3] == 0.0
    _, gm, _ = R.nll_grad_mp(X, y, h["lenscale_sq"], h["amp"], 0.0, h["mean"], SE, jitter=1e-3)
    assert gm[3] == 0
    _, g2, _ = R.nll_grad_f64(X, y, h["lenscale_sq"], h["amp"], 1e-3, h["mean"], SE)
    assert np.allclose(g[[0, 1, 2, 4]], g2[[0, 1, 2, 4]], rtol=1e-12, atol=0)


# ---- 2. the optimiser --------------------------------------------------------------------------------------------------------------
def _rosen(x):
    f = float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))
    g = np.zeros_like(x)
    g[:-1] += -400.0 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2.0 * (1.0 - x[:-1])
    g[1:] += 200.0 * (x[1:] - x[:-1] ** 2)
    return f, g


def _scipy(fun, x0, lo, hi):
    from scipy.optimize import minimize
    return minimize(fun, np.asarray(x0, dtype=np.float64), jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                    options={"maxiter": 2000, "maxfun": 20000})


def test_quadratic_with_the_minimiser_outside_the_box():
    """f = 1/2 sum a_i (x_i - c_i)^2 is separable, so the constrained minimiser is c clipped to the box, with the bounds active
    exactly where c lies outside."""
    from bot7_amd import _lib
    a = np.array([1.0, 4.0, 0.5, 9.0, 2.0])
    c = np.array([3.0, -2.0, 0.25, 0.75, 1.5])
    lo, hi = np.zeros(5), np.ones(5)
    r = _lib.lbfgsb_minimize(lambda x: (0.5 * float(np.sum(a * (x - c) ** 2)), a * (x - c)), np.full(5, 0.5), lo, hi)
    want = np.clip(c, lo, hi)
    assert r["status"] == _lib.LBFGSB_CONVERGED, r
    assert np.array_equal(r["x"][[0, 1, 4]], want[[0, 1, 4]])            # the active bounds, exactly
    assert np.max(np.abs(r["x"] - want)) <= 1e-5, r["x"]
    s = _scipy(lambda x: (0.5 * float(np.sum(a * (x - c) ** 2)), a * (x - c)), np.full(5, 0.5), lo, hi)
    print("quadratic: ours - scipy %.3g" % (r["f"] - s.fun))
    assert r["f"] <= s.fun + _margin(s.fun)


@pytest.mark.parametrize("n", [2, 10])
def test_rosenbrock(n):
    from bot7_amd import _lib
    x0 = np.full(n, -1.2)
    x0[1::2] = 1.0
    lo, hi = np.full(n, -5.0), np.full(n, 5.0)
    r = _lib.lbfgsb_minimize(_rosen, x0, lo, hi, max_iters=1000)
    s = _scipy(_rosen, x0, lo, hi)
    print("rosenbrock %d: ours %.3g in %d iterations, %d evaluations; scipy %.3g in %d, %d; ours - scipy %.3g"
          % (n, r["f"], r["iters"], r["evals"], s.fun, s.nit, s.nfev, r["f"] - s.fun))
    assert r["status"] == _lib.LBFGSB_CONVERGED, r
    assert np.max(np.abs(r["x"] - 1.0)) <= 1e-3
    assert r["f"] <= s.fun + _margin(s.fun)
    assert r["f"] <= _rosen(x0)[0]


def test_nan_on_half_the_box_is_never_stepped_into():
    """f is NaN for x_0 > 0.5; the minimiser over the rest, (0.4, 0.8, 0.8), lies inside the finite half, and the first full step from
    the start lands in the NaN half.  Every evaluation is recorded: some did land there (the case is not vacuous), the result is an
    evaluated finite point and the lowest finite value ever seen, never above the start's, and it is the minimiser."""
    from bot7_amd import _lib
    c = np.array([0.4, 0.8, 0.8])
    seen = []

    def f(x):
        if x[0] > 0.5:
            seen.append((x.copy(), float("nan")))
            return float("nan"), np.full(3, np.nan)
        v = float(np.sum((x - c) ** 2))
        seen.append((x.copy(), v))
        return v, 2.0 * (x - c)
    x0 = np.full(3, -0.9)
    r = _lib.lbfgsb_minimize(f, x0, -np.ones(3), np.ones(3))
    finite = [v for _, v in seen if np.isfinite(v)]
    assert r["evals"] == len(seen) and len(finite) < len(seen)           # trial points did land in the NaN half
    assert np.array_equal(seen[0][0], x0) and r["f"] <= seen[0][1]
    assert r["x"][0] <= 0.5 and r["f"] == min(finite)                    # it ends on the best finite value it ever saw ...
    assert any(np.array_equal(x, r["x"]) and v == r["f"] for x, v in seen)   # ... which is an evaluated point
    assert r["status"] == _lib.LBFGSB_CONVERGED and np.max(np.abs(r["x"] - c)) <= 1e-5, r
    # a start on the edge of the finite half whose every descent step leaves it: x0 comes back, with the failed-line-search bit
    nan_seen = []

    def edge(x):
        if x[0] > 0.5:
            nan_seen.append(x.copy())
            return float("nan"), np.full(3, np.nan)
        return -float(x[0]), np.array([-1.0, 0.0, 0.0])
    r2 = _lib.lbfgsb_minimize(edge, np.array([0.5, 0.0, 0.0]), -np.ones(3), np.ones(3))
    assert np.array_equal(r2["x"], [0.5, 0.0, 0.0]) and r2["f"] == -0.5 and r2["status"] & _lib.LBFGSB_LINESEARCH
    assert len(nan_seen) == r2["evals"] - 1 and len(nan_seen) >= 20      # every trial point was refused, down to the last halving


def test_fixed_component_and_zero_iterations():
    from bot7_amd import _lib
    lo, hi = np.array([-5.0, 0.7, -5.0]), np.array([5.0, 0.7, 5.0])
    x0 = np.array([-1.2, 0.7, 2.0])
    r = _lib.lbfgsb_minimize(_rosen, x0, lo, hi, max_iters=500)
    assert r["x"][1].tobytes() == np.float64(0.7).tobytes() and r["status"] == _lib.LBFGSB_CONVERGED
    s = _scipy(_rosen, x0, lo, hi)
    print("fixed component: ours - scipy %.3g" % (r["f"] - s.fun))
    assert r["f"] <= s.fun + _margin(s.fun)
    r0 = _lib.lbfgsb_minimize(_rosen, x0, lo, hi, max_iters=0)
    assert np.array_equal(r0["x"], x0) and r0["f"] == _rosen(x0)[0] and r0["evals"] == 1 and r0["status"] == _lib.LBFGSB_MAX_ITERS
    r3 = _lib.lbfgsb_minimize(_rosen, x0, lo, hi, max_evals=3)
    assert r3["evals"] == 3 and r3["status"] & _lib.LBFGSB_MAX_EVALS and r3["f"] <= r0["f"]


def test_invalid_arguments():
    import ctypes as C
    from bot7_amd import _lib
    ok = (np.zeros(2), -np.ones(2), np.ones(2))
    for x0, lo, hi in [(np.array([np.nan, 0.0]), ok[1], ok[2]), (np.array([np.inf, 0.0]), ok[1], ok[2]), (np.array([2.0, 0.0]), ok[1], ok[2]),
                       (ok[0], np.array([0.5, -1.0]), np.array([0.25, 1.0])), (np.zeros(0), np.zeros(0), np.zeros(0)),
                       (np.zeros(100), -np.ones(100), np.ones(100))]:
        with pytest.raises(_lib.Bot7HipError) as e:
            _lib.lbfgsb_minimize(_rosen, x0, lo, hi)
        assert e.value.code == -1
    L = _lib.load()
    x = np.zeros(2)
    assert L.b7_lbfgsb_minimize(None, None, 2, _lib._ptr(ok[0]), _lib._ptr(ok[1]), _lib._ptr(ok[2]), None, _lib._ptr(x), None, None, None, None, None) == -1
    assert L.b7_lbfgsb_default_opts(None) == -1
    o = _lib.LbfgsbOpts()
    assert L.b7_lbfgsb_default_opts(C.byref(o)) == 0 and (o.max_iters, o.max_evals, o.gtol) == (50, 0, 0.0)


def test_the_same_bits_twice_and_an_exception_passes_through():
    from bot7_amd import _lib
    x0, lo, hi = np.array([-1.2, 1.0, -0.5, 0.3]), np.full(4, -2.0), np.full(4, 2.0)
    a, b = (_lib.lbfgsb_minimize(_rosen, x0, lo, hi, max_iters=200) for _ in range(2))
    assert a["x"].tobytes() == b["x"].tobytes() and a["g"].tobytes() == b["g"].tobytes()
    assert (a["f"], a["iters"], a["evals"], a["status"]) == (b["f"], b["iters"], b["evals"], b["status"])

    def boom(x):
        raise KeyError("from the objective")
    with pytest.raises(KeyError):
        _lib.lbfgsb_minimize(boom, x0, lo, hi)


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------
NEW = ["b7_gp_fit_hyp_grad", "b7_gp_nll_grad", "b7_lbfgsb_default_opts", "b7_lbfgsb_minimize", "b7_gp_fit_map", "b7_gp_fit_map_trace_enable",
       "b7_gp_fit_map_trace"]


def test_header_lua_bindings_and_build_list_carry_the_new_entries():
    from bot7_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert re.search(r"\bint %s\(" % name, lua), name
        assert name in _lib.SYMBOLS
    assert "#define B7_ABI_VERSION 1\n" in header
    assert "b7_lbfgsb_opts" in lua and "b7_objective_fn" in lua
    assert "nll_grad.hip" in build.SOURCES and "lbfgsb.hip" in build.SOURCES
    for f in ("nll_grad.hip", "lbfgsb.hip", "lbfgsb.h"):
        assert os.path.exists(os.path.join(ROOT, "bot7_amd", "csrc", f))
    assert "function model:fit_map" in open(os.path.join(ROOT, "lua", "models_gp_hip.lua")).read()
    for m in ("gp_fit_hyp_grad", "gp_nll_grad", "gp_fit_map"):
        assert callable(getattr(_lib.Context, m))


def test_model_refusals_name_the_case():
    import bot7_amd
    from bot7_amd.models.gp_classifier import gp_classifier
    from bot7_amd.models.dngo import dngo
    G = bot7_amd.models.gp_regressor
    with pytest.raises(NotImplementedError, match="sample = True"):
        G({"fit": "map", "sample": True})
    with pytest.raises(NotImplementedError, match="only 'map'"):
        G({"fit": "newton"})
    with pytest.raises(NotImplementedError, match="gp_classifier.*fit"):
        gp_classifier({"fit": "map"})
    with pytest.raises(NotImplementedError, match="dngo.*fit"):
        dngo({"fit": "map", "network": {"weights": [np.zeros((2, 2))], "biases": [np.zeros(2)]}})
    m = G({"fit": "map"}, context=object())
    X = np.random.default_rng(0).random((5, 2))
    with pytest.raises(NotImplementedError, match="2 response columns"):
        m.sample_hypers(X, np.zeros((5, 2)))

    class Sharded(object):
        def comm_info(self):
            return 0, 2
    with pytest.raises(NotImplementedError, match="sharded"):
        G({"fit": "map"}, context=Sharded()).sample_hypers(X, np.arange(5.0))


def test_fit_absent_returns_what_it_returns_today():
    """Without config.fit, sample_hypers (config.sample = False) is the heuristic point estimate, object for object: the vector built
    from self.hyp, which init made and nothing replaced; no context is touched."""
    import bot7_amd
    m = bot7_amd.models.gp_regressor({}, context=object())
    X = np.random.default_rng(1).random((7, 3))
    Y = np.sin(X.sum(axis=1))
    v = m.sample_hypers(X, Y)
    hyp = m.hyp
    want = np.concatenate([np.full(3, 3 / 8.0), [np.var(Y), 1e-4 * np.var(Y), np.mean(Y)]])
    assert v.tobytes() == want.tobytes()
    assert m.sample_hypers(X, Y).tobytes() == want.tobytes() and m.hyp is hyp and m.last_fit is None
