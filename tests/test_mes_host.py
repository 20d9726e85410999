"""Max-value entropy search without a GPU: the references of tests/_mes_ref.py against 50-digit arithmetic and against each other,
the float64 restatement of the device's h(g), the score's registry entry and its device spec."""
import math

import mpmath
import numpy as np
from scipy import special

import bot7_amd.scores as Scores

import _mes_ref as R


def test_h_has_its_known_values_and_decreases():
    """h(0) = log 2; h -> 0 from above as g grows; h strictly decreasing on [-8, 38] (a candidate far above the minimum's value
    tells nothing about it, one below it tells a lot)."""
    with mpmath.workdps(R.DPS):
        assert abs(R.h_mp(0.0) - mpmath.log(2)) < mpmath.mpf(10) ** -45
        gs = np.linspace(-8.0, 38.0, 4601)
        hs = [R.h_mp(float(g)) for g in gs]
        assert all(a > b for a, b in zip(hs, hs[1:]))
        assert hs[-1] > 0 and hs[-1] < mpmath.mpf(10) ** -300
        # against the definition with Phi from mpmath's own normal CDF, where that is well conditioned
        for g in (-8.0, -2.5, -1.0, -0.3, 0.0, 0.7, 3.0):
            cdf = mpmath.ncdf(g)
            want = mpmath.mpf(g) * mpmath.npdf(g) / (2 * cdf) - mpmath.log(cdf)
            assert abs(R.h_mp(g) - want) <= mpmath.mpf(10) ** -40 * max(1, abs(want))


def test_float64_restatement_of_h_meets_the_device_bar():
    """The formula of mes_math.h with scipy's erfc / erfcx in place of ocml's, g in [-8, 40] packed around the branch points 0 and
    -1: within 1e-13 max(1, |h|) of 50 digits (measured 6.5e-15 at g = -7.9); finite on [-1e6, -8)."""
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.uniform(-8.0, 40.0, 3000), rng.normal(scale=0.02, size=300), -1.0 + rng.normal(scale=0.02, size=300),
                        [0.0, -1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -8.0, 40.0]])
    g = g[(g >= -8.0) & (g <= 40.0)]
    with mpmath.workdps(R.DPS):
        ref = [R.h_mp(float(x)) for x in g]
    err = R.scaled_errors(R.h_np(g), ref)
    print("h, float64 restatement: worst scaled error %.3g at g = %.6g" % (err.max(), g[err.argmax()]))
    assert err.max() <= R.BAR
    far = R.h_np(-np.exp(rng.uniform(math.log(8.0), math.log(1e6), 500)))
    assert np.isfinite(far).all()


def test_log_survival_against_50_digits():
    mu, var = R.distribution("u1", 64)
    for y in (-4.0, -2.5, -2.0, 0.0):
        with mpmath.workdps(R.DPS):
            want = sum(R.log_ndtr_mp((mpmath.mpf(float(m)) - mpmath.mpf(y)) / mpmath.sqrt(mpmath.mpf(float(v)))) for m, v in zip(mu, var))
            got = mpmath.mpf(R.log_survival(y, mu, var))
            assert abs(got - want) <= mpmath.mpf(4e-15) * abs(want)


def test_ystar_reference_brackets_the_root():
    """One row: L = log Phi((mu - y)/sigma) and y*_k = mu + sigma Phi^-1(u_k), in closed form.  A grid: the returned double and its
    predecessor straddle the target, the roots increase with k and lie in the bracket; rows of the other classes change nothing."""
    for K in (1, 8):
        u = (np.arange(1, K + 1) - 0.5) / K
        got = R.ystar_ref([0.25], [4.0], K)
        assert np.allclose(got, 0.25 + 2.0 * special.ndtri(u), rtol=0, atol=1e-14)
    mu, var = R.distribution("u2", 257)
    lo0, hi0 = R.bracket(mu, var)
    ys, t = R.ystar_ref(mu, var, 8), R.targets(8)
    assert (np.diff(ys) > 0).all() and lo0 < ys[0] and ys[-1] < hi0
    for y, tk in zip(ys, t):
        assert R.log_survival(np.nextafter(y, -np.inf), mu, var) > tk >= R.log_survival(y, mu, var)
    mu2 = np.insert(mu, [3, 100, 200, 250], [0.0, np.nan, -50.0, 1.0])
    var2 = np.insert(var, [3, 100, 200, 250], [0.0, 1.0, -1.0, np.nan])
    assert R.ystar_ref(mu2, var2, 8).tobytes() == ys.tobytes() and R.bracket(mu2, var2) == (lo0, hi0)
    assert np.isnan(R.ystar_ref([0.0, np.nan], [0.0, 1.0], 3)).all()


def test_reference_scores_and_nominee_rule():
    mu = np.array([0.0, 1.0, np.nan, 0.5, 0.5])
    var = np.array([1.0, 0.0, 1.0, -1.0, 0.25])
    sc = R.mes_ref(mu, var, [-1.0, 0.0])
    assert mpmath.isnan(sc[2]) and mpmath.isnan(sc[3]) and sc[1] == 0
    with mpmath.workdps(R.DPS):
        assert abs(sc[0] - (R.h_mp(1.0) + R.h_mp(0.0)) / 2) < mpmath.mpf(10) ** -45
        assert abs(sc[4] - (R.h_mp(3.0) + R.h_mp(1.0)) / 2) < mpmath.mpf(10) ** -45
    assert R.nominee(sc) == 2                                       # the first NaN wins
    assert R.nominee([sc[0], sc[1], sc[4], sc[0]]) == 0             # else the maximum, ties to the lowest index
    assert R.top2_gap([sc[0], sc[1], sc[4]]) == float(sc[0] - sc[4])


def test_registry_and_device_spec():
    assert "max_value_entropy_search" in Scores.registry
    cls = Scores.registry["max_value_entropy_search"]
    assert cls is Scores.max_value_entropy_search and cls.title == "bot7.scores.max_value_entropy_search"
    assert cls().config["nLevels"] == 8
    assert cls().device_spec(np.zeros((3, 1))) == {"score": "mes", "levels": 8}
    assert cls({"nLevels": 3}).device_spec() == {"score": "mes", "levels": 3}
    assert hasattr(cls, "add_to") and hasattr(cls, "compute")
