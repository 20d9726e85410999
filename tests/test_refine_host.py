"""The off-grid refinement without a GPU: the float64 reference of tests/_refine_ref.py against the 50-digit truth and against
central differences, the ladder's rules, the binding's new entries, and the harness bot's switch (off by default: the parent's
nominee sequence; the refusals by name)."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _exact as E  # noqa: E402
import _refine_ref as R  # noqa: E402


def _problem(N, d, seed, noise=1e-3):
    X, y = E.grid_data(N, d, seed)
    rng = np.random.default_rng(seed + 100)
    hyp = {"lenscale_sq": np.full(d, 0.25), "amp": 1.5, "noise": noise, "mean": 0.1}
    return X, y, hyp, rng.random((5, d))


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("N,d", [(20, 3), (70, 2)])
def test_reference_gradients_against_truth_and_central_differences(kernel, N, d):
    """post_grad64 against post_grad_truth (mpmath at N = 20, longdouble at N = 70): every quantity within 1e-9 of its scale (the
    float64 algebra's own conditioning at noise 1e-3); and the analytic gradients against central differences of the reference's
    own mean and variance, h = 1e-5: the difference's truncation and rounding leave about 1e-6 relative."""
    X, y, hyp, xs = _problem(N, d, 3)
    f = R.fit64(X, y, hyp, kernel)
    got = R.post_grad64(f, xs)
    truth = R.post_grad_truth(X, y, hyp, xs, kernel)
    gs = math.sqrt(1.0 / 0.25)
    for g, t, scale in zip(got, truth, (math.sqrt(1.5) + 0.1, 1.5, (math.sqrt(1.5) + 0.1) * gs, 1.5 * gs)):
        assert R.err_vs_truth(g, t) <= 1e-9 * scale
    h = 1e-5
    for c in range(d):
        e = np.zeros(d)
        e[c] = h
        mp_, vp, _, _ = R.post_grad64(f, xs + e)
        mm, vm, _, _ = R.post_grad64(f, xs - e)
        assert np.allclose((mp_ - mm) / (2 * h), got[2][:, c], rtol=1e-5, atol=1e-6)
        assert np.allclose((vp - vm) / (2 * h), got[3][:, c], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("kind", ["ei", "logei", "cb"])
def test_score_reference_against_50_digits_and_central_differences(kind):
    """score_value_grad64 (S = 3) against score_value_grad_mp, and its gradient against central differences of its own value along a
    random direction in (mu, sigma) space."""
    rng = np.random.default_rng(5)
    S, P, d = 3, 6, 4
    mu, var = rng.normal(size=(S, P)), rng.uniform(0.05, 1.0, (S, P))
    dmu, dvar = rng.normal(size=(S, P, d)), rng.normal(size=(S, P, d)) * 0.1
    spec = {"fmin": -0.5, "tradeoff": 0.01} if kind != "cb" else {"tradeoff": 1.7, "upper": False, "sign": -1.0}
    v, g = R.score_value_grad64(kind, mu, var, dmu, dvar, spec)
    tv, tg = R.score_value_grad_mp(kind, mu, var, dmu, dvar, spec)
    assert R.err_vs_truth(v, tv) <= 1e-13 * max(1.0, float(np.max(np.abs(v))))
    assert R.err_vs_truth(g, tg) <= 1e-12 * max(1.0, float(np.max(np.abs(g))))
    if kind == "ei":
        return   # its gradient is the exact-EI formula with A&S's Phi: a direction, not the derivative of the A&S value to 1e-7
    h = 1e-6
    for c in range(d):
        vp, _ = R.score_value_grad64(kind, mu + h * dmu[:, :, c], var + h * dvar[:, :, c], dmu, dvar, spec)
        vm, _ = R.score_value_grad64(kind, mu - h * dmu[:, :, c], var - h * dvar[:, :, c], dmu, dvar, spec)
        assert np.allclose((vp - vm) / (2 * h), g[:, c], rtol=1e-6, atol=1e-7)


def test_ladder_rules():
    lo, hi = np.zeros(3), np.array([1.0, 2.0, 1.0])
    x, g = np.array([0.5, 1.0, 0.99]), np.array([1.0, -0.25, 4.0])
    c = R.ladder_candidates(x, g, 0.25, lo, hi)
    gt = g * (hi - lo)
    r = gt / 4.0
    for k in range(4):
        want = np.minimum(np.maximum(x + ((0.25 * 4.0 ** -k) * r) * (hi - lo), lo), hi)
        assert np.array_equal(c[k], want)
    assert c[0][2] == 1.0 and c[3][2] < 1.0                      # the first rung is clipped at the face, the last is not
    assert R.ladder_candidates(x, np.zeros(3), 0.25, lo, hi) is None
    assert R.ladder_candidates(x, np.array([1.0, np.nan, 0.0]), 0.25, lo, hi) is None
    assert R.ladder_candidates(x, np.array([1.0, np.inf, 0.0]), 0.25, lo, hi) is None
    # strict improvement; ties to the lowest rung; a NaN never wins; the eta updates and the floor
    assert R.ladder_decide(1.0, 0.25, [1.0, 1.0, 1.0, 1.0]) == (-1, 1.0, 0.25 / 256.0, False)
    assert R.ladder_decide(1.0, 0.25, [2.0, 3.0, 3.0, 0.0]) == (1, 3.0, 0.25, False)
    assert R.ladder_decide(1.0, 0.25, [np.nan, 0.5, 2.0, np.nan]) == (2, 2.0, 0.0625, False)
    assert R.ladder_decide(1.0, 0.5, [5.0, 0.0, 0.0, 0.0]) == (0, 5.0, 1.0, False)
    assert R.ladder_decide(1.0, 0.25, [np.nan] * 4)[0] == -1
    assert R.ladder_decide(-np.inf, 0.25, [-np.inf] * 4)[0] == -1
    assert R.ladder_decide(1.0, 2.0 ** -33, [0.0] * 4) == (-1, 1.0, 2.0 ** -41, True)
    assert R.ladder_decide(1.0, 2.0 ** -32, [0.0] * 4) == (-1, 1.0, 2.0 ** -40, False)
    assert R.ladder_decide(1.0, 2.0 ** -39, [0.0, 0.0, 0.0, 2.0]) == (3, 2.0, 2.0 ** -43, True)


def test_refine_run_never_decreases_and_th_top():
    f = lambda xs: (-np.sum((np.atleast_2d(xs) - 0.3) ** 2, 1), -2.0 * (np.atleast_2d(xs) - 0.3))
    out = R.refine_run(f, np.array([[0.9, 0.9], [0.3, 0.3], [0.0, 1.0]]), 12, 1.0 / 16.0, 0.0, 1.0)
    assert np.all(out["val"] >= out["val0"]) and out["val"][0] > out["val0"][0]
    assert out["status"][1] & R.FLAT and not out["status"][1] & R.MOVED
    assert R.th_top([1.0, 3.0, np.nan, 3.0, 2.0], 4) == [2, 1, 3, 4]


def test_binding_has_the_new_entries():
    from bot7_amd import _lib
    for name in ("b7_refine_default_opts", "b7_eval_nominate_refine", "b7_refine_last", "b7_refine_shape", "b7_refine_trace_enable", "b7_refine_trace",
                 "b7_gp_grad_at", "b7_score_grad_compute"):
        assert name in _lib.SYMBOLS
    for name in ("eval_nominate_refine", "gp_grad_at", "score_grad_compute", "refine_last", "refine_shape", "refine_trace"):
        assert callable(getattr(_lib.Context, name))
    assert (_lib.REFINE_MAX_STARTS, _lib.REFINE_MAX_ITERS, _lib.REFINE_TRACE_WIDTH) == (16, 256, 200)


def test_bot_refine_is_off_by_default_and_off_is_the_parents_loop():
    """config.bot.refine defaults to False, and with it off a seeded run of the default experiment on oracle/hostctx.py nominates
    what it nominated before the switch existed (recorded from that commit)."""
    from harness import bots, default_regime as dr
    from oracle.hostctx import OracleContext

    class H(object):
        def __init__(self, name):
            self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1
    bot = bots.bayesopt.__new__(bots.bayesopt)
    bot.hypers = [H("a"), H("b")]
    cfg = bots.bayesopt.configure(bot, {})
    assert cfg["bot"]["refine"] is False
    on = bots.bayesopt.configure(bot, {"bot": {"refine": {"iters": 4}}})
    assert on["bot"]["refine"] == {"starts": 16, "iters": 4, "eta0": 1.0 / 16.0}
    r = dr.run(OracleContext(), budget=6, grid_size=2000)
    assert r["nominees"] == [1887, 1023, 1536, 271, 1931, 1153]


def test_bot_refusals_by_name():
    import importlib
    B = importlib.import_module("harness.bots.bayesopt")   # the module (harness.bots re-exports the class under the same name)
    base = {"bot": {"batch": 1, "refine": dict(B.REFINE_DEFAULTS)}, "score": {"type": "expected_improvement"}}
    assert B.refine_refusal(base) is None
    assert B.refine_refusal(dict(base, score={"type": "log_expected_improvement"})) is None
    assert "batch" in B.refine_refusal(dict(base, bot={"batch": 2, "refine": {}}))
    assert "sharded" in B.refine_refusal(base, sharded=True)
    assert "dngo" in B.refine_refusal(base, model_class="bot7.models.dngo")
    assert "thompson_sampling" in B.refine_refusal(dict(base, score={"type": "thompson_sampling"}))
    assert "max_value_entropy_search" in B.refine_refusal(dict(base, score={"type": "max_value_entropy_search"}))
