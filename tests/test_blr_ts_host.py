"""Thompson sampling on the Bayesian-linear head without a GPU: the transpose of the weight map at 50 digits, the references of
tests/_blr_ts_ref.py against each other, the ABI's three symbols, and the host layers' acceptance and refusals."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import _blr_ref as B
import _blr_ts_ref as R
import bot7_amd
from bot7_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["b7_blr_ts_nominate", "b7_blr_ts_last_draws", "b7_blr_paths_compute"]


@pytest.mark.parametrize("z", [1, 3, 8])
def test_the_map_is_the_inverse_transpose(z):
    """_blr_ref.exact_head gives an A = beta Z'Z + alpha I that is exact in float64; at 50 digits, with A = L L', the map
    eps -> L^-T eps has covariance L^-T L^-1 = inv(A) to 45 digits, and eps -> L^-1 eps (covariance L^-1 L^-T) does not -- except at
    z = 1, where L is a number and the two maps are the same map."""
    p = B.problem(40, z, 4)
    A, _ = B.exact_head(p.Z0, p.Y, *B.WIDE_HYP)
    Ainv, right, wrong = R.map_covariances(A, 50)
    d_right, d_wrong = R.rel_distance(right, Ainv), R.rel_distance(wrong, Ainv)
    print("z = %d: |L^-T L^-1 - inv(A)| / |inv(A)| = %.2e, |L^-1 L^-T - inv(A)| / |inv(A)| = %.2e" % (z, d_right, d_wrong))
    assert d_right < 1e-45
    if z > 1:
        assert d_wrong > 1e-10          # not to 45 digits -- nor to 10: float64 arithmetic tells the two maps apart
    else:
        assert d_wrong < 1e-45


def test_draws_depend_on_seed_path_and_component_only():
    a, b = R.eps_ref(11, 2, 50), R.eps_ref(11, 2, 256)
    assert np.array_equal(a, b[:50])
    assert not np.array_equal(a, R.eps_ref(11, 3, 50)) and not np.array_equal(a, R.eps_ref(12, 2, 50))
    # a stream of its own: none of _ts_ref's path streams (1 + j) nor its basis stream (0) gives these numbers
    for stream in range(0, 18):
        other = R.T.counter_normal(R.T.counter_key(11, stream), np.arange(50, dtype=np.uint64))
        assert not np.array_equal(a, other)
    zs = R.eps_ref(5, 0, 256)
    assert abs(zs.mean()) < 0.2 and 0.8 < zs.std() < 1.2


def test_weight_reference_and_its_bar():
    """weights_exact against 50-digit arithmetic on a LAPACK head, numpy inside its own bar, and the two wrong maps far outside."""
    import mpmath
    p = B.problem(40, 8, 4)
    A, q = B.exact_head(p.Z0, p.Y, *B.WIDE_HYP)
    _, Li, m = B.lapack_head(A, q)
    eps = R.eps_ref(3, 1, 8)
    ref = R.weights_exact(Li, m, eps)
    with mpmath.workdps(50):
        for k in range(8):
            t = mpmath.mpf(float(m[k])) + mpmath.fsum(mpmath.mpf(float(Li[i, k])) * mpmath.mpf(float(eps[i])) for i in range(k, 8))
            assert abs(mpmath.mpf(float(ref.hi[k])) + mpmath.mpf(float(ref.lo[k])) - t) <= abs(t) * mpmath.mpf(2) ** -100
    assert R.judge_weights(ref, R.weights_host(Li, m, eps)).max() <= 1.0 / 8.0 + 1e-12
    assert R.judge_weights(ref, m + np.tril(Li) @ eps).max() > 1e6          # L^-1 eps: the transpose forgotten
    assert R.judge_weights(ref, m + Li.T @ eps[::-1]).max() > 1e6


def test_path_reference_catches_a_dropped_feature_and_a_wrong_mean():
    rng = np.random.default_rng(0)
    Phi, W, means = rng.random((20, 7)), rng.normal(size=(7, 3)), [0.3, -1.1, 2.0]
    P = np.stack([means[j] + Phi @ W[:, j] for j in range(3)], axis=1)
    assert R.judge_paths(W, means, Phi, P).max() <= 1.0
    bad = P.copy()
    bad[:, 1] -= Phi[:, 6] * W[6, 1]
    assert R.judge_paths(W, means, Phi, bad)[:, 1].min() > 1e6
    assert R.judge_paths(W, [means[1], means[0], means[2]], Phi, P)[:, :2].min() > 1e6
    assert R.nominees_ref(np.array([[1.0, 0.0], [0.0, 0.0], [np.nan, -1.0]])) == [1, 2]


def test_the_three_symbols_are_declared_everywhere():
    hdr = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    lib = ctypes.CDLL(bot7_amd.lib_path())
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert re.search(r"\bint %s\s*\(" % name, cdef), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert getattr(L, name).restype is ctypes.c_int and getattr(L, name).argtypes
    assert L.b7_abi_version() == 1                                          # additive: no version change
    nargs = {name: len(re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, cdef, flags=re.S).group(1).split(",")) for name in SYMBOLS}
    assert nargs == {n: len(getattr(L, n).argtypes) for n in SYMBOLS} == {"b7_blr_ts_nominate": 15, "b7_blr_ts_last_draws": 4,
                                                                             "b7_blr_paths_compute": 8}
    for name in ("blr_ts_nominate", "blr_ts_last_draws", "blr_paths_compute"):
        assert callable(getattr(_lib.Context, name))
    assert callable(bot7_amd.models.dngo.ts_nominate)
    # the header's "Not built" line of b7_ts_nominate points at the new entry
    assert "b7_blr_ts_nominate below" in hdr and "Not built: sharded grids and groups, more than one response column" in hdr
    shim = open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read()
    assert "bot7.models.dngo_hip" in shim and "ts_nominate" in open(os.path.join(ROOT, "lua", "models_dngo_hip.lua")).read()


class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _net(d=3, width=16):
    rng = np.random.default_rng(1)
    return {"weights": [rng.normal(size=(width, d)), rng.normal(size=(width, width)), rng.normal(size=(width, width))],
            "biases": [rng.normal(size=width) for _ in range(3)], "activation": "Tanh"}


def test_the_bot_accepts_dngo_with_thompson_sampling_and_still_refuses_the_rest():
    from harness import benchmarks, bots
    Bm = importlib.import_module("harness.bots.bayesopt")
    cfg = {"bot": {"verbose": 0, "budget": 4, "nInitial": 2, "nSamples": 1, "seed": 1, "batch": 2},
           "grid": {"type": "random", "size": 32, "dims": 3}, "score": {"type": "thompson_sampling"},
           "model": {"type": "dngo", "network": _net()}}
    model = bot7_amd.models.dngo(cfg["model"], context=object())            # no device is touched at construction
    bot = bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(3)], cfg,
                        cache={"candidates": np.random.default_rng(0).random((32, 3)), "model": model})
    assert bot._thompson() and bot.model.class_() == "bot7.models.dngo" and bot.config["bot"]["batch"] == 2
    src = open(os.path.join(ROOT, "harness", "bots", "bayesopt.py")).read()
    body = src.split("def _ts_nominate(self, q, cand):")[1].split("\n    def ")[0]
    assert 'model.class_() == "bot7.models.dngo"' in body and 'model.class_() != "bot7.models.dngo"' not in body
    assert 'not hasattr(cand, "commit")' in body                            # the sharded-grid assertion stays
    # what stays refused for the dngo model, by the messages the existing host tests pin
    dn = "bot7.models.dngo"
    kg = {"bot": {"batch": 1, "refine": False, "constraints": None}, "score": {"type": "knowledge_gradient", "discretisation": "thompson"}}
    assert Bm.kg_refusal(kg, dn) == "knowledge_gradient with the dngo model: the Bayesian-linear head has no posterior-covariance kernel"
    ts = {"bot": {"batch": 1, "refine": {"starts": 4}, "constraints": None, "objectives": None, "trust_region": None},
          "score": {"type": "thompson_sampling"}}
    assert Bm.refine_refusal(ts, dn) is not None
    ei = {"bot": {"batch": 1, "refine": {"starts": 4}}, "score": {"type": "expected_improvement"}}
    assert Bm.refine_refusal(ei, dn) == "config.bot.refine with the dngo model: the Bayesian-linear head has no gradient kernels"
    con = {"bot": {"batch": 1, "refine": False, "constraints": [{"threshold": 0.0, "model": {"type": "gp_regressor"}}]},
           "score": {"type": "expected_improvement"}}
    assert Bm.constraint_refusal(con, dn) == "config.bot.constraints with the dngo model: the Bayesian-linear head has no feasibility weight"
    text = open(os.path.join(ROOT, "harness", "bots", "bayesopt.py")).read()
    for msg in ("config.bot.objectives with the dngo model: the Bayesian-linear head keeps no posterior for a second objective",
                "config.bot.objectives with the dngo model: the Bayesian-linear head keeps no posterior for further objectives",
                "config.bot.trust_region with the dngo model: the box is shaped by a GP's ARD lengthscales"):
        assert msg in text


def test_score_dispatches_on_the_model_class():
    calls = []

    class FakeDngo(object):
        def class_(self):
            return "bot7.models.dngo"

        def ts_nominate(self, X, Y, cand, hyps, q, seed):
            calls.append(("dngo", q, seed, len(hyps)))
            return np.zeros(q), np.arange(1, q + 1)

    class FakeCtx(object):
        def ts_nominate(self, hyps, q, n_features, seed):
            calls.append(("gp", q, seed, n_features))
            return np.zeros(q), np.arange(1, q + 1)

    score = bot7_amd.scores.registry["thompson_sampling"]({"nFeatures": 64})
    assert list(score.nominate(FakeCtx(), [{}], 2, 9)) == [1, 2]
    assert list(score.nominate(FakeCtx(), [{"alpha": 1.0}], 3, 7, model=FakeDngo(), observed=None, responses=None, candidates=None)) == [1, 2, 3]
    assert calls == [("gp", 2, 9, 64), ("dngo", 3, 7, 1)]
