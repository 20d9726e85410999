"""The knowledge gradient without a GPU: the references of tests/_kg_ref.py against each other, the ABI's three symbols and
constant, the score's registry entry, the bot's refusals and the Lua shims' static checks."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import bot7_amd
import bot7_amd.scores as Scores
from bot7_amd import _lib

import _kg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()


# ---- the references ----------------------------------------------------------------------------------------------------------------
def random_line_sets():
    """40 sets of lines, L = 2 .. 17: duplicate slopes, values rounded to one decimal (three lines then often meet in a point),
    slope scales from 1e-3 to 5."""
    rng = np.random.default_rng(1)
    sets = []
    for k in range(40):
        L = 2 + k % 16
        a, b = rng.standard_normal(L), rng.standard_normal(L) * float(rng.choice([1e-3, 0.1, 1.0, 5.0]))
        if k % 3 == 0:
            a, b = np.round(a, 1), np.round(b, 1)
        if k % 4 == 1:
            b[L // 2] = b[0]
        sets.append((a, b))
    return sets


def test_numpy_form_against_the_sort_and_prune_algorithm():
    """kg_numpy (the library's O(L^2) form in float64) against kg_mp (sort and prune, 50 digits).  Bar, per set: a term
    (b_i - b_next) f(-|z|) carries a relative error of about (1 + z^2)^2 units of 2^-53 -- the argument z^2 / 2 of exp is rounded, so
    phi(z) is off by z^2 / 2 units relative, and phi(z) - |z| Phi(-|z|) then cancels to ~1/z^2 of its operands (erfc and exp through
    float64 cannot do better; z's own three roundings enter through f'(z) z / f(z) ~ z^2 only) -- so the sum is held to
    32 x 2^-53 x sum_i term_i (1 + z_i^2)^2.  Never negative.  Measured here: worst 0.05 of the bar."""
    worst = 0.0
    for a, b in random_line_sets():
        got, cond = R.kg_numpy(a[None, :], b[None, :], want_cond=True)
        ref = R.kg_mp(a, b)
        err = abs(float(mpmath.mpf(float(got[0])) - ref))
        bar = 32.0 * R.EPS * float(cond[0])
        worst = max(worst, err / bar if bar > 0 else (0.0 if err == 0 else np.inf))
        assert got[0] >= 0.0 and err <= bar, (len(a), got[0], float(ref), err, bar)
    print("numpy O(L^2) form against sort-and-prune at 50 digits: worst error / bar %.3g" % worst)


def test_reference_against_numerical_integration():
    """kg_mp against E[min] by quadrature (mpmath, 30 digits) on five of the sets: the positive-term identity itself."""
    for a, b in random_line_sets()[::8]:
        with mpmath.workdps(30):
            la, lb = [mpmath.mpf(float(v)) for v in a], [mpmath.mpf(float(v)) for v in b]
            cuts = sorted({(la[j] - la[i]) / (lb[i] - lb[j]) for i in range(len(a)) for j in range(i) if lb[i] != lb[j]})
            cuts = [c for c in cuts if abs(c) < 30]
            emin = mpmath.quad(lambda z: min(x + s * z for x, s in zip(la, lb)) * mpmath.npdf(z), [-40] + cuts + [40])
            want = min(la) - emin
            assert abs(R.kg_mp(a, b) - want) <= mpmath.mpf(10) ** -20 * (1 + abs(want))


def test_envelope_edge_cases_of_the_numpy_form():
    a = np.array([[0.3, -0.2, 1.0]])
    assert R.kg_numpy(a[:, :1], np.array([[0.7]]))[0] == 0.0                       # one line
    assert R.kg_numpy(a, np.zeros((1, 3)))[0] == 0.0                                # all slopes zero
    assert R.kg_numpy(a, np.array([[np.nan, 0.0, 0.0]]))[0] == 0.0                  # no own line
    two = R.kg_numpy(np.array([[0.0, 0.0]]), np.array([[1.0, -1.0]]))[0]            # E[-|Z|] = -sqrt(2/pi)
    assert abs(two - np.sqrt(2.0 / np.pi)) < 4 * R.EPS
    cases = R.envelope_cases()
    assert set(len(v[0]) for v in cases.values()) == {65} and (R.kg_numpy(*cases["all slopes zero"]) == 0.0).all()
    al, b = cases["three lines through one point"]
    y = al[:, :3] + b[:, :3] * ((al[:, 1] - al[:, 0]) / (b[:, 0] - b[:, 1]))[:, None]
    assert (y[:, 0] == y[:, 1]).all() and (y[:, 0] == y[:, 2]).all()                # concurrent exactly


def test_posterior_covariance_reference():
    """posterior_ld: the covariance against a row of A that is the query itself is the variance; at an observed point with tiny
    noise it vanishes; long double against numpy float64 to 1e-9."""
    rng = np.random.default_rng(4)
    X, Xs = rng.random((20, 3)), rng.random((30, 3))
    Xs[5] = X[2]
    y = np.sin(3.0 * X.sum(axis=1))
    hyp = {"lenscale_sq": np.full(3, 0.4), "amp": 1.3, "noise": 1e-9, "mean": 0.1}
    for kernel in ("ardse", "ardmatern52"):
        mu, var, C = R.posterior_ld(X, y, Xs, hyp, kernel, [0, 5, 7])
        assert abs(float(C[0, 0] - var[0])) < 1e-15 and abs(float(C[7, 2] - var[7])) < 1e-15 and abs(float(C[3, 1] - C[5, 0] * 0)) < 1e-6
        assert abs(float(var[5])) < 1e-6 and np.abs(np.asarray(C[5], dtype=float)).max() < 1e-6
        K = np.asarray(R.cov_ld(X, X, hyp["lenscale_sq"], hyp["amp"], kernel), dtype=float) + hyp["noise"] * np.eye(20)
        Ks = np.asarray(R.cov_ld(Xs, X, hyp["lenscale_sq"], hyp["amp"], kernel), dtype=float)
        Ka = np.asarray(R.cov_ld(Xs, Xs[[0, 5, 7]], hyp["lenscale_sq"], hyp["amp"], kernel), dtype=float)
        want = Ka - Ks @ np.linalg.solve(K, Ks[[0, 5, 7]].T)
        assert np.abs(np.asarray(C, dtype=float) - want).max() < 1e-6
    rows0, alpha, slopes, mu = R.slopes_ref(X, y, Xs, [hyp, dict(hyp, amp=2.0)], "ardse", n=4)
    assert slopes.shape == (2, 30, 5) and np.isnan(slopes[:, rows0, 0]).all() and np.isfinite(np.delete(slopes[0, :, 0], rows0)).all()
    assert list(rows0) == list(np.argsort(mu.mean(axis=0), kind="stable")[:4])
    v = R.values_ref(alpha, slopes, mu)
    assert v.shape == (2, 30) and (v >= 0).all() and R.nominee_ref(np.array([0.0, 2.0, np.nan, 3.0])) == 2


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_symbols():
    lib = ctypes.CDLL(bot7_amd.lib_path())
    for name in ("b7_kg_nominate", "b7_kg_last", "b7_kg_compute", "b7_kg_trace_enable"):
        assert re.search(r"\bint %s\(b7_ctx \*ctx" % name, HEADER), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"int b7_kg_nominate\(b7_ctx \*ctx, int S, const b7_hyp \*hyps, int n, const int64_t \*rows1", HEADER)
    assert re.search(r"int b7_kg_compute\(b7_ctx \*ctx, int64_t M1, int L, const double \*alpha", HEADER)


def test_max_points_constant():
    assert re.search(r"^#define B7_KG_MAX_POINTS 16$", HEADER, flags=re.M)
    assert _lib.KG_MAX_POINTS == 16
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    assert "M.KG_MAX_POINTS = 16" in lua


# ---- the host layers -----------------------------------------------------------------------------------------------------------------
def test_registry_and_the_refusal_of_compute():
    assert Scores.registry["knowledge_gradient"] is Scores.knowledge_gradient
    cls = Scores.knowledge_gradient
    assert cls.title == "bot7.scores.knowledge_gradient"
    cfg = cls().config
    assert cfg["points"] == 16 and cfg["discretisation"] == "mean" and cls({"points": 5}).config["points"] == 5
    assert not hasattr(cls, "device_spec")
    with pytest.raises(NotImplementedError, match="not a per-point score"):
        cls().compute(np.zeros(3), np.ones(3))
    with pytest.raises(NotImplementedError, match="not a per-point score"):
        cls().add_to(None)


def _config(**bot):
    return {"bot": dict({"batch": 1, "refine": False, "constraints": None}, **bot), "score": {"type": "knowledge_gradient"}}


def test_bot_refusal_messages():
    import importlib
    B = importlib.import_module("harness.bots.bayesopt")   # (harness.bots.bayesopt the attribute is the class)
    assert B.kg_refusal(_config()) is None
    assert B.kg_refusal(_config(batch=2)) == "knowledge_gradient with config.bot.batch > 1: knowledge-gradient batches are not built"
    assert B.kg_refusal(_config(refine={"starts": 4})) == \
        "config.bot.refine with knowledge_gradient: refinement of a knowledge-gradient nominee is not built"
    assert B.refine_refusal(_config(refine={"starts": 4})) == B.kg_refusal(_config(refine={"starts": 4}))
    con = [{"threshold": 0.0, "model": {"type": "gp_regressor"}}]
    assert B.kg_refusal(_config(constraints=con)) == \
        "config.bot.constraints with knowledge_gradient: the knowledge gradient has no feasibility weight"
    assert B.constraint_refusal(_config(constraints=con)) == B.kg_refusal(_config(constraints=con))
    assert B.kg_refusal(_config(), sharded=True) == \
        "knowledge_gradient over sharded candidates: the knowledge gradient over a sharded grid is not built"
    assert B.kg_refusal(_config(), "bot7.models.dngo") == \
        "knowledge_gradient with the dngo model: the Bayesian-linear head has no posterior-covariance kernel"
    bad = _config()
    bad["score"]["discretisation"] = "sobol"
    assert "config.score.discretisation = 'sobol'" in B.kg_refusal(bad)
    # no existing message changed
    ei = {"bot": {"batch": 2, "refine": True}, "score": {"type": "expected_improvement"}}
    assert B.refine_refusal(ei) == "config.bot.refine with config.bot.batch > 1: refinement of a batch is not built"
    ts = {"bot": {"batch": 1, "refine": True}, "score": {"type": "thompson_sampling"}}
    assert B.refine_refusal(ts) == "config.bot.refine with thompson_sampling: a sample path is not a per-point score"


def test_lua_shims_carry_the_policy():
    import test_lua_shims as T
    T.test_cdef_block_is_the_header()
    T.test_every_ffi_call_matches_a_declared_prototype()
    T.test_lua_blocks_and_brackets_balance()
    bt = T.strip_lua_comments(open(os.path.join(T.LUA, "bots_bayesopt_hip.lua")).read())
    sc = T.strip_lua_comments(open(os.path.join(T.LUA, "scores_hip.lua")).read())
    assert "local function nominate_kg(self, candidates)" in bt
    assert re.search(r"b7_kg_nominate\(hip\.ctx, S, hyps, n, rows, v, i, jit, info\)", bt)
    assert "'bot7.scores.knowledge_gradient_hip' then return nominate_kg(self, candidates)" in bt
    assert "torch.class('bot7.scores.knowledge_gradient_hip', 'bot7.scores.abstract')" in sc and "S.knowledge_gradient = KG" in sc
    assert ("b7_kg_nominate", 9) in T.calls(bt)
