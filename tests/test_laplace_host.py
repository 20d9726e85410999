"""The probit GP classifier by Laplace's method, on the host: the float64 restatement of the device's rule (tests/_laplace_ref.py)
against the 50-digit solution of the mode equation, the identities the FitSet reuse rests on, the float64 probit pieces against 50
digits, the entry points in header / Lua cdef / Python SYMBOLS, the model class, the bot's binary-constraint branch on stub contexts
and the Lua mirror's static checks.  No GPU needed; the device is held by tests/test_gpu_laplace.py."""
import math
import os
import re
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib

import _laplace_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_clf_nll_batch", "b7_clf_fit_hyp", "b7_clf_mode_get", "b7_clf_eval_logfeas", "b7_probit_compute")
NAN = float("nan")


# ---- 1. the restatement against 50 digits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.host_cases(), ids=lambda c: "N%d-d%d-amp%g-mean%g-%s-%s" % c)
def test_restatement_against_50_digits(case):
    """The float64 rule converges within the cap on every case, and its own error against the 50-digit mode -- in f^, a, W, the
    latent mean and variance at 8 rows, and nll -- is recorded: these are the yardsticks of the GPU tests.  What is asserted of the
    error is only that it is an error of rounding: B's condition number is at most 1 + N amp, so eps N amp of the quantity's scale is
    what rounding can cost; the bound is 1e-11 max(1, amp), some 2000 times that at N = 24."""
    sol = R.solved_case(case)
    fit = sol["fit"]
    print("%s: %d iterations, at most %d halvings; own error %s" % (case, fit["iters"], max(fit["halvings"]),
                                                                   {q: "%.2g" % sol["err"][q] for q in sol["err"]}))
    assert fit["converged"] and 1 <= fit["iters"] <= 16 and max(fit["halvings"]) <= 1, (fit["iters"], fit["halvings"])
    for q, e in sol["err"].items():
        assert e <= 1e-11 * max(1.0, sol["amp"]) * max(1.0, sol["scale"][q]), (q, e)


def test_longdouble_rule_agrees_with_50_digits():
    """The truth of the GPU tests above N = 24 is the same rule in numpy.longdouble with a hand-written Cholesky: at N = 24 it is held
    to the 50-digit mode itself, far inside the float64 restatement's own error."""
    case = (24, 6, 100.0, 0.0, R.SE, "mixed")
    sol = R.solved_case(case)
    LD = np.longdouble
    tr = R.laplace_fit(R.cov(sol["X"], sol["X"], sol["ls"], sol["amp"], sol["kern"], LD), sol["v"], sol["mean"], LD)
    mu, var = R.posterior(R.cov(sol["Xs"], sol["X"], sol["ls"], sol["amp"], sol["kern"], LD), sol["amp"], sol["mean"], tr)
    got = {"f": tr["f"], "a": tr["a"], "W": tr["W"], "mu": mu, "var": var, "nll": np.array([tr["nll"]])}
    assert tr["converged"]
    for q in got:
        truth = sol["truth"][q].astype(LD) + sol["truth_lo"][q].astype(LD)
        err = float(np.max(np.abs(got[q] - truth)))
        assert err <= sol["err"][q] / 64.0 + 4.0 * float(np.finfo(LD).eps) * sol["scale"][q], (q, err, sol["err"][q])


# ---- 2. identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.host_cases() if c[0] >= 12 and c[2] <= 100.0], ids=lambda c: "N%d-d%d-amp%g-mean%g-%s-%s" % c)
def test_identities(case):
    """amp - |L^-1 W^1/2 k*|^2 == k** - k*'(K + W^-1)^-1 k* where W > 0 (the regressor's form with Linv := L^-1 W^1/2); a == g(f^) at
    convergence; W >= 0; psi non-decreasing over the accepted steps."""
    sol = R.solved_case(case)
    fit, X, Xs, ls, amp, mean, kern = sol["fit"], sol["X"], sol["Xs"], sol["ls"], sol["amp"], sol["mean"], sol["kern"]
    assert (fit["W"] >= 0.0).all() and (fit["W"] <= 1.0 + 1e-15).all()
    assert np.max(np.abs(fit["a"] - fit["g"])) <= 1e-9 * max(1.0, np.max(np.abs(fit["a"])))
    tr = np.array(fit["psi_trace"], dtype=np.float64)
    assert (np.diff(tr) >= -1e-12 * np.maximum(1.0, np.abs(tr[1:]))).all(), tr
    assert (fit["W"] > 0.0).all()
    K, Ks = R.cov(X, X, ls, amp, kern), R.cov(Xs, X, ls, amp, kern)
    _, var = R.posterior(Ks, amp, mean, fit)
    other = amp - np.einsum("ij,ij->i", Ks, np.linalg.solve(K + np.diag(1.0 / fit["W"]), Ks.T).T)
    assert np.max(np.abs(var - other)) <= 1e-9 * amp, np.max(np.abs(var - other))
    assert (var > 0.0).all() and (var <= amp * (1.0 + 1e-12)).all()


# ---- 3. the float64 probit pieces ---------------------------------------------------------------------------------------------------
def test_probit_pieces_against_50_digits():
    """log Phi, phi/Phi and W as the device writes them, in float64 with scipy's erfc / erfcx, over z in [-1e6, 40]: within
    1e-13 max(1, |ref|) of 50 digits -- across the switch of W to the continued fraction at z = -6 and the three branches of log Phi."""
    rng = np.random.default_rng(7)
    z = np.concatenate([-np.exp(rng.uniform(0.0, math.log(1e6), 300)), rng.uniform(-40.0, 40.0, 500), rng.uniform(-7.0, -5.0, 100),
                        [-1e6, -6.0, np.nextafter(-6.0, 0.0), np.nextafter(-6.0, -7.0), -1.0, np.nextafter(-1.0, 0.0), 0.0, -0.0, 40.0, 37.5]])
    got = R.pieces(z)
    worst = [0.0, 0.0, 0.0]
    with mpmath.workdps(R.DPS):
        for i, zi in enumerate(z):
            ref = R.pieces_mp(float(zi))
            for k in range(3):
                worst[k] = max(worst[k], float(abs(mpmath.mpf(float(got[k][i])) - ref[k]) / max(1, abs(ref[k]))))
    print("float64 probit pieces: worst scaled error log Phi %.3g, phi/Phi %.3g, W %.3g" % tuple(worst))
    assert max(worst) <= 1e-13, worst
    assert (got[2] >= 0.0).all() and (got[2] <= 1.0 + 1e-15).all()
    # the plain product loses what the continued fraction keeps: at z = -1e4 it is off by far more than the bar
    zz = np.array([-1e4])
    rho = R.ratio(zz)
    with mpmath.workdps(R.DPS):
        ref = float(R.pieces_mp(-1e4)[2])
    assert abs(float(rho[0] * (rho[0] + zz[0])) - ref) > 1e-10 > 1e-13 >= abs(float(R.wfun(zz, rho)[0]) - ref)


# ---- 4. the surface ----------------------------------------------------------------------------------------------------------------
def test_header_cdef_and_symbols_carry_the_entries():
    decls = {re.search(r"\b(b7_[a-z0-9_]+)\s*\(", d).group(1): d for d in gen_lua_cdef.cdef_lines(HEADER)
             if re.match(r"^(?!typedef).*\bb7_[a-z0-9_]+\s*\(", d)}
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    block = lua.split(gen_lua_cdef.BEGIN_CDEF)[1].split(gen_lua_cdef.END_CDEF)[0].splitlines()
    for name in NEW:
        assert name in decls, "include/bot7hip.h does not declare %s" % name
        assert decls[name] in block, "lua/bot7hip_ffi.lua does not carry the header's %s" % name
        assert name in _lib.SYMBOLS
    assert gen_lua_cdef.defines(HEADER)["B7_ABI_VERSION"] == 1      # additive: the version stays
    i = HEADER.index("int b7_clf_nll_batch(")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    for word in ("No counterpart", "Gelbart", "Rasmussen", "VIOLATED", "B7_ERR_INVALID", "B7_ERR_UNSUPPORTED", "B7_ERR_STATE", "N <= 128",
                 "b7_feas_add_acc", "var_with_noise"):
        assert word in comment, word
    for meth in ("clf_nll_batch", "clf_fit_hyp", "clf_mode_get", "clf_eval_logfeas", "probit_compute"):
        assert callable(getattr(bot7_amd.Context, meth)), meth
    from bot7_amd import build
    assert "laplace.hip" in build.SOURCES and any(h.endswith("probit_math.h") for h in build.HEADERS)


def test_model_class():
    from bot7_amd import models
    assert models.registry["gp_classifier"] is models.gp_classifier
    with pytest.raises(NotImplementedError) as e:
        models.gp_classifier({"sampler": "slice_device"})
    assert "slice_device" in str(e.value) and "gp_classifier" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        models.gp_classifier({"chains": 4})
    assert "chains" in str(e.value)

    log = []

    class Ctx(object):
        fit_token, grid_version = 0, 0

        def gp_set_kernel(self, k):
            log.append(("kernel", k))

        def gp_set_data(self, X, Y):
            self.fit_token += 1
            log.append(("data", np.asarray(Y).copy()))

        def clf_nll_batch(self, hyps, want_info=False):
            log.append(("nll", hyps[0]))
            return np.array([3.5]), np.array([4], dtype=np.int32), np.array([0], dtype=np.int32)

        def clf_fit_hyp(self, ls, amp, noise, mean):
            log.append(("fit", amp, noise, mean))
            return {"nll": 3.5, "iters": 4, "info": 0}

        def gp_predict_at(self, X1):
            return np.array([[0.0], [1.0], [-2.0]]), np.array([0.0, 3.0, 0.0])

    m = models.gp_classifier({"kernel": "ardmatern52"}, context=Ctx())
    X, v = np.random.default_rng(0).random((5, 2)), np.array([0.0, 1.0, 1.0, 0.0, 1.0])
    h = m.init(X, v)
    assert h["amp"] == 1.0 and h["noise"] == 0.0 and list(h["lenscale_sq"]) == [0.25, 0.25]
    from statistics import NormalDist
    assert h["mean"] == NormalDist().inv_cdf(4.0 / 7.0)
    vec = m.sample_hypers(X, v)
    assert m.parse_hypers(vec)["mean"] == h["mean"] and vec.size == 5           # the regressor's layout: noise carried as 0
    th = m._to_theta(h)
    assert th.size == 4 and m._from_theta(th)["noise"] == 0.0                  # the sampler walks [log lenscale_sq, log amp, mean]
    lo, hi = m._bounds_compute(X, v.reshape(-1, 1))
    assert lo.size == hi.size == 4 and (lo < th).all() and (th < hi).all()
    assert m.log_posterior(th, X, v) == -3.5 and m.log_posterior(hi + 1.0, X, v) == -np.inf
    assert float(m.nll(X, v)[0]) == 3.5
    out = m.predict(X, v, np.zeros((3, 2)))
    assert ("kernel", "ardmatern52") in log and ("fit", 1.0, 0.0, h["mean"]) in log
    want = [0.5, 0.5 * math.erfc(-0.5 * math.sqrt(0.5)), 0.5 * math.erfc(2.0 * math.sqrt(0.5))]   # Phi(mu / sqrt(var + 1))
    assert np.allclose(out["mean"][:, 0], want, rtol=0, atol=1e-15) and list(out["latent"][:, 0]) == [0.0, 1.0, -2.0]
    assert [np.array_equal(e[1][:, 0], v) for e in log if e[0] == "data"] == [True]      # the labels went up once
    with pytest.raises(NotImplementedError):
        m.fantasize(2, X, v, X[:1])
    with pytest.raises(NotImplementedError):
        m.sample_hypers(X, np.stack([v, v], axis=1))


def test_hidden_constraint_toy():
    from harness import benchmarks as B
    X = np.random.default_rng(0).random((2000, 2))
    full, hid = B.gardner1(X), B.gardner1_hidden(X)
    assert B.registry["gardner1_hidden"] is B.gardner1_hidden and hid.shape == (2000, 2) and B.gardner1_hidden(X[0]).shape == (1, 2)
    bad = full[:, 1] > B.GARDNER1_THRESHOLD
    assert set(np.unique(hid[:, 1])) == {0.0, 1.0} and np.array_equal(hid[:, 1] == 1.0, bad) and 0.1 < bad.mean() < 0.6
    assert np.isnan(hid[bad, 0]).all() and np.array_equal(hid[~bad, 0], full[~bad, 0])


# ---- 5. the bot's binary branch on stub contexts -----------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401  (the package re-exports the class under the module's name)
    return sys.modules["harness.bots.bayesopt"]


def _cfg(cons=None, **bot):
    cons = cons or [{"threshold": 0.5, "binary": True, "model": {"type": "gp_classifier", "sample": True}}]
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 3, "constraints": cons}, **bot),
            "grid": {"dims": 2}, "score": {"type": "log_expected_improvement"}}


def _stubs(log):
    class Ctx(object):
        def __init__(self, name, device_id=0):
            self.name, self.device_id, self.grid_version = name, device_id, 0

        def grid_upload(self, X):
            self.grid_version += 1
            log.append((self.name, "grid_upload", np.asarray(X).shape))

        def eval_nominate(self, hyps, **kw):
            log.append((self.name, "eval_nominate", len(hyps), kw["score"], list(kw["fmin"]), kw["tradeoff"]))
            return 0.0, 1

        def clf_eval_logfeas(self, hyps):
            log.append((self.name, "clf_eval_logfeas", len(hyps)))
            return 0.0, 1

        def feas_reset(self):
            log.append((self.name, "feas_reset"))

        def feas_add_acc(self, src):
            log.append((self.name, "feas_add_acc", src.name))

        def feas_nominate(self):
            log.append((self.name, "feas_nominate"))
            return -0.1, 2

        def eval_nominate_feasible(self, hyps, **kw):
            log.append((self.name, "eval_nominate_feasible", len(hyps), kw["score"], list(kw["fmin"])))
            return -1.0, 3

    class Model(object):
        def __init__(self, ctx):
            self.ctx, self.n, self.inits = ctx, 0, []

        def class_(self):
            return "bot7.models.gp_regressor"

        def init(self, X, Y):
            self.inits.append((np.asarray(X).copy(), np.asarray(Y).copy()))

        def sample_hypers(self, X, Y, *a):
            assert np.asarray(Y).shape == (len(X), 1)
            self.last_X, self.last_Y = np.asarray(X).copy(), np.asarray(Y).copy()
            self.n += 1
            return np.array([1.0, 1.0, 1.0, 0.1, 0.0])

        def parse_hypers(self, v):
            return {"lenscale_sq": v[:2], "amp": v[2], "noise": v[3], "mean": v[4]}

        def stage(self, X, Y, grid):
            log.append((self.ctx.name, "stage", np.asarray(Y).copy()))

        def _is_resident(self, X1):
            return False

    return Ctx, Model


def test_bot_binary_constraint_call_order_and_rows():
    """Which calls, in which order; which rows reach which model: NaN-objective rows leave the objective's data only."""
    Bz = _bot_module()
    log = []
    Ctx, Model = _stubs(log)
    resp = np.array([[1.0, 0.0], [NAN, 1.0], [-2.0, 0.0], [NAN, 1.0], [0.8, 0.0]])
    assert list(Bz.objective_rows(resp[:, :1], [{"binary": True}])) == [True, False, True, False, True]
    assert Bz.objective_rows(resp[:, :1], [{"threshold": 0.5}]).all()                    # without a binary constraint: every row, as ever
    assert list(Bz.feasible_rows(resp, [0.5])) == [True, False, True, False, True] and list(Bz.best_feasible_fmin(resp, [0.5])) == [-2.0]
    cand = np.random.default_rng(3).random((16, 2))
    bot = Bz.bayesopt(None, [], _cfg(), {"model": Model(Ctx("obj")), "candidates": cand})
    con_cfg = bot.config["bot"]["constraints"][0]
    assert con_cfg["binary"] is True and con_cfg["model"]["type"] == "gp_classifier" and con_cfg["threshold"] == 0.5
    assert Bz.bayesopt(None, [], _cfg([{"threshold": 0.5, "binary": True}]), {"model": Model(Ctx("o")), "candidates": cand}
                       ).config["bot"]["constraints"][0]["model"]["type"] == "gp_classifier"   # the default model of a binary constraint
    con_model = Model(Ctx("con"))
    bot.constraints = [{"threshold": 0.5, "ctx": con_model.ctx, "grid": None, "binary": True, "model": con_model}]
    bot.observed, bot.nTrials, bot.responses = np.random.default_rng(4).random((5, 2)), 5, resp
    idx = bot.nominate_constrained()
    names = [e[:2] for e in log]
    assert ("con", "eval_nominate") not in names and log[names.index(("con", "clf_eval_logfeas"))][2] == 3
    assert names.index(("con", "stage")) < names.index(("con", "clf_eval_logfeas")) < names.index(("obj", "stage")) \
        < names.index(("obj", "feas_reset")) < names.index(("obj", "feas_add_acc")) < len(names) - 1
    assert log[-1] == ("obj", "eval_nominate_feasible", 3, "logei", [-2.0]) and idx == 3
    # the classifier sees every row's label; the objective's model only the rows with a finite objective, X and Y alike
    assert np.array_equal(con_model.last_Y[:, 0], resp[:, 1]) and con_model.last_X.shape == (5, 2)
    assert list(bot.model.last_Y[:, 0]) == [1.0, -2.0, 0.8] and np.array_equal(bot.model.last_X, bot.observed[[0, 2, 4]])
    staged = [e[2] for e in log if e[:2] == ("obj", "stage")][0]
    assert list(staged[:, 0]) == [1.0, -2.0, 0.8] and np.isfinite(staged).all()
    assert list(bot.last_constrained["objective_rows"]) == [True, False, True, False, True]
    # no run has returned an objective yet: feasibility alone, the objective's model is not touched
    del log[:]
    n0 = bot.model.n
    bot.responses = np.array([[NAN, 1.0]] * 5)
    assert bot.nominate_constrained() == 2 and log[-1] == ("obj", "feas_nominate") and bot.model.n == n0
    assert ("obj", "stage") not in [e[:2] for e in log] and ("obj", "grid_upload") in [e[:2] for e in log]
    # a regression constraint beside it is served as ever, and the rows are filtered all the same
    del log[:]
    reg_model = Model(Ctx("reg"))
    bot.config["bot"]["constraints"] = [con_cfg, {"threshold": 0.25, "model": Bz.bayesopt._model_defaults(None, 3)}]
    bot.constraints.append({"threshold": 0.25, "ctx": reg_model.ctx, "grid": None, "binary": False, "model": reg_model})
    bot.responses = np.column_stack([resp, [0.1, 0.9, 0.2, 0.3, 0.9]])
    bot.nominate_constrained()
    names = [e[:2] for e in log]
    assert log[names.index(("reg", "eval_nominate"))][2:] == (3, "logpi", [0.25], 0.0) and ("con", "clf_eval_logfeas") in names
    assert [e[2] for e in log if e[1] == "feas_add_acc"] == ["con", "reg"] and log[-1][-1] == [-2.0]
    assert list(bot.model.last_Y[:, 0]) == [1.0, -2.0, 0.8] and reg_model.last_Y.shape == (5, 1)


def test_bot_initialises_the_objective_on_finite_rows():
    Bz = _bot_module()
    log = []
    Ctx, Model = _stubs(log)
    rows = iter([[NAN, 1.0], [0.5, 0.0], [NAN, 1.0]])
    bot = Bz.bayesopt(lambda x: np.array(next(rows)), [], _cfg(), {"model": Model(Ctx("obj")), "candidates": np.random.default_rng(1).random((8, 2))})
    con_model = Model(Ctx("con"))
    bot.constraints = [{"threshold": 0.5, "ctx": con_model.ctx, "grid": None, "binary": True, "model": con_model}]
    for _ in range(3):
        bot.run_trial()
    assert len(bot.model.inits) == 1 and list(bot.model.inits[0][1][:, 0]) == [0.5] and bot.model.inits[0][0].shape == (1, 2)
    assert len(con_model.inits) == 1 and list(con_model.inits[0][1][:, 0]) == [1.0, 0.0, 1.0]
    for y in ([NAN, 1.0], [0.5, 0.0], [NAN, 1.0], [0.7, 0.0]):                         # the best FEASIBLE trial; NaN rows never are
        bot.update_best(np.zeros(2), y)
    assert float(np.ravel(bot.best["y"])[0]) == 0.5


def test_bot_refusals_pinned_and_new():
    """Every refusal the constrained bot already made keeps its text and its trigger; the new ones are made by name."""
    Bz = _bot_module()
    base = Bz.bayesopt(None, [], _cfg(), {"model": object(), "candidates": np.zeros((4, 2))}).config
    assert Bz.constraint_refusal(base) is None
    pinned = [(dict(base, bot=dict(base["bot"], batch=2)), {}, "config.bot.constraints with config.bot.batch > 1: feasibility-weighted believer batches are not built"),
              (dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "config.bot.constraints with config.bot.refine: refinement of a constrained nominee is not built"),
              (base, {"sharded": True}, "config.bot.constraints over sharded candidates: constrained nomination over a sharded grid is not built"),
              (base, {"model_class": "bot7.models.dngo"}, "config.bot.constraints with the dngo model: the Bayesian-linear head has no feasibility weight"),
              (dict(base, score={"type": "thompson_sampling"}), {}, "config.bot.constraints with thompson_sampling: a sample path has no feasibility weight"),
              (dict(base, score={"type": "confidence_bound"}), {}, "config.bot.constraints with confidence_bound: a signed score has no product form with a feasibility weight"),
              (dict(base, score={"type": "max_value_entropy_search"}), {}, "config.bot.constraints with max_value_entropy_search: the score has no feasibility weight")]
    for cfg, kw, text in pinned:
        assert (Bz.constraint_refusal(cfg, **kw) or "").startswith(text), (text, Bz.constraint_refusal(cfg, **kw))
    reg = dict(base, bot=dict(base["bot"], constraints=[{"threshold": 0.5, "model": {"type": "dngo"}}]))
    assert Bz.constraint_refusal(reg) == "config.bot.constraints[0] with the dngo model: a constraint is modelled by a gp_regressor"

    def with_con(con, **score):
        return dict(base, bot=dict(base["bot"], constraints=[con]), score=dict(base["score"], **score))
    why = Bz.constraint_refusal(with_con({"threshold": 0.5, "binary": True, "model": {"type": "gp_regressor"}}))
    assert why == "config.bot.constraints[0] is binary with the gp_regressor model: a binary constraint is modelled by a gp_classifier"
    why = Bz.constraint_refusal(with_con({"threshold": 0.5, "model": {"type": "gp_classifier"}}))
    assert why and "config.bot.constraints[0] with the gp_classifier model" in why and "binary = True" in why
    why = Bz.constraint_refusal(with_con({"threshold": 0.0, "binary": True, "model": {"type": "gp_classifier"}}))
    assert why and "binary with threshold 0" in why and "threshold 0.5" in why
    why = Bz.constraint_refusal(with_con({"threshold": 0.5, "binary": True, "model": {"type": "gp_classifier"}}, type="constrained_thompson_sampling"))
    assert why and why.startswith("constrained_thompson_sampling with config.bot.constraints[0] binary") and "classifier" in why
    ok = with_con({"threshold": 0.5, "model": {"type": "gp_regressor"}}, type="constrained_thompson_sampling")
    assert Bz.constraint_refusal(ok) is None                                             # ... which a regression constraint still passes

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    bot = Bz.bayesopt(None, [], with_con({"threshold": 0.5, "binary": True, "model": {"type": "gp_regressor"}}),
                      {"model": M(), "candidates": np.zeros((4, 2))})
    with pytest.raises(NotImplementedError) as e:
        bot.run_trial()
    assert "binary constraint is modelled by a gp_classifier" in str(e.value) and bot.nTrials == 0


# ---- 6. the Lua mirror ---------------------------------------------------------------------------------------------------------------
def test_lua_mirror_static_checks():
    import test_lua_shims as L
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
    L.test_lua_blocks_and_brackets_balance()
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    i = bt.index("function bot:nominate_constrained(")
    body = bt[i:bt.index("\nend", i)]
    assert "b7_clf_eval_logfeas(hip.ctx, S, hyps, v, i, nil, nil)" in body and "b7_eval_nominate(hip.ctx, S, hyps, spec, 0, v, i, nil, nil)" in body
    assert body.index("if con.binary then") < body.index("b7_clf_eval_logfeas") < body.index("b7_eval_nominate(")
    assert "bot7.models.gp_classifier_hip" in body and "X_obs:index(1, rows), Y_obs:index(1, rows)" in body
    assert body.index("b7_clf_eval_logfeas") < body.index("sample_hyps(model, X_obs, Y_obs, S, keep)") < body.index("b7_feas_reset")
    assert "have_objective" in body and "b7_feas_nominate" in body
    i = bt.index("local function constrained_ts_refusal(")
    assert "cfg.binary" in bt[i:bt.index("\nend", i)]
    shim = open(os.path.join(ROOT, "lua", "models_gp_classifier_hip.lua")).read()
    code = L.strip_lua_comments(shim)
    assert "torch.class(title, parent)" in code and "'bot7.models.gp_classifier_hip'" in code and "'bot7.models.gp_hip'" in code
    for meth in ("init", "bounds", "nll_batch", "nll", "log_posterior", "sample_hypers", "fit", "predict", "predict_device", "fantasize"):
        assert re.search(r"function model:%s\(" % meth, code), meth
    protos = L.prototypes()
    calls = dict(L.calls(code))
    assert calls["b7_clf_nll_batch"] == protos["b7_clf_nll_batch"] == 6 and calls["b7_clf_fit_hyp"] == protos["b7_clf_fit_hyp"] == 5
    assert "slice_device" in code and "config.chains" in code
