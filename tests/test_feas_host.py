"""Constrained nomination, host side (no GPU): the float64 restatement of log Phi's three branches against 50-digit arithmetic,
the weight rule w(v, L), the declarations of the new entry points (header, Lua cdef, Python SYMBOLS), the score class, the
constrained toy, and the bot's pure bookkeeping -- column split, best-feasible fmin, the no-feasible-row branch, the refusals."""
import os
import re
import sys

import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib

import _feas_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_score_logpi", "b7_logpi_compute", "b7_feas_reset", "b7_feas_add", "b7_feas_add_acc", "b7_feas_get", "b7_feas_nominate",
       "b7_eval_nominate_feasible")
INF, NAN = np.inf, np.nan


def test_three_branches_against_50_digits():
    """log Phi(z) as score.hip evaluates it (z >= 0: log1p(-erfc(z/sqrt2)/2); -1 < z < 0: log(erfc(-z/sqrt2)/2); z <= -1:
    (-z^2/2 - log 2) + log(erfcx(-z/sqrt2))) in float64 with scipy, against mpmath on the exact values of the inputs: 3000 rows
    over z uniform [-40, 8], log-uniform [-1e6, -1], uniform [8, 40], the branch points -1, its neighbours and 0; sigma log-uniform
    in [1e-6, 1].  Bar 1e-14 in |err| / max(1, |ref|) (this test prints its figure: 4.6e-16)."""
    mu, var = R.z_set(np.random.default_rng(20141212), 3000)
    got = R.logpi_np(mu, var, 0.0, 0.0)
    err = R.scaled_errors(got, R.logpi_mp(mu, var, 0.0, 0.0))
    z = -mu / np.sqrt(var)
    print("LogPI restatement: max scaled error %.3g at z = %.6g; z in [%.3g, %.3g]" % (err.max(), z[err.argmax()], z.min(), z.max()))
    assert z.min() < -9e5 and z.max() > 39.0 and list(z[:4]) == [-1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), 0.0]
    assert not np.isnan(got).any() and (got <= 0.0).all() and np.isfinite(got).all()
    assert err.max() <= R.HOST_BAR
    assert got[3] == np.log(0.5)
    # with a threshold and a trade-off: imprv = (fmin - mu) - xi
    got = R.logpi_np(mu[:500], var[:500], 0.25, 0.5)
    assert R.scaled_errors(got, R.logpi_mp(mu[:500], var[:500], 0.25, 0.5)).max() <= R.HOST_BAR
    # the branches meet: monotone across -1 and 0
    zz = np.array([np.nextafter(-1.0, -2.0), -1.0, np.nextafter(-1.0, 0.0), np.nextafter(0.0, -1.0), 0.0, np.nextafter(0.0, 1.0)])
    g = R.logpi_np(-zz, np.ones(6), 0.0)
    assert (np.diff(g) >= 0).all() and g[2] - g[0] < 1e-15 and g[5] - g[3] < 1e-15


def test_row_classes_of_the_restatement():
    #              var == 0: imprv > 0, == 0, < 0;  var < 0;  var NaN;  mu NaN;  mu NaN at var == 0
    mu = np.array([-2.0, 0.0, 3.0, 0.0, 0.0, NAN, NAN])
    var = np.array([0.0, 0.0, 0.0, -1.0, NAN, 1.0, 0.0])
    got = R.logpi_np(mu, var, 0.0, 0.0)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == -INF and np.isnan(got[3:]).all()
    # z = +-inf with sigma > 0 (the division overflows): 0.0 and -inf; beyond |z| ~ 1.3e154 z^2/2 overflows: -inf, never NaN
    tiny = np.array([1e-320])
    assert R.logpi_np(np.array([-1e300]), tiny, 0.0)[0] == 0.0 and R.logpi_np(np.array([1e300]), tiny, 0.0)[0] == -INF
    out = R.logpi_np(np.array([1e13, 1e100, 1e154, 1e155, 1e300]), np.ones(5), 0.0)
    assert not np.isnan(out).any() and np.isfinite(out[:3]).all() and (out[3:] == -INF).all() and (np.diff(out[:3]) < 0).all()
    assert (R.logpi_np(np.array([-40.0, -1e3, -1e300]), np.ones(3), 0.0) == 0.0).all()     # Phi = 1 to the last bit


def test_weight_rule():
    """w(v, L): log kinds v + L, EI v * exp(L); NaN if either is NaN; otherwise L = -inf gives -inf / 0.0 whatever v is."""
    v = np.array([-3.0, 2.5, INF, -INF, NAN, 1.0, NAN, INF, 0.0])
    L = np.array([-1.0, 0.0, -INF, -INF, -INF, NAN, NAN, -2.0, -INF])
    wl, we = R.feas_weight_np(v, L, True), R.feas_weight_np(v, L, False)
    assert list(wl[:4]) == [-4.0, 2.5, -INF, -INF] and np.isnan(wl[4:7]).all() and wl[7] == INF and wl[8] == -INF
    assert we[0] == -3.0 * np.exp(-1.0) and we[1] == 2.5 and we[2] == 0.0 and we[3] == 0.0 and np.isnan(we[4:7]).all()
    assert we[7] == INF and we[8] == 0.0
    # L = 0 leaves a log score as it is, bit for bit, and EI as it is (x * 1.0)
    a = np.random.default_rng(1).normal(size=64)
    assert R.feas_weight_np(a, np.zeros(64), True).tobytes() == a.tobytes()
    assert R.feas_weight_np(a, np.zeros(64), False).tobytes() == a.tobytes()
    # TH's rule on the weighted vector: the first NaN wins, else the first maximum
    assert R.first_max([1.0, 3.0, 3.0, NAN, NAN]) == 3 and R.first_max([1.0, 3.0, 3.0]) == 1 and R.first_max([-INF, -INF]) == 0


def test_header_cdef_and_symbols_agree_on_the_new_entries():
    decls = {re.search(r"\b(b7_[a-z0-9_]+)\s*\(", d).group(1): d for d in gen_lua_cdef.cdef_lines(HEADER)
             if re.match(r"^(?!typedef).*\bb7_[a-z0-9_]+\s*\(", d)}
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    block = lua.split(gen_lua_cdef.BEGIN_CDEF)[1].split(gen_lua_cdef.END_CDEF)[0].splitlines()
    for name in NEW:
        assert name in decls, "include/bot7hip.h does not declare %s" % name
        assert decls[name] in block, "lua/bot7hip_ffi.lua does not carry the header's %s" % name
        assert name in _lib.SYMBOLS
    assert decls["b7_score_logpi"] == decls["b7_score_ei"].replace("b7_score_ei", "b7_score_logpi")
    assert decls["b7_logpi_compute"] == decls["b7_ei_compute"].replace("b7_ei_compute", "b7_logpi_compute")
    defs = gen_lua_cdef.defines(HEADER)
    assert defs["B7_SCORE_LOGPI"] == 5 == _lib.SCORE_LOGPI and defs["B7_SCORE_MES"] == 4 and defs["B7_SCORE_LOGEI"] == 3
    assert defs["B7_ABI_VERSION"] == 1                      # additive: the version stays
    assert "M.SCORE_LOGPI = 5" in lua.split(gen_lua_cdef.BEGIN_CONST)[1].split(gen_lua_cdef.END_CONST)[0]
    for name in ("b7_score_logpi", "b7_feas_reset"):
        i = HEADER.index(name + "(")
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "no counterpart" in comment.lower() and "Gelbart" in comment and "Gardner" in comment, name
    # which entry point does what with the kind is written down
    i = HEADER.index("#define B7_SCORE_LOGPI")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    for word in ("b7_eval_nominate_batch", "b7_blr_eval_nominate", "b7_group_eval_nominate", "b7_eval_nominate_refine", "B7_ERR_UNSUPPORTED"):
        assert word in comment, word


def test_score_class_registry_and_spec():
    from bot7_amd import scores
    assert scores.registry["log_probability_of_improvement"] is scores.log_probability_of_improvement
    lpi = scores.log_probability_of_improvement({"tradeoff": 0.25})
    assert lpi.title == "bot7.scores.log_probability_of_improvement" and lpi.config["tradeoff"] == 0.25
    Y = np.array([[3.0], [-1.5], [2.0]])
    spec = lpi.device_spec(Y)
    assert spec["score"] == "logpi" and list(spec["fmin"]) == [-1.5] and spec["tradeoff"] == 0.25
    s, fm = bot7_amd.Context._pack_spec("logpi", [0.5], 0.0, False, -1.0)
    assert (s.kind, s.tradeoff, s.fmin[0]) == (5, 0.0, 0.5)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        bot7_amd.Context._pack_spec("logpi", None, 0.0, False, -1.0)
    assert e.value.code == -1 and "LogPI needs fmin" in str(e.value)

    class Rec(object):
        def score_logpi(self, fmin, tradeoff):
            self.got = (list(fmin), tradeoff)
    r = Rec()
    lpi.add_to(r, Y)
    assert r.got == ([-1.5], 0.25)
    for meth in ("score_logpi", "logpi_compute", "feas_reset", "feas_add", "feas_add_acc", "feas_get", "feas_nominate", "eval_nominate_feasible"):
        assert callable(getattr(bot7_amd.Context, meth)), meth


def test_constrained_toy():
    """Gardner et al. 2014, simulation 1, on the unit square scaled by 6: rows [y, c], c = cos(x1 + x2); the constraint c <= 0.5
    leaves a minimum of -2 feasible and cuts other good regions out."""
    from harness import benchmarks as B
    X = np.random.default_rng(0).random((4000, 2))
    R2 = B.gardner1(X)
    assert R2.shape == (4000, 2) and B.registry["gardner1"] is B.gardner1 and B.GARDNER1_THRESHOLD == 0.5
    x1, x2 = 6.0 * X[:, 0], 6.0 * X[:, 1]
    assert np.allclose(R2[:, 0], np.cos(2 * x1) * np.cos(x2) + np.sin(x1), rtol=0, atol=1e-15)
    assert np.allclose(R2[:, 1], np.cos(x1 + x2), rtol=0, atol=1e-14)
    assert B.gardner1(X[0]).shape == (1, 2)
    ok = R2[:, 1] <= 0.5
    assert 0.4 < ok.mean() < 0.9
    assert (~ok & (R2[:, 0] < -1.0)).any() and (ok & (R2[:, 0] < -1.9)).any()   # good objective values on both sides of the constraint


def _bot_module():
    import harness.bots  # noqa: F401  (the package re-exports the class under the module's name)
    return sys.modules["harness.bots.bayesopt"]


def _cfg(**bot):
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 3, "constraints": [{"threshold": 0.5, "model": {"sample": True}}]}, **bot),
            "grid": {"dims": 2}, "score": {"type": "log_expected_improvement"}}


def test_bot_bookkeeping_columns_fmin_and_the_no_feasible_branch():
    Bz = _bot_module()
    resp = np.array([[1.0, 0.9], [0.3, 0.5], [-2.0, 0.7], [0.8, -1.0], [5.0, NAN]])
    Y, cols = Bz.split_columns(resp, 1)
    assert Y.shape == (5, 1) and list(Y[:, 0]) == [1.0, 0.3, -2.0, 0.8, 5.0] and len(cols) == 1 and cols[0].shape == (5, 1)
    assert Y.flags["C_CONTIGUOUS"] and cols[0].flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        Bz.split_columns(resp, 2)
    assert list(Bz.feasible_rows(resp, [0.5])) == [False, True, False, True, False]      # <= is feasible; a NaN is not
    assert list(Bz.best_feasible_fmin(resp, [0.5])) == [0.3]                              # not -2.0: that row violates
    assert Bz.best_feasible_fmin(resp[[0, 2, 4]], [0.5]) is None                          # -> feas_nominate
    two = np.array([[1.0, 0.0, 3.0], [0.5, 0.0, 0.0], [0.2, 1.0, 0.0]])
    assert list(Bz.feasible_rows(two, [0.5, 0.5])) == [False, True, False] and list(Bz.best_feasible_fmin(two, [0.5, 0.5])) == [0.5]

    # the nomination on stub contexts: which calls, in which order, with which arguments
    log = []

    class Ctx(object):
        def __init__(self, name, device_id=0):
            self.name, self.device_id, self.grid_version = name, device_id, 0

        def grid_upload(self, X):
            self.grid_version += 1
            log.append((self.name, "grid_upload", np.asarray(X).shape))

        def eval_nominate(self, hyps, **kw):
            log.append((self.name, "eval_nominate", len(hyps), kw["score"], list(kw["fmin"]), kw["tradeoff"]))
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
            self.ctx, self.n = ctx, 0

        def class_(self):
            return "bot7.models.gp_regressor"

        def sample_hypers(self, X, Y, *a):
            assert np.asarray(Y).shape == (len(X), 1)
            self.last_Y = np.asarray(Y).copy()
            self.n += 1
            return np.array([1.0, 1.0, 1.0, 0.1, 0.0])

        def parse_hypers(self, v):
            return {"lenscale_sq": v[:2], "amp": v[2], "noise": v[3], "mean": v[4]}

        def stage(self, X, Y, grid):
            log.append((self.ctx.name, "stage", np.asarray(Y).shape))

    cand = np.random.default_rng(3).random((16, 2))
    bot = Bz.bayesopt(None, [], _cfg(), {"model": Model(Ctx("obj")), "candidates": cand})
    assert bot.config["bot"]["constraints"] == [{"threshold": 0.5, "model": dict(Bz.bayesopt._model_defaults({"sample": True}, 3))}]
    con_model = Model(Ctx("con"))
    bot.constraints = [{"threshold": 0.5, "ctx": con_model.ctx, "grid": None, "model": con_model}]
    bot.observed, bot.nTrials = np.random.default_rng(4).random((5, 2)), 5
    for resp_k, want_tail in ((resp, ("obj", "eval_nominate_feasible", 3, "logei", [0.3])), (resp[[0, 2, 4, 0, 2]], ("obj", "feas_nominate"))):
        del log[:]
        bot.responses = resp_k
        idx = bot.nominate_constrained()
        names = [e[:2] for e in log]
        assert ("con", "eval_nominate") in names and log[names.index(("con", "eval_nominate"))][2:] == (3, "logpi", [0.5], 0.0)
        assert names.index(("con", "eval_nominate")) < names.index(("obj", "feas_reset")) < names.index(("obj", "feas_add_acc")) < len(names) - 1
        assert log[names.index(("obj", "feas_add_acc"))][2] == "con" and log[-1] == want_tail
        assert idx == (3 if len(want_tail) > 2 else 2)
        assert np.array_equal(con_model.last_Y[:, 0], resp_k[:, 1], equal_nan=True)                  # constraint model: column 1
        assert not np.array_equal(resp_k[:, 0], resp_k[:, 1], equal_nan=True)                        # (the columns differ)
        assert list(bot.model.last_Y[:, 0]) == list(resp_k[:, 0])                                    # objective model: column 0
    assert con_model.n == bot.model.n == 2 * 4                   # per trial: the burn-in call and nSamples draws, on each model
    # the initial trials draw a random row and touch no model
    del log[:]
    bot.nTrials = 2
    assert 1 <= bot.nominate_constrained() <= 16 and log == []


def test_bot_refusals_by_name():
    Bz = _bot_module()
    base = Bz.bayesopt(None, [], _cfg(), {"model": object(), "candidates": np.zeros((4, 2))}).config
    assert Bz.constraint_refusal(base) is None
    assert Bz.bayesopt(None, [], {"bot": {"verbose": 0}, "grid": {"dims": 2}}, {"model": object(), "candidates": np.zeros((4, 2))}
                       ).config["bot"]["constraints"] is None    # the default: the reference's loop
    cases = [(dict(base, bot=dict(base["bot"], batch=2)), {}, "batch"),
             (dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "refine"),
             (base, {"sharded": True}, "sharded"),
             (base, {"model_class": "bot7.models.dngo"}, "dngo"),
             (dict(base, score={"type": "thompson_sampling"}), {}, "thompson_sampling"),
             (dict(base, score={"type": "confidence_bound"}), {}, "confidence_bound"),
             (dict(base, score={"type": "max_value_entropy_search"}), {}, "max_value_entropy_search")]
    for cfg, kw, word in cases:
        why = Bz.constraint_refusal(cfg, **kw)
        assert why and word in why and "config.bot.constraints" in why, (word, why)

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    for cfg, kw, word in cases[:2] + cases[4:]:
        bot = Bz.bayesopt(None, [], cfg, {"model": M(), "candidates": np.zeros((4, 2))})
        with pytest.raises(NotImplementedError) as e:
            bot.run_trial()
        assert word in str(e.value)
        assert bot.nTrials == 0                                  # refused before anything moved


def _L_body(src, header):
    """Text of the Lua function whose header starts with `header`, up to the `end` in column 0 that closes it."""
    i = src.index(header)
    return src[i:src.index("\nend", i)]


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new ones: their calls name declared functions with the declared
    number of arguments, the score class exists and maps to B7_SCORE_LOGPI, and nominate_constrained makes the Python mirror's calls
    in the mirror's order."""
    import test_lua_shims as L
    protos = L.prototypes()
    sc = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "scores_hip.lua")).read())
    assert dict(L.calls(sc))["b7_score_logpi"] == protos["b7_score_logpi"] == 3
    assert "torch.class('bot7.scores.log_probability_of_improvement_hip', 'bot7.scores.abstract')" in sc
    assert "S.log_probability_of_improvement = LPI" in sc
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    assert "'bot7.scores.log_probability_of_improvement_hip'" in bt and "hip.SCORE_LOGPI" in bt
    body = _L_body(bt, "function bot:nominate_constrained(")
    order = [body.index(w) for w in ("b7_eval_nominate(hip.ctx, S, hyps, spec, 0,", "b7_feas_reset(hip.ctx)", "b7_feas_add_acc(hip.ctx, con.ctx)",
                                     "b7_feas_nominate(hip.ctx, v, i)", "b7_eval_nominate_feasible(hip.ctx, S, hyps, spec, v, i, jit, info)")]
    assert order == sorted(order)
    assert "self.nTrials <= self.config.bot.nInitial" in body and "R:narrow(2, k + 1, 1)" in body and "R:narrow(2, 1, 1)" in body
    # the stolen row leaves every constraint context's grid, whose record then names the driver's new tensor: before anything is staged
    assert "b7_grid_remove_rows(con.ctx, arr, 1, nil)" in _L_body(bt, "local function follow_steal(")
    assert "con.resident = {ptr = torch.data(candidates)" in bt and "self.constrained_idx = tonumber(i[0])" in body
    assert body.index("follow_steal(con, self.constrained_idx, candidates)") < body.index("on_context(con, function()")
    # on_context swaps EVERY per-context cache bot7hip_ffi keeps (the context, the resident-grid record, the kernel last set), and
    # a new constraint context starts on ARD-SE; a cache added to the ffi module later trips the list below
    ffi_src = L.strip_lua_comments(re.sub(r"ffi\.cdef\[\[.*?\]\]", "", open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read(), flags=re.S))
    state = set(re.findall(r"^\s*M\.([a-z_]+)\s*=\s*(?!function)", ffi_src, flags=re.M))
    assert state == {"ctx", "device", "group", "solo", "kernel", "resident", "_orig_steal"}, state
    per_context = ("ctx", "resident", "kernel")              # the rest belongs to the process: device, group, solo, the steal hook
    oc = _L_body(bt, "local function on_context(")
    assert "local ctx0, res0, ker0 = hip.ctx, hip.resident, hip.kernel" in oc
    assert "hip.ctx, hip.resident, hip.kernel = con.ctx, con.resident, con.kernel" in oc
    assert "con.resident, con.kernel = hip.resident, hip.kernel" in oc and "hip.ctx, hip.resident, hip.kernel = ctx0, res0, ker0" in oc
    for name in per_context:
        assert oc.count("hip." + name) >= 3, name
    assert "kernel = hip.KERNEL_ARDSE}" in body and "b7_create(ctxp, hip.device)" in body and "M.device = dev" in ffi_src
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
