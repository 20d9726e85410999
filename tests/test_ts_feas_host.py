"""Constrained Thompson sampling without a GPU: the float64 restatement of the key (tests/_ts_feas_ref.py) against exact rational
arithmetic, the order and the sequential pick on made-up path matrices, the bot's refusals and bookkeeping, the Lua shim and the
bindings.

The bar of the restatement is derived, not measured, with u = 2^-53.  A term max(c_k - t_k, 0) is one rounded difference, relative
error at most u; the running sum of C non-negative terms from 0 adds C roundings (the first, 0 + term, is exact): every term is
carried with at most (1 + u)^(C + 1) - 1 <= 2 C u for C >= 1 to first order, and no cancellation enters.  A difference of two distinct
doubles is never 0 (subnormals included), so viol is exactly 0 exactly where the exact value is 0 and the class is the exact class."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

import _ts_feas_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"b7_ts_feas_nominate": 9, "b7_ts_feas_compute": 11}
NAN, INF = float("nan"), float("inf")


# ---- 1. the restatement against exact rational arithmetic ------------------------------------------------------------------------------
def _rows_with_specials(C, n, seed):
    """c [C, n, 1] and thresholds [C]: random rows, then rows with a constraint one ulp on either side of its threshold, on it,
    the smallest subnormal against a threshold of 0, and rows far on either side."""
    rng = np.random.default_rng(seed)
    thr = rng.normal(0.0, 1.0, C)
    thr[0] = 0.0
    c = rng.normal(0.0, 1.0, (C, n))
    c[:, :8] = thr[:, None] - np.abs(c[:, :8])            # eight wholly feasible rows
    k = np.arange(n) % C
    for i, (kind, kk) in enumerate(zip(["up", "down", "on", "tiny", "tiny_neg", "huge", "low"] * 3, k[8:29])):
        row = 8 + i
        c[:, row] = thr - 0.25                            # the other constraints feasible: this one decides the class
        t = thr[kk]
        c[kk, row] = {"up": np.nextafter(t, INF), "down": np.nextafter(t, -INF), "on": t, "tiny": t + 5e-324 if t == 0.0 else np.nextafter(t, INF),
                      "tiny_neg": t - 5e-324 if t == 0.0 else np.nextafter(t, -INF), "huge": 1e300, "low": -1e300}[kind]
    return c.reshape(C, n, 1), thr


@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_key_restatement_against_rationals(C):
    c, thr = _rows_with_specials(C, 96, 100 + C)
    f = np.random.default_rng(C).normal(0.0, 1.0, (96, 1))
    viol, cls, key = R.keys(f, c, thr)
    worst = 0.0
    for i in range(96):
        exact = R.viol_exact(c[:, i, 0], thr)
        assert cls[i, 0] == (0 if exact == 0 else 1), i                     # the class is the exact class
        assert (viol[i, 0] == 0.0) == (exact == 0), i                       # 0 exactly where the exact value is 0
        assert cls[i, 0] == (0 if (c[:, i, 0] <= thr).all() else 1), i      # ... which is "every c_k <= t_k"
        assert key[i, 0] == (f[i, 0] if exact == 0 else viol[i, 0])
        if exact != 0:
            err = abs(Fraction(float(viol[i, 0])) - exact) / exact
            worst = max(worst, float(err / Fraction(2.0 * C * R.U)))
    print("viol restatement, C = %d: worst error / bar %.3f" % (C, worst))
    assert worst <= 1.0
    assert (cls[:8, 0] == 0).all() and cls[8:29, 0].tolist().count(0) > 0 and cls[8:29, 0].tolist().count(1) > 0


def test_subnormal_and_one_ulp_neighbours_of_the_threshold():
    thr = [0.0, 1.0]
    c = np.array([[[5e-324], [0.0], [-5e-324], [0.0], [0.0]], [[0.0], [0.0], [0.0], [np.nextafter(1.0, 2.0)], [np.nextafter(1.0, 0.0)]]])
    viol, cls, key = R.keys(np.arange(5.0).reshape(5, 1), c, thr)
    assert cls[:, 0].tolist() == [1, 0, 0, 1, 0]
    assert viol[0, 0] == 5e-324 and viol[3, 0] == 2.0 ** -52 and key[1, 0] == 1.0 and key[4, 0] == 4.0


def test_infinities_and_nans():
    thr = [0.5]
    f = np.array([[1.0], [-INF], [INF], [2.0], [3.0], [NAN], [4.0]])
    c = np.array([[[0.0], [0.0], [0.0], [INF], [-INF], [0.0], [NAN]]])
    viol, cls, key = R.keys(f, c, thr)
    assert cls[:, 0].tolist() == [0, 0, 0, 1, 0, -1, -1]
    assert key[1, 0] == -INF and key[2, 0] == INF and key[3, 0] == INF and viol[4, 0] == 0.0 and np.isnan(viol[5:, 0]).all()
    out = R.replay(f, c, thr)
    assert out["index"][0] == 2 and out["cls"][0] == 0 and out["key"][0] == -INF          # -inf is a legal objective value and wins


# ---- 2. the order and the sequential pick --------------------------------------------------------------------------------------------
def test_order_ties_nans_and_empty_paths():
    thr = [0.0]
    f = np.array([[3.0, NAN, 1.0], [1.0, NAN, 1.0], [1.0, NAN, 1.0], [0.0, NAN, 1.0], [NAN, NAN, 1.0]])
    c = np.array([[[-1.0, 0.0, 2.0], [-1.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 0.0, 3.0], [-1.0, 0.0, NAN]]])
    out = R.replay(f, c, thr)
    # path 0: rows 1 and 2 tie on f = 1 among the feasible; the infeasible row 3 with the lower f and the NaN row never win
    assert out["index"][0] == 2 and out["cls"][0] == 0 and out["key"][0] == 1.0
    # path 1: every row has a NaN: index 0, class -1, key NaN, NaN values; it excludes nothing
    assert out["index"][1] == 0 and out["cls"][1] == -1 and np.isnan(out["key"][1]) and np.isnan(out["y"][1]).all()
    # path 2: no feasible row: the smallest violation, a tie between rows 1 and 2; row 1 is taken, so row 2
    assert out["unexcluded"][2] == 1 and out["index"][2] == 3 and out["cls"][2] == 1 and out["key"][2] == 1.0 and out["reruns"] == 1
    assert out["y"][2].tolist() == [1.0, 1.0]


def _made_up(M, q, C, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (M, q)), rng.normal(0.0, 1.0, (C, M, q)), rng.normal(0.0, 0.5, C)


@pytest.mark.parametrize("C", [0, 1, 3])
def test_pick_rule_against_brute_force_and_prefix(C):
    f, c, thr = _made_up(90, 5, C, 7 + C)
    f[:, 3] = f[:, 1]                                       # paths 1 and 3 share their ordering: a collision
    c[:, :, 3] = c[:, :, 1]
    out = R.replay(f, c, thr)
    assert len(set(out["index"].tolist())) == 5 and out["reruns"] >= 1
    _, cls, key = R.keys(f, c, thr)
    for j in range(5):
        order = sorted((r for r in range(90) if r + 1 not in out["index"][:j].tolist()), key=lambda r: (cls[r, j], key[r, j], r))
        assert out["index"][j] == order[0] + 1 and out["cls"][j] == cls[order[0], j] and out["key"][j] == key[order[0], j]
        if C:
            feas = [r for r in order if (c[:, r, j] <= thr).all()]
            assert (out["cls"][j] == 0) == bool(feas) and (not feas or f[order[0], j] == min(f[r, j] for r in feas))
    if C == 0:                                              # no constraint: the path's first minimum over the rows not taken
        assert (out["cls"] == 0).all() and out["index"][0] == int(np.argmin(f[:, 0])) + 1
    # the prefix property: a key depends on its own path alone and the rule is sequential
    out3 = R.replay(f[:, :3], c[:, :, :3], thr)
    for name in ("index", "cls", "key", "y"):
        assert np.array_equal(out3[name], out[name][:3]), name


# ---- 3. the bot, the shim and the bindings ----------------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401
    return sys.modules["harness.bots.bayesopt"]


KIND = "constrained_thompson_sampling"


def _cfg(kind=KIND, **bot):
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "constraints": [{"threshold": 0.5, "model": {"sample": True}}]}, **bot),
            "grid": {"dims": 2}, "score": {"type": kind, "nFeatures": 64}}


def test_bot_refusals_by_name():
    Bz = _bot_module()
    cands = {"model": object(), "candidates": np.zeros((4, 2))}
    for q in (1, 4, 16):
        cfg = Bz.bayesopt(None, [], _cfg(batch=q), dict(cands)).config
        assert Bz.constraint_refusal(cfg) is None, q
    base = Bz.bayesopt(None, [], _cfg(batch=4), dict(cands)).config
    cases = [(dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "config.bot.refine"),
             (base, {"sharded": True}, "sharded"),
             (base, {"model_class": "bot7.models.dngo"}, "dngo"),
             (dict(base, bot=dict(base["bot"], constraints=[{"threshold": 0.5, "model": {"type": "dngo"}}])), {}, "modelled by a gp_regressor"),
             (dict(base, bot=dict(base["bot"], objectives={"ref": None, "model": {}})), {}, "config.bot.objectives"),
             (dict(base, bot=dict(base["bot"], trust_region={"length_init": 0.5})), {}, "config.bot.trust_region"),
             (dict(base, bot=dict(base["bot"], batch=17)), {}, "at most 16"),
             (dict(base, bot=dict(base["bot"], constraints=None)), {}, "without config.bot.constraints")]
    for cfg, kw, word in cases:
        why = Bz.constraint_refusal(cfg, **kw)
        assert why and why.startswith(KIND) and word in why, (word, why)
    # trust_region_refusal is as it was
    assert Bz.trust_region_refusal(cases[5][0]) == "config.bot.trust_region with config.bot.constraints: constraints inside a trust region are not built"

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    for cfg, kw, word in [c for c in cases if not c[1]]:
        bot = Bz.bayesopt(None, [], cfg, {"model": M(), "candidates": np.zeros((4, 2))})
        with pytest.raises(NotImplementedError) as e:
            bot.run_trial()
        assert KIND in str(e.value) and word in str(e.value), (word, str(e.value))
        assert bot.nTrials == 0                                  # refused before anything moved

    # the unchanged answers: thompson_sampling with constraints, and LogEI with a batch
    ts = Bz.constraint_refusal(dict(base, score={"type": "thompson_sampling"}, bot=dict(base["bot"], batch=1)))
    assert ts.startswith("config.bot.constraints with thompson_sampling: a sample path has no feasibility weight") and KIND in ts
    logei = Bz.constraint_refusal(dict(base, score={"type": "log_expected_improvement"}, bot=dict(base["bot"], batch=2)))
    assert logei == "config.bot.constraints with config.bot.batch > 1: feasibility-weighted believer batches are not built"
    for kind in ("confidence_bound", "max_value_entropy_search", "knowledge_gradient"):
        why = Bz.constraint_refusal(dict(base, score={"type": kind}, bot=dict(base["bot"], batch=1)))
        assert why.startswith("config.bot.constraints with %s" % kind)


def test_bot_bookkeeping_of_a_batch_trial_on_stub_contexts():
    """A batch-3 trial with two constraints against recording stand-ins: which calls, in which order, with which arguments; the three
    rows leave the candidates and every constraint context's grid; the response rows are kept whole; last_constrained keeps the call."""
    Bz = _bot_module()
    log = []

    class Ctx(object):
        def __init__(self, name, device_id=0):
            self.name, self.device_id, self.grid_version = name, device_id, 0

        def grid_upload(self, X):
            self.grid_version += 1
            log.append((self.name, "grid_upload", np.asarray(X).shape))

        def grid_remove_rows(self, idx):
            self.grid_version += 1
            log.append((self.name, "grid_remove_rows", [int(i) for i in idx]))

        def ts_paths(self, hyps, q, n_features=1024, seed=0, want_report=False):
            log.append((self.name, "ts_paths", len(hyps), q, n_features, seed))

        def ts_feas_nominate(self, cons, thresholds):
            log.append((self.name, "ts_feas_nominate", [o.name for o in cons], list(thresholds)))
            return {"key": np.array([-1.0, 0.25, -0.5]), "cls": np.array([0, 1, 0], dtype=np.int32), "index": np.array([5, 2, 9], dtype=np.int64),
                    "y": np.arange(9.0).reshape(3, 3), "reruns": 1}

    class Model(object):
        def __init__(self, ctx):
            self.ctx, self.n, self.inits = ctx, 0, 0

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
            log.append((self.ctx.name, "stage", np.asarray(Y).shape, np.asarray(grid).shape))

        def init(self, X, Y):
            self.inits += 1

    def objective(x):
        return np.array([[x[0] + x[1], x[0], x[1]]])

    two = [{"threshold": 0.5, "model": {"sample": True}}, {"threshold": -0.25, "model": {"sample": True}}]
    cand = np.random.default_rng(3).random((16, 2))
    bot = Bz.bayesopt(objective, [], _cfg(batch=3, constraints=two, seed=11), {"model": Model(Ctx("obj")), "candidates": cand.copy()})
    assert bot.score.title == "bot7.scores.constrained_thompson_sampling" and bot.score.config["nFeatures"] == 64
    cms = [Model(Ctx("con1")), Model(Ctx("con2"))]
    bot.constraints = [{"threshold": t["threshold"], "ctx": m.ctx, "grid": None, "model": m} for t, m in zip(two, cms)]
    bot.observed = np.random.default_rng(4).random((5, 2))
    bot.responses = np.concatenate([objective(x) for x in bot.observed], 0)
    bot.nTrials = 5
    x, y = bot.run_trial()
    names = [e[:2] for e in log]
    # every model samples and stages, then every context draws its paths, then ONE nomination on the objective's context
    paths = [i for i, n in enumerate(names) if n[1] == "ts_paths"]
    assert [names[i][0] for i in paths] == ["obj", "con1", "con2"] and paths == list(range(paths[0], paths[0] + 3))
    assert max(i for i, n in enumerate(names) if n[1] == "stage") < paths[0]
    assert names[paths[-1] + 1] == ("obj", "ts_feas_nominate") and log[paths[-1] + 1][2:] == (["con1", "con2"], [0.5, -0.25])
    assert all(log[i][2:5] == (2, 3, 64) for i in paths)
    seeds = [log[i][5] for i in paths]
    assert len(set(seeds)) == 3 and seeds == bot.last_constrained["seeds"]
    # no fmin, no feasibility column
    assert not any(n[1] in ("feas_reset", "feas_add_acc", "eval_nominate", "eval_nominate_feasible", "feas_nominate") for n in names)
    # each model saw its own column; the burn-in call and nSamples draws on each
    assert list(bot.model.last_Y[:, 0]) == list(bot.responses[:5, 0])
    assert [list(m.last_Y[:, 0]) for m in cms] == [list(bot.responses[:5, 1]), list(bot.responses[:5, 2])]
    assert bot.model.n == cms[0].n == cms[1].n == 3
    # the three rows left the candidates and both constraint grids in one stable pass; the response rows are whole
    assert bot.candidates.shape == (13, 2) and np.array_equal(bot.candidates, np.delete(cand, [4, 1, 8], axis=0))
    assert [e for e in log if e[1] == "grid_remove_rows"] == [("con1", "grid_remove_rows", [5, 2, 9]), ("con2", "grid_remove_rows", [5, 2, 9])]
    assert np.array_equal(bot.observed[5:], cand[[4, 1, 8]]) and bot.responses.shape == (8, 3)
    assert np.array_equal(bot.responses[5:], np.concatenate([objective(r) for r in cand[[4, 1, 8]]], 0))
    assert bot.nTrials == 6 and bot.constraints[0]["grid"].shape == (13, 2)
    lc = bot.last_constrained
    assert lc["index"] == [5, 2, 9] and lc["cls"].tolist() == [0, 1, 0] and lc["reruns"] == 1 and lc["thresholds"] == [0.5, -0.25]
    assert lc["y"].shape == (3, 3) and len(lc["hyps"]) == 2 and [len(h) for h in lc["constraint_hyps"]] == [2, 2] and "fmin" not in lc
    # the returned row is the batch's best feasible one, or its best where none is feasible
    ys = bot.responses[5:]
    ok = (ys[:, 1] <= 0.5) & (ys[:, 2] <= -0.25)
    want = int(np.where(ok, ys[:, 0], np.inf).argmin()) if ok.any() else int(ys[:, 0].argmin())
    assert np.array_equal(y, ys[want:want + 1]) and np.array_equal(x, cand[[4, 1, 8]][want])
    # the initial trials draw distinct random rows and touch no model
    del log[:]
    bot.nTrials = 2
    idx = bot.nominate_constrained()
    assert len(set(idx)) == 3 and all(1 <= i <= 13 for i in idx) and log == []


def test_score_class_calls_paths_in_model_order_then_nominates():
    from bot7_amd.scores import registry
    log = []

    class Ctx(object):
        def __init__(self, name):
            self.name = name

        def ts_paths(self, hyps, q, n_features=1024, seed=0, want_report=False):
            log.append(("paths", self.name, hyps, q, n_features, seed))

        def ts_feas_nominate(self, cons, thresholds):
            log.append(("nominate", self.name, [o.name for o in cons], thresholds))
            return "out"

    score = registry[KIND]({"nFeatures": 48})
    assert score.title == "bot7.scores." + KIND and registry[KIND]().config["nFeatures"] == 1024
    ctxs = [Ctx(k) for k in range(3)]
    assert score.nominate_constrained(ctxs, ["h0", "h1", "h2"], 4, [10, 11, 12], [0.5, 0.25]) == "out"
    assert log[:3] == [("paths", k, "h%d" % k, 4, 48, 10 + k) for k in range(3)] and log[3:] == [("nominate", 0, [1, 2], [0.5, 0.25])]
    with pytest.raises(NotImplementedError):
        score.add_to(None)


def test_header_cdef_and_symbols_carry_the_entries():
    import test_lua_shims as L
    from bot7_amd import _lib, build
    protos = L.prototypes()
    cdef = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    for name, nargs in ENTRIES.items():
        assert protos.get(name) == nargs, name
        assert re.search(r"\bint %s\(" % name, cdef), name
        assert name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
    assert re.search(r"#define B7_ABI_VERSION 1\b", header) and re.search(r"#define B7_TS_FEAS_CMAX 8\b", header)
    assert "M.TS_FEAS_CMAX = 8" in cdef and _lib.TS_FEAS_CMAX == 8 == _bot_module().TS_FEAS_CMAX
    i = header.index("int b7_ts_feas_nominate(")
    comment = header[header.rindex("/*", 0, i):i]
    for word in ("no counterpart", "Eriksson", "B7_ERR_STATE", "B7_ERR_UNSUPPORTED", "B7_ERR_INVALID", "reruns_out"):
        assert word.lower() in comment.lower(), word
    for meth in ("ts_feas_nominate", "ts_feas_compute"):
        assert callable(getattr(_lib.Context, meth))
    assert "ts_feas.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "bot7_amd", "csrc", "ts_feas.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "B7_DIAG" not in src      # the arm's switch is read in context.hip alone


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new branch: its calls name declared functions with the declared
    number of arguments, and nominate_constrained_ts makes the Python mirror's calls in the mirror's order."""
    import test_lua_shims as L
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos = L.prototypes()
    body = L._function_body(bt, "function bot:nominate_constrained_ts(")
    called = L.calls(body)
    names = [n for n, _ in called]
    for name, nargs in called:
        assert name in protos and nargs == protos[name], (name, nargs)
    assert "b7_ts_paths" in names and "b7_ts_feas_nominate" in names
    for absent in ("b7_feas_reset", "b7_feas_add_acc", "b7_eval_nominate_feasible", "b7_eval_nominate", "b7_ts_nominate"):
        assert absent not in names, absent
    first, last = body.index("b7_ts_paths(hip.ctx,"), body.rindex("b7_ts_paths(")
    assert body.index("sample_hyps(model,") < body.index("model:stage(X_obs, Y1, candidates)") < first
    assert body.index("sample_hyps(con.model,") < body.index("con.model:stage(") < first <= last < body.index("b7_ts_feas_nominate(")
    assert "self.nTrials <= self.config.bot.nInitial" in body
    for refused in ("config.bot.refine", "config.bot.objectives", "config.bot.trust_region", "without config.bot.constraints", "at most 16"):
        assert refused in bt[bt.index("local function constrained_ts_refusal("):], refused
    assert "return self:nominate_constrained_ts(" in L._function_body(bt, "function bot:nominate_constrained(")
    assert "return self:nominate_constrained_ts(" in L._function_body(bt, "function bot:nominate_batch(")
    sc = open(os.path.join(ROOT, "lua", "scores_hip.lua")).read()
    assert "constrained_thompson_sampling" in sc and "nominate_constrained_ts" in sc
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
