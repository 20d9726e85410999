"""Multi-objective Thompson sampling without a GPU: the float64 restatements of the two kernels (tests/_ts_hvi_ref.py) against exact
rational arithmetic, the pick rule on made-up path matrices, the bot's refusals, the Lua shim and the bindings.

The bar of the restatements is derived, not measured, with u = 2^-53.  Two objectives: a term is two rounded differences and one
rounded product of non-negative factors, relative error at most 3u to first order; the running sum of P + 1 non-negative terms adds
P roundings: (P + 3)u; the bar is 2 (P + 4) u of the exact value.  Three objectives: three differences and two products per term,
B - 1 additions over the B boxes: 2 (B + 5) u.  Every term is non-negative, so no cancellation enters, and a difference of two
distinct doubles is never 0: the score is exactly 0 exactly where the exact value is 0."""
import os
import re
import sys

import numpy as np
import pytest

import _ehvi3_ref as R3
import _ehvi_ref as R2
import _ts_hvi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("b7_ts_paths", "b7_ts_hvi_nominate", "b7_ts_hvi3_nominate", "b7_hvi_compute")


# ---- 1. the restatements against exact rational arithmetic ---------------------------------------------------------------------------
def _against_exact(got, hi, lo, bar_rel):
    """Row classes; exactly 0 where the exact value is 0; elsewhere the worst |got - exact| / (bar_rel exact)."""
    assert np.array_equal(np.isnan(got), np.isnan(hi))
    ok = ~np.isnan(hi)
    zero = ok & (hi == 0.0) & (lo == 0.0)
    assert (got[zero] == 0.0).all() and (got[ok & ~zero] > 0.0).all()
    live = ok & ~zero
    err = np.abs((got[live] - hi[live]) - lo[live])
    return float((err / (bar_rel * hi[live])).max()) if live.any() else 0.0


@pytest.mark.parametrize("P", [0, 1, 2, 33, 256])
def test_hvi2_restatement_against_rationals(P):
    front = R2.make_front(P)
    Y, n = R.special_rows(front, R2.REF, 96)
    got = R.hvi2_numpy(Y, front, R2.REF)
    hi, lo = R.hvi2_exact(Y, front, R2.REF)
    worst = _against_exact(got, hi, lo, 2.0 * (P + 4) * R.U)
    print("hvi2 restatement, P = %d: worst error / bar %.3f over %d rows (%d special)" % (P, worst, len(Y), n))
    assert worst <= 1.0
    assert np.isnan(got[2:5]).all() and (got[:2] == 0.0).all()          # NaN, +inf, -inf rows; ref itself and beyond ref
    assert got[5] > 0.0                                                  # the row that dominates the whole front
    # an independent float64 yardstick: the brute-force area difference agrees to its own cancellation error
    fin = np.isfinite(Y).all(axis=1)
    brute = R2.hv_improvement(front, R2.REF, Y[fin])
    assert np.abs(brute - got[fin]).max() <= 64 * (P + 4) * R2.EPS * float(np.prod(R2.REF + 0.5))


@pytest.mark.parametrize("P", [0, 1, 2, 24])
def test_hvi3_restatement_against_rationals(P):
    front = R3.make_front3(P)
    Y, n = R.special_rows(front, R3.REF3, 64)
    bx = R3.boxes3(front, R3.REF3)
    got = R.hvi3_numpy(Y, front, R3.REF3)
    fin = np.isfinite(Y).all(axis=1)
    hi, lo = np.full(len(Y), np.nan), np.zeros(len(Y))
    hi[fin], lo[fin] = R3.hv_improvement3_exact(front, R3.REF3, Y[fin])
    worst = _against_exact(got, hi, lo, 2.0 * (len(bx) + 5) * R.U)
    print("hvi3 restatement, P = %d, B = %d: worst error / bar %.3f over %d rows (%d special)" % (P, len(bx), worst, len(Y), n))
    assert worst <= 1.0
    assert np.isnan(got[2:5]).all() and (got[:2] == 0.0).all() and got[5] > 0.0


# ---- 2. the pick rule on made-up path matrices ---------------------------------------------------------------------------------------
def _made_up(m, M, q, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 1.0, (M, q)) for _ in range(m)]


@pytest.mark.parametrize("m", [2, 3])
def test_pick_rule_properties(m):
    ref = R2.REF if m == 2 else R3.REF3
    front = R2.make_front(5) if m == 2 else R3.make_front3(5)
    paths = _made_up(m, 120, 6, 11 + m)
    hv, rows, ys, fb = R.replay(paths, front, ref)
    assert len(set(rows.tolist())) == 6 and not fb.any() and (hv > 0.0).all()
    for j in range(6):
        # a picked row scores 0 under every later path once it is in that path's working front
        Yj = np.stack([p[:, j] for p in paths], axis=1)
        wf = R.canonical(np.concatenate([front, Yj[rows[:j]].reshape(-1, m)], axis=0), ref)
        assert (R.hvi_numpy(Yj[rows[:j]].reshape(-1, m), wf, ref) == 0.0).all()
        assert np.array_equal(ys[j], Yj[rows[j]])
        # and the pick is the arg-max of the restated score over the rows not taken
        s = R.hvi_numpy(Yj, wf, ref)
        s[rows[:j]] = -np.inf
        assert hv[j] == s.max() and rows[j] == int(np.argmax(s))
    # the prefix property: paths depend on j alone, the rule is sequential
    hv3, rows3, ys3, _ = R.replay([p[:, :3] for p in paths], front, ref)
    assert np.array_equal(rows3, rows[:3]) and np.array_equal(hv3, hv[:3]) and np.array_equal(ys3, ys[:3])


@pytest.mark.parametrize("m", [2, 3])
def test_pick_rule_fallback(m):
    ref = R2.REF if m == 2 else R3.REF3
    front = R2.make_front(3) if m == 2 else R3.make_front3(3)
    paths = _made_up(m, 50, 4, 5 + m)
    for p in paths:
        p[:, 1] += 2.0            # path 1's whole image lies beyond ref: nothing improves the hypervolume
    paths[1 % m][7, 1] = np.nan   # (and a NaN does not win the fallback's arg-min)
    hv, rows, ys, fb = R.replay(paths, front, ref)
    assert fb.tolist() == [False, True, False, False] and hv[1] == 0.0 and len(set(rows.tolist())) == 4
    col = paths[1 % m][:, 1].copy()
    col[rows[0]] = np.inf
    assert rows[1] == int(np.nanargmin(col)) and rows[1] != 7
    # every path dominated: objective 1 + (j mod m) takes turns
    far = [p + 2.0 for p in paths]
    hv, rows, ys, fb = R.replay(far, front, ref)
    assert fb.all() and (hv == 0.0).all()
    for j in range(4):
        assert rows[j] == R.ts_argmin(far[j % m][:, j], rows[:j])


# ---- 3. the bot, the shim and the bindings ---------------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401
    return sys.modules["harness.bots.bayesopt"]


def _ocfg(kind, three=False, **bot):
    obj = {"ref": None, "models": [{"sample": True}, {"sample": True}]} if three else {"ref": None, "model": {"sample": True}}
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "objectives": obj}, **bot), "grid": {"dims": 2}, "score": {"type": kind}}


def test_bot_refusals():
    """thompson_sampling with either objectives form passes for batch 1, 4 and 16; everything else refused with objectives keeps its
    words -- with Thompson sampling too, and for the other score types exactly as before."""
    Bz = _bot_module()
    cands = {"model": object(), "candidates": np.zeros((4, 2))}
    con = [{"threshold": 0.5, "model": {}}]
    for three in (False, True):
        count = "three" if three else "two"
        for q in (1, 4, 16):
            cfg = Bz.bayesopt(None, [], _ocfg("thompson_sampling", three, batch=q), dict(cands)).config
            assert Bz.objectives_refusal(cfg) is None, (three, q)
        ts = Bz.bayesopt(None, [], _ocfg("thompson_sampling", three, batch=4), dict(cands)).config
        why = Bz.objectives_refusal(dict(ts, bot=dict(ts["bot"], batch=17)))
        assert why and "batch = 17" in why and "at most 16" in why
        for over, kw, word in [(dict(refine={"starts": 2}), {}, "config.bot.refine: refinement of a %s-objective nominee is not built" % count),
                               (dict(constraints=con), {}, "config.bot.constraints: constraints combined with objectives are not built"),
                               ({}, {"sharded": True}, "over sharded candidates: %s objectives over a sharded grid are not built" % count),
                               ({}, {"model_class": "bot7.models.dngo"}, "with the dngo model: the Bayesian-linear head keeps no posterior")]:
            why = Bz.objectives_refusal(dict(ts, bot=dict(ts["bot"], **over)), **kw)
            assert why and why.startswith("config.bot.objectives") and word in why, (word, why)
        why = Bz.trust_region_refusal(dict(ts, bot=dict(ts["bot"], trust_region={"length_init": 0.5})))
        assert why and "trust_region" in why and "objectives" in why
        if three:
            why = Bz.objectives_refusal(dict(ts, bot=dict(ts["bot"], trust_region={"length_init": 0.5})))
            assert why == "config.bot.objectives with config.bot.trust_region: three objectives inside a trust region are not built"
            four = dict(ts, bot=dict(ts["bot"], objectives={"ref": None, "models": [{}, {}, {}]}))
            assert "four or more objectives are not built" in Bz.objectives_refusal(four)
        # the other score types: the old words, letter for letter
        ehvi = Bz.bayesopt(None, [], _ocfg(Bz.EHVI, three), dict(cands)).config
        assert Bz.objectives_refusal(dict(ehvi, bot=dict(ehvi["bot"], batch=2))) == \
            "config.bot.objectives with config.bot.batch > 1: %s-objective batches are not built" % count
        for kind in ("expected_improvement", "knowledge_gradient"):
            assert Bz.objectives_refusal(dict(ehvi, score={"type": kind})) == \
                "config.bot.objectives with %s: only expected_hypervolume_improvement is built" % kind
    none = dict(ts, bot=dict(ts["bot"], objectives=None, batch=1))
    assert Bz.objectives_refusal(none) is None                            # plain Thompson sampling: the single-objective loop
    assert "a sample path is not a per-point score" in Bz.refine_refusal(none)


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new branch: its calls name declared functions with the declared
    number of arguments, nominate_objectives and nominate_batch hand over to nominate_objectives_ts, which makes the Python mirror's
    calls in the mirror's order: hyper samples and staging per objective, the paths in objective order, then the nomination."""
    import test_lua_shims as L
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos = L.prototypes()
    body = L._function_body(bt, "function bot:nominate_objectives_ts(")
    called = L.calls(body)
    names = [n for n, _ in called]
    for name, nargs in called:
        assert name in protos and nargs == protos[name], (name, nargs)
    for name in ("b7_ts_paths", "b7_ts_hvi_nominate", "b7_ts_hvi3_nominate", "b7_pareto_front2", "b7_pareto_front3"):
        assert name in names, name
    assert "b7_eval_posterior" not in names and "b7_ts_nominate" not in names
    first, last = body.index("b7_ts_paths(hip.ctx,"), body.rindex("b7_ts_paths(")
    assert body.index("sample_hyps(model,") < body.index("model:stage(X_obs, Y1, candidates)") < first
    assert body.index("sample_hyps(o.model,") < body.index("o.model:stage(") < first < last < body.index("b7_ts_hvi_nominate(")
    assert body.count("torch.random()") == 1 and "for k = 1, m do seeds[k]" in body      # a seed per objective, in objective order
    assert "self.nTrials <= self.config.bot.nInitial" in body and "follow_steal_rows(o, self.objectives_rows, candidates)" in body
    for refused in ("config.bot.refine", "config.bot.constraints", "config.bot.trust_region", "four or more objectives"):
        assert refused in body
    handover = "return self:nominate_objectives_ts("
    assert handover in L._function_body(bt, "function bot:nominate_objectives(") and handover in L._function_body(bt, "function bot:nominate_batch(")
    # the EHVI branches keep refusing batches
    assert "two-objective batches are not built" in bt and "three-objective batches are not built" in bt
    sc = open(os.path.join(ROOT, "lua", "scores_hip.lua")).read()
    assert "nominate_objectives_ts" in sc and "b7_ts_hvi_nominate" in sc


def test_header_cdef_and_symbols_carry_the_entries():
    import test_lua_shims as L
    from bot7_amd import _lib
    protos = L.prototypes()
    cdef = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    want = {"b7_ts_paths": 8, "b7_ts_hvi_nominate": 8, "b7_ts_hvi3_nominate": 9, "b7_hvi_compute": 8}
    for name in ENTRIES:
        assert protos.get(name) == want[name], name
        assert re.search(r"\bint %s\(" % name, cdef), name
        assert name in _lib.SYMBOLS
    for meth in ("ts_paths", "ts_hvi_nominate", "hvi_compute"):
        assert callable(getattr(_lib.Context, meth))
    assert re.search(r"#define B7_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "bot7hip.h")).read())
    from bot7_amd import build
    assert "ts_hvi.hip" in build.SOURCES


def test_score_class_calls_paths_in_objective_order_then_nominates():
    """scores.thompson_sampling.nominate_objectives on recording stand-ins: ts_paths on every context in objective order with its own
    hyper samples and seed, then ONE ts_hvi_nominate on the first context with the others."""
    from bot7_amd.scores import registry
    log = []

    class Ctx(object):
        def __init__(self, name):
            self.name = name

        def ts_paths(self, hyps, q, n_features=1024, seed=0, want_report=False):
            log.append(("paths", self.name, hyps, q, n_features, seed))

        def ts_hvi_nominate(self, others, front, ref):
            log.append(("nominate", self.name, [o.name for o in ([others] if isinstance(others, Ctx) else others)]))
            return "hvi", "idx", "y"

    score = registry["thompson_sampling"]({"nFeatures": 64})
    for m in (2, 3):
        del log[:]
        ctxs = [Ctx(k) for k in range(m)]
        out = score.nominate_objectives(ctxs, ["h%d" % k for k in range(m)], 4, [10 + k for k in range(m)], "front", "ref")
        assert out == ("hvi", "idx", "y")
        assert log[:m] == [("paths", k, "h%d" % k, 4, 64, 10 + k) for k in range(m)]
        assert log[m:] == [("nominate", 0, list(range(1, m)))]
