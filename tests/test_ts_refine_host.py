"""CPU-side checks of the refinement of Thompson nominees on their sample paths: the float64 restatement of a path's value and
gradient (tests/_ts_refine_ref.py) against 50 digits and central differences, the start selection's restatement, the binding, the
hosts' refusals by name and the bot's bookkeeping on a stub context.  No GPU needed."""
import importlib
import os
import re

import numpy as np
import pytest

import _exact as E
import _post_ref as PR
import _refine_ref as RR
import _ts_ref as TR
import _ts_refine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problem(N, d, kernel, F=256, seed=11):
    X, Y, hyp = PR.case_inputs(N, d)
    dr = TR.draws(seed, 0, F, d, N, hyp["lenscale_sq"], hyp["noise"], kernel)
    _, vs = TR.paths_ref(X, Y, X[:1], hyp, kernel, [dr], want_v=True)
    xs = np.random.default_rng(N + d).random((4, d))
    return X, hyp, dr, vs[0], xs


@pytest.mark.parametrize("kernel", TR.KERNELS)
@pytest.mark.parametrize("N,d", [(5, 3), (64, 9)])
def test_restatement_against_50_digits_and_central_differences(kernel, N, d):
    """The float64 restatement IS numpy float64 doing this algebra, so of _exact.gp_bar (8 x numpy's own error + 16 eps x scale) only
    the second term is left to hold it to: its error against 50 digits stays below 16 eps x the sum of the absolute terms.  The
    gradient also agrees with central differences of the value to 1e-5 of its scale."""
    X, hyp, dr, v, xs = problem(N, d, kernel)
    val, grad, sv, sg = R.value_grad64(X, hyp, kernel, dr, v, xs, want_scale=True)
    tv, tg = R.value_grad_mp(X, hyp, kernel, dr, v, xs)
    for p in range(len(xs)):
        ev, eg = RR.err_vs_truth(val[p:p + 1], tv[p:p + 1]), RR.err_vs_truth(grad[p], tg[p])
        print("N %d d %d %s point %d: value %.3g of bar %.3g, gradient %.3g of bar %.3g" % (N, d, kernel, p, ev, E.gp_bar(0.0, sv[p]), eg,
                                                                                        E.gp_bar(0.0, sg[p])))
        assert ev <= E.gp_bar(0.0, sv[p]) and eg <= E.gp_bar(0.0, sg[p])
    h = 1e-6
    for c in range(d):
        e = np.zeros(d)
        e[c] = h
        fd = (R.value_grad64(X, hyp, kernel, dr, v, xs + e)[0] - R.value_grad64(X, hyp, kernel, dr, v, xs - e)[0]) / (2.0 * h)
        assert np.all(np.abs(fd - grad[:, c]) <= 1e-5 * np.maximum(sg, 1.0)), (c, fd, grad[:, c])


def test_descent_never_increases_and_moves():
    X, hyp, dr, v, xs = problem(64, 9, PR.SE)
    out = R.descend(lambda x: R.value_grad64(X, hyp, PR.SE, dr, v, x), xs, 6, 1.0 / 16.0, 0.0, 1.0)
    assert np.all(out["val"] <= out["val0"]) and np.all(out["status"] & RR.MOVED)
    assert out["winner"] == int(np.argmin(out["val"]))
    assert np.all(out["x"] >= 0.0) and np.all(out["x"] <= 1.0)


def test_start_selection():
    """Ascending by (value, row) among the rows that are no path's nominee; ties go to the lower row, a NaN is never chosen, and
    starts = M - q + 1 takes every row that is left."""
    paths = np.array([[3.0, 0.5], [1.0, 0.5], [1.0, np.nan], [np.nan, 0.1], [0.0, 0.7], [1.0, 0.2], [-1.0, 0.5]])
    nominees = [6, 3]                      # path 0's minimum, path 1's
    got = R.starts_ref(paths, nominees, 4)
    assert got[0].tolist() == [6, 4, 1, 2]              # 0.0, then the tie at 1.0 in row order; row 3 is a nominee (and a NaN)
    assert got[1].tolist() == [3, 5, 0, 1]              # 0.2, then the tie at 0.5 in row order; row 6 is path 0's nominee, row 2 a NaN
    full = R.starts_ref(paths, nominees, 7 - 2 + 1)
    assert full[0].tolist() == [6, 4, 1, 2, 5, 0] and full[1].tolist() == [3, 5, 0, 1, 4, -1]     # the NaN row leaves a rank empty
    order = np.lexsort((np.arange(7), paths[:, 0]))     # the same thing said another way
    assert [r for r in order if r not in nominees and not np.isnan(paths[r, 0])][:3] == got[0][1:].tolist()
    assert R.starts_ref(paths, nominees, 1).tolist() == [[6], [3]]


def test_binding_header_and_cdef_have_the_new_entries():
    from bot7_amd import _lib
    names = ("b7_ts_nominate_refine", "b7_ts_refine_last", "b7_ts_refine_trace_enable", "b7_ts_refine_trace", "b7_ts_path_grad_at")
    header = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
    cdef = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    for name in names:
        assert name in _lib.SYMBOLS and re.search(r"\bint %s\(" % name, header) and re.search(r"\bint %s\(" % name, cdef)
    for name in ("ts_nominate_refine", "ts_refine_last", "ts_refine_trace_enable", "ts_refine_trace", "ts_path_grad_at"):
        assert callable(getattr(_lib.Context, name))


def test_refusals_by_name():
    B = importlib.import_module("harness.bots.bayesopt")
    on = dict(B.REFINE_DEFAULTS)
    base = {"bot": {"batch": 4}, "score": {"type": "thompson_sampling", "refine": on}, "grid": {"dims": 6, "size": 512}}
    assert B.ts_refine_refusal(base) is None
    assert B.ts_refine_refusal(dict(base, bot={"batch": 16})) is None
    assert B.ts_refine_refusal(dict(base, score={"type": "thompson_sampling"})) is None, "off is not judged"
    assert B.ts_refine_refusal(dict(base, score={"type": "expected_improvement"})) is None
    assert "at most 16" in B.ts_refine_refusal(dict(base, bot={"batch": 17}))
    assert "dngo" in B.ts_refine_refusal(base, model_class="bot7.models.dngo")
    assert "sharded" in B.ts_refine_refusal(base, sharded=True)
    assert "constraints" in B.ts_refine_refusal(dict(base, bot={"batch": 1, "constraints": [{"threshold": 0.0}]}))
    assert "objectives" in B.ts_refine_refusal(dict(base, bot={"batch": 1, "objectives": {"ref": None}}))
    assert "knowledge_gradient" in B.ts_refine_refusal(dict(base, score={"type": "knowledge_gradient", "refine": on, "discretisation": "thompson"}))
    assert "expected_improvement" in B.ts_refine_refusal(dict(base, score={"type": "expected_improvement", "refine": on}))
    assert "unknown entries" in B.ts_refine_refusal(dict(base, score={"type": "thompson_sampling", "refine": dict(on, step=1)}))
    # config.bot.refine with Thompson sampling stays refused, with the message it has
    both = dict(base, bot={"batch": 1, "refine": on})
    msg = "config.bot.refine with thompson_sampling: a sample path is not a per-point score"
    assert B.refine_refusal(both) == msg and B.ts_refine_refusal(both) == msg
    assert B.refine_refusal({"bot": {"batch": 1, "refine": on}, "score": {"type": "thompson_sampling"}}) == msg
    # the trust region takes it: this is the combination the switch exists for
    assert B.trust_region_refusal(dict(base, bot={"batch": 4, "trust_region": {}})) is None


def test_configure_normalises_the_switch_and_off_adds_nothing():
    from harness import bots

    class H(object):
        def __init__(self, name):
            self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1
    bot = bots.bayesopt.__new__(bots.bayesopt)
    bot.hypers = [H("a"), H("b")]
    off = bots.bayesopt.configure(bot, {"score": {"type": "thompson_sampling"}})
    assert "refine" not in off["score"]
    on = bots.bayesopt.configure(bot, {"score": {"type": "thompson_sampling", "refine": {"iters": 4}}})
    assert on["score"]["refine"] == {"starts": 16, "iters": 4, "eta0": 1.0 / 16.0}
    from bot7_amd.scores.thompson_sampling import thompson_sampling
    assert thompson_sampling({"refine": True}).config["refine"] == {"starts": 16, "iters": 16, "eta0": 1.0 / 16.0}


class StubCtx(object):
    """ts_nominate_refine on the host: nominees = the first q rows' 1-based indices reversed, refined points = those rows + 0.25."""
    def __init__(self, grid):
        self.grid, self.calls = grid, []

    def ts_nominate_refine(self, hyps, q, n_features=1024, seed=0, starts=16, iters=16, eta0=1.0 / 16.0, lo=None, hi=None):
        self.calls.append(dict(q=q, F=n_features, starts=starts, iters=iters, eta0=eta0, lo=np.array(lo), hi=np.array(hi), S=len(hyps)))
        idx = np.arange(q, 0, -1, dtype=np.int64)
        x = self.grid[idx - 1] + 0.25
        return np.zeros(q), idx, x, np.zeros(q), idx.copy()


class StubModel(object):
    def __init__(self, ctx):
        self.ctx, self.staged = ctx, 0

    def class_(self):
        return "bot7.models.gp_regressor"

    def sample_hypers(self, *a):
        return 0

    def parse_hypers(self, _):
        return {"lenscale_sq": np.ones(2), "amp": 1.0, "noise": 1e-3, "mean": 0.0}

    def stage(self, X, Y, cand):
        self.staged += 1


def test_bot_steals_the_grid_nominees_and_observes_the_refined_points():
    B = importlib.import_module("harness.bots.bayesopt")
    from bot7_amd.scores.thompson_sampling import thompson_sampling
    grid = np.arange(20, dtype=np.float64).reshape(10, 2) / 40.0
    ctx = StubCtx(grid)
    bot = B.bayesopt.__new__(B.bayesopt)
    bot.config = {"bot": {"batch": 3, "nSamples": 2, "nInitial": 2, "refine": False, "constraints": None, "objectives": None, "trust_region": None},
                  "score": {"type": "thompson_sampling", "nFeatures": 32, "refine": {"starts": 4, "iters": 3, "eta0": 0.125}},
                  "grid": {"dims": 2, "size": 10, "mins": [0.0, 0.0], "maxes": [1.0, 1.0]}}
    bot.score = thompson_sampling(bot.config["score"])
    bot.model, bot.candidates = StubModel(ctx), grid.copy()
    bot.observed, bot.responses = np.array([[0.9, 0.9], [0.8, 0.8]]), np.array([[1.0], [2.0]])
    bot._rng, bot.nTrials = np.random.default_rng(0), 2
    seen = []
    bot.objective = lambda x: seen.append(np.array(x)) or float(np.sum(x))
    x, y = bot.run_trial()
    call = ctx.calls[0]
    assert (call["q"], call["F"], call["starts"], call["iters"], call["eta0"], call["S"]) == (3, 32, 4, 3, 0.125, 2)
    assert call["lo"].tolist() == [0.0, 0.0] and call["hi"].tolist() == [1.0, 1.0]
    assert bot.last_ts_refine["index"] == [3, 2, 1], "the rows stolen are the grid nominees"
    assert np.array_equal(bot.candidates, grid[3:]), "... all of them, in one stable pass"
    want = grid[[2, 1, 0]] + 0.25
    assert np.array_equal(np.stack(seen), want), "the objective is evaluated at the refined points"
    assert np.array_equal(bot.observed[2:], want) and bot.responses.shape == (5, 1), "... and the bot observes them"
    assert bot.nTrials == 3 and np.array_equal(x, want[2]) and y[0, 0] == want[2].sum()
    # refused configurations never reach the library
    bot.config["bot"]["constraints"] = [{"threshold": 0.0}]
    with pytest.raises(NotImplementedError, match="config.score.refine with config.bot.constraints"):
        bot.run_trial()
    assert len(ctx.calls) == 1
