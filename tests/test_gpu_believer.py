"""b7_eval_nominate_batch on the GPU: greedy batch nomination by kriging-believer variance downdates.

Pick 1 is b7_eval_nominate's, bit for bit.  Picks 2..q are checked against a REFIT through entry points this feature does not
touch -- per hyper sample b7_gp_fit on the observations with the believed rows appended at their posterior means, b7_gp_predict,
the step scores, b7_score_finish(S) -- and against the float64 restatement of tests/_believer_ref.py.  Bars: the project's
posterior bar, |dvar| <= 1e-5 amp and |dscore| <= 1e-5 max(1, |score|); at every pick the reference's top-2
gap must exceed 1000 x the achieved score error, else the test fails.  The seeds below were chosen on the CPU with
_believer_ref.greedy so that every case has top-2 gaps of at least 2e-4.  Shapes: the smallest at which each path can go wrong (one
and two 64-blocks of the small regime, ragged N in the general layout, d > 32; M never a multiple of 64)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _believer_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        name        N    d   M     q  seed
SHAPES = {"small1": (24, 3, 777, 4, 1), "small2": (100, 6, 777, 4, 2), "general": (150, 5, 1300, 4, 3), "wide": (150, 40, 520, 3, 4)}
CASES = ([("small1", S, "ardse", k) for S in (1, 3) for k in ("ei", "cb", "logei")] +
         [("small2", 3, kern, "ei") for kern in ("ardse", "ardmatern52")] +
         [("general", S, "ardse", k) for S in (1, 3) for k in ("ei", "cb", "logei")] +
         [("wide", 1, "ardse", "ei")])


def problem(name, S):
    N, d, M, q, seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rng.standard_normal(N)
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.05 * s} for s in range(S)]
    return X, y.reshape(-1, 1), Xc, hyps, q


def spec_of(kind, y):
    if kind == "cb":
        return {"score": "cb", "tradeoff": 1.0, "upper": False, "sign": -1.0}
    return {"score": kind, "fmin": [float(y.min())], "tradeoff": 0.0}


def ref_spec(kind, y):
    return {"tradeoff": 1.0, "upper": False, "sign": -1.0} if kind == "cb" else {"fmin": float(y.min()), "tradeoff": 0.0}


@pytest.fixture(scope="module")
def dctx():
    """The diagnostic build beside the shipped one: b7dbg_believer_var (the per-sample downdated variances) exists there only."""
    import bot7_amd
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_believer_var.restype = C.c_int
    c._L.b7dbg_believer_var.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    yield c
    c.close()


def believer_var(c, S, s, M):
    out = np.empty(M, dtype=np.float64)
    assert c._L.b7dbg_believer_var(c._h, S, s, out.ctypes.data) == 0
    return out


def stage(c, X, y, Xc, kernel):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def step_scores(c, kind, y, S, fits):
    """The refit path: fits = [(X_aug, y_aug, hyp)] per sample -> (means, variances, score / S, its arg-max) through
    b7_gp_fit + b7_gp_predict + the step score + b7_score_finish(S)."""
    mus, vrs = [], []
    c.score_reset()
    for Xa, ya, h in fits:
        c.gp_fit(Xa, ya, h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
        mu, var = c.gp_predict()
        mus.append(mu[:, 0].copy()), vrs.append(var.copy())
        if kind == "cb":
            c.score_cb(1.0, False, -1.0)
        elif kind == "ei":
            c.score_ei([float(y.min())], 0.0)
        else:
            c.score_logei([float(y.min())], 0.0)
    _, _, scores = c.score_finish(float(S), download=True)
    return mus, vrs, scores


@pytest.mark.parametrize("name,S,kernel,kind", CASES)
def test_picks_variances_and_scores_against_the_refit(ctx, dctx, name, S, kernel, kind):
    X, y, Xc, hyps, q = problem(name, S)
    M = len(Xc)
    stage(dctx, X, y, Xc, kernel)
    grid_before = dctx.grid_download()
    # ---- pick 1 is b7_eval_nominate's, bit for bit; q = 1 is the first pick of q = 4; two calls give identical bits
    v1, i1 = dctx.eval_nominate(hyps, **spec_of(kind, y))
    vq, iq = dctx.eval_nominate_batch(hyps, q, **spec_of(kind, y))
    vq2, iq2 = dctx.eval_nominate_batch(hyps, q, **spec_of(kind, y))
    vo, io = dctx.eval_nominate_batch(hyps, 1, **spec_of(kind, y))
    assert vq[0].tobytes() == np.float64(v1).tobytes() and iq[0] == i1
    assert vo.tobytes() == vq[:1].tobytes() and io[0] == iq[0]
    assert vq.tobytes() == vq2.tobytes() and np.array_equal(iq, iq2)
    assert len(set(iq.tolist())) == q and iq.min() >= 1 and iq.max() <= M
    assert np.array_equal(dctx.grid_download(), grid_before)                    # the caller commits, not the call
    # ---- the float64 restatement: the same greedy sequence, by the recurrence
    rp, rs, rg, _ = R.greedy(X, y, Xc, hyps, kernel, q, kind, "downdate", **ref_spec(kind, y))
    assert [p + 1 for p in rp] == iq.tolist()
    # ---- picks 2..q against the refit through the existing entry points (ctx: the shipped library)
    ctx.gp_set_kernel(kernel)
    ctx.grid_upload(Xc)
    fits = [(X, y, h) for h in hyps]
    worst_var = worst_score = 0.0
    mus = step_scores(ctx, kind, y, S, fits)[0]
    for j in range(1, q):
        row = iq[j - 1] - 1                                                     # the believed row, observed at its own mean
        fits = [(np.vstack([Xa, Xc[row]]), np.vstack([ya, [[mus[s][row]]]]), h) for s, (Xa, ya, h) in enumerate(fits)]
        mus2, vrs, scores = step_scores(ctx, kind, y, S, fits)
        vj, ij = dctx.eval_nominate_batch(hyps, j + 1, **spec_of(kind, y))       # its last pick is pick j + 1 of the batch
        assert vj.tobytes() == vq[:j + 1].tobytes() and np.array_equal(ij, iq[:j + 1])
        for s in range(S):
            dv = float(np.max(np.abs(believer_var(dctx, S, s, M) - vrs[s]))) / hyps[s]["amp"]
            worst_var = max(worst_var, dv)
            assert np.max(np.abs(mus2[s] - mus[s])) <= 1e-5 * max(1.0, np.max(np.abs(mus[s])))   # the lie leaves the mean alone
        got = dctx.score_finish(1.0, download=True)[2]                           # the accumulator: the last pick's score / S
        es = float(np.max(np.abs(got - scores) / np.maximum(1.0, np.abs(scores))))
        worst_score = max(worst_score, es)
        picked = [int(i) - 1 for i in iq[:j]]
        best, gap = R.top2(scores, picked)
        err_abs = float(np.max(np.abs(got - scores)))
        print("%s S=%d %s %s pick %d: |dvar|/amp %.3e  |dscore| %.3e (scaled %.3e)  top-2 gap %.3e" %
              (name, S, kernel, kind, j + 1, dv, err_abs, es, gap))
        assert gap > 1000.0 * err_abs, "top-2 gap %.3e within 1000 x the score error %.3e" % (gap, err_abs)
        assert best + 1 == iq[j] and vq[j] == got[best]
        assert np.max(np.abs(rs[j] - scores) / np.maximum(1.0, np.abs(scores))) <= 1e-5
        mus = mus2
    print("%s S=%d %s %s worst: |dvar|/amp %.3e  |dscore| scaled %.3e" % (name, S, kernel, kind, worst_var, worst_score))
    assert worst_var <= 1e-5 and worst_score <= 1e-5


@pytest.mark.parametrize("kind", ["ei", "cb", "logei"])
def test_pick_one_through_the_jitter_redo(dctx, kind):
    """Duplicated observations without noise under one of three hyper samples: the nomination is redone through the jitter
    schedule; pick 1 and the reports equal b7_eval_nominate's, and the later picks are distinct rows."""
    rng = np.random.default_rng(7)
    X = rng.random((300, 3))
    X[7], X[250] = X[3], X[100]
    y = np.sin(3.0 * X).sum(axis=1, keepdims=True)
    Xc = rng.random((777, 3))
    good = dict(lenscale_sq=np.full(3, 0.4), amp=1.0, noise=1e-3, mean=0.1)
    hyps = [good, dict(lenscale_sq=np.full(3, 0.4), amp=1.0, noise=0.0, mean=0.0), dict(good, amp=1.3)]
    stage(dctx, X, y, Xc, "ardse")
    v1, i1, rep1 = dctx.eval_nominate(hyps, want_report=True, **spec_of(kind, y))
    vq, iq, repq = dctx.eval_nominate_batch(hyps, 3, want_report=True, **spec_of(kind, y))
    assert rep1["jitter"][1] > 0 and rep1["info"][1] > 0
    assert vq[0].tobytes() == np.float64(v1).tobytes() and iq[0] == i1
    assert np.array_equal(repq["jitter"], rep1["jitter"]) and np.array_equal(repq["info"], rep1["info"])
    assert len(set(iq.tolist())) == 3


def test_pick_one_matern_general_layout(dctx):
    X, y, Xc, hyps, q = problem("general", 3)
    stage(dctx, X, y, Xc, "ardmatern52")
    for kind in ("ei", "cb", "logei"):
        v1, i1 = dctx.eval_nominate(hyps, **spec_of(kind, y))
        vq, iq = dctx.eval_nominate_batch(hyps, 2, **spec_of(kind, y))
        assert vq[0].tobytes() == np.float64(v1).tobytes() and iq[0] == i1 and iq[1] != iq[0]
    dctx.gp_set_kernel("ardse")


def test_refusals_leave_the_context_usable():
    import bot7_amd
    from bot7_amd import _lib
    X, y, Xc, hyps, _ = problem("small1", 3)
    c = bot7_amd.Context(0)
    try:
        stage(c, X, y, Xc[:9], "ardse")
        sp = spec_of("ei", y)
        usual = c.eval_nominate(hyps, **sp)

        def refused(code, q=2):
            before = c.eval_nominate(hyps, **sp)      # under the options in force (var_with_noise changes the score itself)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                c.eval_nominate_batch(hyps, q, **sp)
            assert e.value.code == code, str(e.value)
            assert c.eval_nominate(hyps, **sp) == before

        refused(-1, 0), refused(-1, 17), refused(-1, 10)                          # q outside 1..16, q > M = 9
        assert c.eval_nominate(hyps, **sp) == usual
        c.gp_set_opts(var_with_noise=1)
        refused(-5)
        c.gp_set_opts()
        assert c.eval_nominate(hyps, **sp) == usual
        c.gp_set_opts(var_clamp=1)
        refused(-5)
        c.gp_set_opts()
        assert c.eval_nominate(hyps, **sp) == usual
        c.gp_set_data(X, np.hstack([y, y + 1.0]))                                # two response columns
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.eval_nominate_batch(hyps, 2, score="ei", fmin=[float(y.min()), float(y.min()) + 1.0])
        assert e.value.code == -5
        c.gp_set_data(X, y)
        assert c.eval_nominate(hyps, **sp) == usual
        vq, iq = c.eval_nominate_batch(hyps, 3, **sp)
        c.comm_init(0, 1, _lib.comm_unique_id())                                 # a world of one: accepted, same bits
        vw, iw = c.eval_nominate_batch(hyps, 3, **sp)
        assert vw.tobytes() == vq.tobytes() and np.array_equal(iw, iq) and (vq[0], iq[0]) == usual
    finally:
        c.close()


def test_world_of_two_is_refused(ctx, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub): b7_eval_nominate_batch answers B7_ERR_UNSUPPORTED on
    both, and the b7_eval_nominate that follows gives the single-context nomination of the union."""
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7bel_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_believer_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, y, Xc, hyps, _ = problem("small1", 3)
    stage(ctx, X, y, Xc, "ardse")
    want = ctx.eval_nominate(hyps, **spec_of("ei", y))
    for o in outs:
        res = json.load(open(o))
        assert res["code"] == -5 and (res["value"], res["index"]) == want


class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, batch):
    import bot7_amd
    from harness import benchmarks, bots
    grid = bot7_amd.grids.random({"size": 256, "dims": 2, "seed": 5, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    cfg = {"bot": {"verbose": 0, "budget": 5, "nInitial": 2, "nSamples": 1, "seed": 1},
           "grid": {"type": "random", "size": 256, "dims": 2}, "score": {"type": "expected_improvement"}}
    if batch is not None:
        cfg["bot"]["batch"] = batch
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    return bots.bayesopt(benchmarks.braninhoo, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})


def test_python_round_trip_and_harness_bot(ctx):
    # batch = 1 (and no batch at all) is the existing loop
    runs = []
    for batch in (None, 1):
        bot = _bot(ctx, batch)
        assert bot.config["bot"]["batch"] == 1
        runs.append(np.array([bot.run_trial()[0] for _ in range(5)]))
    assert np.array_equal(runs[0], runs[1])
    assert bot.nominate_batch(1) == [bot.nominate()]
    # batch = 3: two random trials, then three model-based ones, three rows committed per trial
    bot = _bot(ctx, 3)
    host = np.asarray(bot.candidates).copy()
    calls, inner = [], bot.nominate_batch
    bot.nominate_batch = lambda *a, **k: calls.append(inner(*a, **k)) or calls[-1]
    for t in range(1, 6):
        before = np.asarray(bot.candidates).copy()
        obs, resp = bot.observed, bot.responses
        bot.run_trial()
        idx = calls[-1]
        assert len(calls) == t and len(set(idx)) == 3
        assert bot.observed.shape == (3 * t, 2) and bot.responses.shape == (3 * t, 1)
        assert np.asarray(bot.candidates).shape == (256 - 3 * t, 2)
        assert np.array_equal(bot.observed[-3:], before[np.array(idx) - 1])
        assert np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
        if t > 2:   # model-based: the float64 restatement names the same three rows from the same data
            picks = R.greedy(obs, resp, before, [bot.model.hyp], "ardse", 3, "ei", fmin=float(resp.min()), tradeoff=0.0)[0]
            assert [p + 1 for p in picks] == idx
    assert host.shape == (256, 2)
