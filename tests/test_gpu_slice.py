"""b7_gp_slice_sample on the GPU: the device chain replayed decision for decision.

The trace gives, per chain, the draws every update used and every density request it made.  The tests hold (i) the draws against
the host's counter generator, (ii) every evaluated density against b7_gp_nll_batch at the traced hyper pack, bit for bit, and
(iii) the whole chain against tests/_slice_ref.py -- the op-by-op restatement that tests/test_slice_host.py pins to
harness/samplers/slice.py -- fed the traced draws and values.  No statistical test: the replay makes the device chain the
reference's chain."""
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib
from conftest import make_problem
from harness import benchmarks as B
from harness import bots

import _slice_ref as R

pytestmark = pytest.mark.gpu
RPC = 1024   # trace records kept per chain


def _objective(X):
    return np.sin(3.0 * X.sum(axis=1, keepdims=True)) + X[:, -1:] ** 2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def within_ulp(a, b, n):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((a == b) | (np.abs(a - b) <= n * np.spacing(np.abs(b)))))


_problems = {}


def problem(orc, N, d):
    """make_problem's data, the model's bounds and C start points (chain c a little off the point estimate, inside the bounds)."""
    if (N, d) not in _problems:
        X, y, _Xc, hyp = make_problem(None, orc, d, N, 200, _objective)
        model = bot7_amd.models.gp_regressor({})
        lo, hi = model._bounds_compute(X, y)
        t0 = model._to_theta(hyp)
        starts = np.stack([np.clip(t0 + 0.05 * c, lo, hi) for c in range(3)])
        _problems[(N, d)] = (X, y, lo, hi, starts)
    return _problems[(N, d)]


def traced(ctx, X, y, kernel, theta0, lo, hi, U, seed, update0=0, max_evals=512, width=0.5):
    ctx.gp_set_kernel(kernel)
    ctx.gp_set_data(X, y)
    ctx.gp_slice_trace_enable(RPC)
    try:
        out = ctx.gp_slice_sample(theta0, lo, hi, np.full(lo.size, width), U, seed, update0=update0, max_evals=max_evals)
        traces = [ctx.gp_slice_trace(c) for c in range(np.atleast_2d(theta0).shape[0])]
    finally:
        ctx.gp_slice_trace_enable(0)
    return out, traces


class TraceDraws(object):
    """The draws a chain's trace recorded, handed to the restatement."""

    def __init__(self, trace):
        self.upd = {r["g"]: r for r in trace if r["type"] == "update"}
        self.shrink, g = {}, None
        for r in trace:
            if r["type"] == "update":
                g = r["g"]
                self.shrink[g] = []
            elif r["kind"] == R.KIND_SHRINK:
                self.shrink[g].append(r["u"])

    def normals(self, g, D):
        return list(self.upd[g]["z"])

    def log_u_Y(self, g):
        return float(self.upd[g]["log_u_Y"])

    def u_right(self, g, D):
        return list(self.upd[g]["u_right"])

    def u_shrink(self, g, i):
        assert i < len(self.shrink[g]), "the restatement shrinks further than the device did (update %d)" % g
        return float(self.shrink[g][i])


def replay_chain(ctx, trace, out, c, theta0, lo, hi, widths, U, seed, update0, max_evals, d):
    """Checks (i) .. (iv) of one chain; returns the number of requests per update."""
    key = R.counter_key(seed, c)
    D = d + 3
    assert len(trace) < RPC, "the trace buffer was too small for this case"
    # (i) the draws
    per_update, g, nshrink = {}, None, 0
    for r in trace:
        if r["type"] == "update":
            g, nshrink = r["g"], 0
            per_update[g] = []
            base = R.CTR_STRIDE * g
            assert r["u_Y"] == R.counter_uniform(key, base + R.CTR_UY)
            assert list(r["u_right"]) == [R.counter_uniform(key, base + R.CTR_RIGHT + k) for k in range(D)]
            assert within_ulp(r["z"], [R.counter_normal(key, base + R.CTR_Z + k) for k in range(D)], 4)
            assert within_ulp(r["log_u_Y"], np.log(r["u_Y"]), 4)
        else:
            per_update[g].append(r)
            if r["kind"] == R.KIND_SHRINK:
                assert r["u"] == R.counter_uniform(key, R.CTR_STRIDE * g + R.CTR_SHRINK + nshrink)
                nshrink += 1
    assert sorted(per_update) == list(range(update0, update0 + U))
    # (ii) every evaluated density is b7_gp_nll_batch's at the traced pack, bit for bit
    table, nev = {}, 0
    for r in trace:
        if r["type"] != "request" or r["reused"] or not r["in_bounds"]:
            continue
        nev += 1
        th, h = r["theta"], r["hyp"]
        assert within_ulp(h[:d + 2], np.exp(th[:d + 2]), 1) and h[d + 2] == th[d + 2]
        nll, jit, info = ctx.gp_nll_batch(h[:d], h[d], h[d + 1], h[d + 2], want_info=True)
        assert jit[0] == 0.0 and info[0] == 0
        assert same_bits(-nll[0], r["value"]), (r, nll)
        table[th.tobytes()] = r["value"]
    assert nev == out["nevals"][c]
    # (iii) the restatement, fed the traced draws and values, makes the same requests and ends on the same points
    ref = R.slice_chain(lambda t: table[np.asarray(t).tobytes()], TraceDraws(trace), theta0, lo, hi, widths, U, update0=update0,
                        max_evals=max_evals)
    dev_req = [r for r in trace if r["type"] == "request"]
    assert len(ref["requests"]) == len(dev_req)
    for a, b in zip(ref["requests"], dev_req):
        assert a["kind"] == b["kind"] and a["in_bounds"] == b["in_bounds"] and a["reused"] == b["reused"]
        assert same_bits(a["theta"], b["theta"]) and same_bits(a["value"], b["value"]) and a["u"] == b["u"]
    assert same_bits(ref["theta"], out["theta"][c]) and same_bits(ref["value"], out["value"][c])
    assert ref["status"] == list(out["status"][c]) and ref["nevals"] == out["nevals"][c]
    # (iv) every accepted value exceeds its slice level
    for u in range(U):
        if out["status"][c][u] == 0:
            reqs = per_update[update0 + u]
            assert reqs[0]["kind"] == R.KIND_START
            Y = reqs[0]["value"] + TraceDraws(trace).log_u_Y(update0 + u)
            assert out["value"][c][u] > Y
    return {g: len(v) for g, v in per_update.items()}


CASES = [(5, 1, "ardse"), (64, 6, "ardse"), (65, 6, "ardse"), (65, 6, "ardmatern52"), (100, 6, "ardse"), (100, 6, "ardmatern52"),
         (128, 32, "ardse")]


@pytest.mark.parametrize("U", [1, 4])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N,d,kernel", CASES)
def test_replay(ctx, orc, N, d, kernel, C, U):
    X, y, lo, hi, starts = problem(orc, N, d)
    seed = 1000 + N
    out, traces = traced(ctx, X, y, kernel, starts[:C], lo, hi, U, seed)
    assert out["theta"].shape == (C, U, d + 3)
    for c in range(C):
        replay_chain(ctx, traces[c], out, c, starts[c], lo, hi, np.full(d + 3, 0.5), U, seed, 0, 512, d)
        assert ((out["theta"][c] >= lo) & (out["theta"][c] <= hi)).all()


def test_split_invariance(ctx, orc):
    """U = 4 in one call is four calls of U = 1 chained through theta_out and update0; chain c does not depend on C."""
    X, y, lo, hi, starts = problem(orc, 65, 6)
    ctx.gp_set_kernel("ardse")
    ctx.gp_set_data(X, y)
    wd = np.full(9, 0.5)
    whole = ctx.gp_slice_sample(starts, lo, hi, wd, 4, 77)
    theta = starts.copy()
    for u in range(4):
        one = ctx.gp_slice_sample(theta, lo, hi, wd, 1, 77, update0=u)
        assert same_bits(one["theta"][:, 0], whole["theta"][:, u]) and same_bits(one["value"][:, 0], whole["value"][:, u])
        assert np.array_equal(one["status"][:, 0], whole["status"][:, u])
        theta = one["theta"][:, 0].copy()
    alone = ctx.gp_slice_sample(starts[:1], lo, hi, wd, 4, 77)
    assert same_bits(alone["theta"][0], whole["theta"][0]) and same_bits(alone["value"][0], whole["value"][0])
    again = ctx.gp_slice_sample(starts, lo, hi, wd, 4, 77)
    assert same_bits(again["theta"], whole["theta"]) and np.array_equal(again["nevals"], whole["nevals"])


def test_evaluation_cap(ctx, orc):
    """max_evals = 3: an update the replay's trace shows to need more returns x0 with status 4, and the next update proceeds."""
    X, y, lo, hi, starts = problem(orc, 64, 6)
    out, traces = traced(ctx, X, y, "ardse", starts[:1], lo, hi, 4, 31)
    counts = replay_chain(ctx, traces[0], out, 0, starts[0], lo, hi, np.full(9, 0.5), 4, 31, 0, 512, 6)
    u = next(g for g in sorted(counts) if counts[g] > 3)   # (a slice update makes at least start, right, left, one shrink)
    x0 = starts[0] if u == 0 else out["theta"][0][u - 1]
    capped, traces = traced(ctx, X, y, "ardse", x0.reshape(1, -1), lo, hi, 2, 31, update0=u, max_evals=3)
    assert capped["status"][0][0] == _lib.SLICE_CAP and same_bits(capped["theta"][0][0], x0)
    first = [r for r in traces[0] if r["type"] == "request"][0]
    assert same_bits(capped["value"][0][0], first["value"])            # f(x0)
    assert not capped["status"][0][1] & _lib.SLICE_NOT_RUN and capped["nevals"][0] >= 2
    replay_chain(ctx, traces[0], capped, 0, x0, lo, hi, np.full(9, 0.5), 2, 31, u, 3, 6)


def singular_problem(orc):
    """Two duplicated observation rows and a start point with log noise = -690: K + noise I has no plain factorisation."""
    X, y, lo, hi, starts = problem(orc, 64, 6)
    X, y = X[:40].copy(), y[:40].copy()
    X[1], y[1] = X[0], y[0]
    lo = lo.copy()
    lo[-2] = -700.0
    t0 = starts[0].copy()
    t0[-2] = -690.0
    return X, y, lo, hi, t0


def test_failed_pivot_stops_the_chain(ctx, orc):
    X, y, lo, hi, t0 = singular_problem(orc)
    ctx.gp_set_kernel("ardse")
    ctx.gp_set_data(X, y)
    out = ctx.gp_slice_sample(t0, lo, hi, np.full(9, 0.5), 3, 5)          # returns: a numerical refusal, not an error
    assert list(out["status"][0]) == [_lib.SLICE_PIVOT, _lib.SLICE_NOT_RUN, _lib.SLICE_NOT_RUN]
    assert all(same_bits(out["theta"][0][u], t0) for u in range(3)) and out["nevals"][0] == 1
    # the model finishes such a chain through the host sampler, whose evaluations carry the jitter schedule
    model = bot7_amd.models.gp_regressor({"sample": True, "sampler": "slice_device", "nBurnin": 2, "seed": 5,
                                          "bounds": {"noise_min": float(np.exp(-700.0))}}, context=ctx)
    model.hyp = model._from_theta(t0)
    model.sample_hypers(X, y)
    assert model._dev["host_calls"] == 1 and model.last_fit["jitter"] > 0.0
    lo_m, hi_m = model._bounds(X, y)
    assert ((model._dev["thetas"] >= lo_m) & (model._dev["thetas"] <= hi_m)).all()


def _nominate_bits(ctx, X, y, Xc, hyp):
    ctx.gp_set_kernel("ardse")
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    return ctx.eval_nominate([hyp], "ei", fmin=float(y.min()))


def test_refusals_leave_the_context_usable(ctx, orc):
    X, y, Xc, hyp = make_problem(None, orc, 3, 37, 300, _objective)
    before = _nominate_bits(ctx, X, y, Xc, hyp)
    rng = np.random.default_rng(0)

    def refused(code, word, X_, y_, t0, lo, hi, U=1, **kw):
        if X_ is not None:
            ctx.gp_set_data(X_, y_)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            ctx.gp_slice_sample(t0, lo, hi, np.full(np.asarray(lo).size, 0.5), U, 1, **kw)
        assert e.value.code == code and word in str(e.value), str(e.value)

    def box(D):
        return np.zeros((1, D)), np.full(D, -5.0), np.full(D, 5.0)

    refused(-5, "N = 129", rng.random((129, 3)), rng.normal(size=(129, 1)), *box(6))
    refused(-5, "d = 33", rng.random((20, 33)), rng.normal(size=(20, 1)), *box(36))
    refused(-5, "2 response columns", rng.random((20, 3)), rng.normal(size=(20, 2)), *box(6))
    t0, lo, hi = box(6)
    ctx.gp_set_data(X, y)
    refused(-1, "C = 0", None, None, np.zeros((0, 6)), lo, hi)
    refused(-1, "U * max_evals", None, None, t0, lo, hi, U=200, max_evals=512)
    refused(-5, "Gibbs", None, None, t0, lo, hi, gibbs=True)
    refused(-5, "linear space", None, None, t0, lo, hi, logspace=False)
    fresh = bot7_amd.Context(0)
    try:
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            fresh.gp_slice_sample(np.zeros((1, 6)), lo, hi, np.full(6, 0.5), 1, 1)
        assert e.value.code == -4 and "no resident data" in str(e.value)
    finally:
        fresh.close()
    after = _nominate_bits(ctx, X, y, Xc, hyp)
    assert after[1] == before[1] and same_bits(after[0], before[0])


def test_nothing_else_moved(ctx, orc):
    """A fit, its predictions and a pending score accumulator are the same before and after a b7_gp_slice_sample."""
    X, y, Xc, hyp = make_problem(None, orc, 6, 64, 300, _objective)
    _X, _y, lo, hi, starts = problem(orc, 64, 6)
    ctx.gp_set_kernel("ardse")
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    ctx.gp_fit_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
    mu0, var0 = ctx.gp_predict(download=True)
    ctx.score_reset()
    ctx.score_ei(float(y.min()), 0.0)          # a pending accumulator
    L0 = ctx.gp_download(64)
    out = ctx.gp_slice_sample(starts, lo, hi, np.full(9, 0.5), 2, 9)
    assert (out["status"] == 0).all()
    assert all(same_bits(a, b) for a, b in zip(L0, ctx.gp_download(64)))
    val, idx, sc = ctx.score_finish(1.0, download=True)
    mu1, var1 = ctx.gp_predict(download=True)
    assert same_bits(mu0, mu1) and same_bits(var0, var1)
    ctx.score_reset()
    ctx.score_ei(float(y.min()), 0.0)
    val2, idx2, sc2 = ctx.score_finish(1.0, download=True)
    assert same_bits(sc, sc2) and idx == idx2 and same_bits(val, val2)


@pytest.mark.parametrize("chains", [1, 4])
def test_trial_loop(ctx, chains):
    """The harness bot on hartmann6 with sampler = 'slice_device': runs to the end, deterministic, ONE library call per trial for
    sampling (burn-in 0: the pool of nSamples updates), every sampled theta inside the bounds."""
    class H(object):
        def __init__(self, name):
            self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1

    def run():
        cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 3, "nSamples": 4, "seed": 2},
               "grid": {"type": "sobol", "size": 2000, "dims": 6}, "score": {"type": "expected_improvement"},
               "model": {"type": "gp_regressor", "sample": True, "sampler": "slice_device", "chains": chains, "nBurnin": 0, "seed": 5}}
        bot = bots.bayesopt(B.hartmann6, [H("x%d" % k) for k in range(6)], cfg)
        assert bot.model.config["prefetch"] == 4
        bot.model._ctx = ctx
        bot.candidates = bot7_amd.grids.sobol(bot.config["grid"], context=ctx)()
        calls, thetas, inner, model = [], [], ctx.gp_slice_sample, bot.model

        def counting(*a, **k):
            calls.append(1)
            return inner(*a, **k)
        sample_inner = model.sample_hypers

        def recording(X, Y, *a):
            v = sample_inner(X, Y, *a)
            if len(a) >= 3 and a[2]:
                Xa = np.atleast_2d(np.asarray(X, dtype=np.float64))
                Ya = np.asarray(Y, dtype=np.float64).reshape(Xa.shape[0], -1)
                lo, hi = model._bounds(Xa, Ya)
                t = model._to_theta(model.parse_hypers(v))
                assert ((t >= lo - 1e-12) & (t <= hi + 1e-12)).all()
                thetas.append(v.copy())
            return v
        ctx.gp_slice_sample, model.sample_hypers = counting, recording
        try:
            bot.run_experiment()
        finally:
            del ctx.gp_slice_sample
        assert np.asarray(bot.observed).shape == (12, 6)
        return len(calls), np.asarray(bot.observed).copy(), np.asarray(thetas)

    n1, obs1, th1 = run()
    n2, obs2, th2 = run()
    assert n1 == n2 == 12 - 3                    # one library call per model-based trial
    assert th1.shape == (4 * (12 - 3), 9)
    assert same_bits(obs1, obs2) and same_bits(th1, th2)
