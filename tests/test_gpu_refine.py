"""b7_eval_nominate_refine, b7_gp_grad_at and b7_score_grad_compute on the GPU, against tests/_refine_ref.py.

The bar, wherever one is needed, is tests/_exact.gp_bar's: 8 x the float64 reference's own error against the same truth (the maximum
over the case) + 16 eps x the quantity's scale.  Truth: 50-digit mpmath for N <= 64, numpy longdouble above, at no more than 8 points
per case.  Scales: sqrt(amp) + |mean| for a mean, amp for a variance, those times max_c 1 / lenscale_c for their gradients (one
lengthscale is the distance over which either changes by its own size), max(1, |v|) for a score and the largest gradient entry of
the bucket for a score's gradient.  Every test prints the worst ratio error / bar it met.

Shapes are a covering list: N in {1, 63, 64, 65, 128, 129, 257, 384} (the Npad classes 64 / 128 / 256 / 384 and their edges), d in
{1, 4, 5, 17, 32, 33, 64, 96} (every dpad class), M1 in {1, 63, 64, 65, 130} (the 64-row chunks), starts in {1, 3, 16}, S in {1, 2, 3,
10}; grids hold at most 4096 rows."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact as E
import _refine_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ratio(err, bar):
    return err / bar if bar > 0 else (0.0 if err == 0 else math.inf)


# ---- 1. b7_gp_grad_at against the truth ------------------------------------------------------------------------------------------
#             N    d   M1  kernel         log4(lenscale_sq)
GRAD_CASES = [(1, 1, 1, "ardse", -1), (63, 4, 63, "ardmatern52", -1), (64, 5, 64, "ardse", -1), (65, 17, 65, "ardmatern52", 0),
              (128, 32, 130, "ardse", 1), (129, 33, 1, "ardmatern52", 1), (257, 64, 64, "ardse", 1), (384, 96, 65, "ardmatern52", 2)]


def _grid_problem(N, d, M1, j):
    """Observations and query rows on the grid k 2^-10 under lenscale_sq = 4^j: every scaled squared distance is exact in float64
    (tests/_exact.grid_data), so K is exactly representable up to the covariance function itself."""
    X, y = E.grid_data(max(N, 2), d, 11 + N)
    X, y = X[:N], y[:N]
    rng = np.random.default_rng(1000 + N)
    xs = np.ldexp(rng.integers(0, 1024, (M1, d)).astype(np.float64), -10)
    hyp = {"lenscale_sq": np.full(d, 4.0 ** j), "amp": 1.25, "noise": 2.0 ** -7, "mean": 0.25}
    return X, y, xs, hyp


@pytest.mark.parametrize("N,d,M1,kernel,j", GRAD_CASES)
def test_gp_grad_at_against_truth(ctx, N, d, M1, kernel, j):
    X, y, xs, hyp = _grid_problem(N, d, M1, j)
    ctx.gp_set_kernel(kernel)
    try:
        ctx.gp_fit(X, y, hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        got = ctx.gp_grad_at(xs)
        mu_p, var_p = ctx.gp_predict_at(xs)
    finally:
        ctx.gp_set_kernel("ardse")
    probes = np.unique(np.concatenate([np.arange(min(4, M1)), np.arange(max(0, M1 - 4), M1)]))     # both ends of the chunks: <= 8 rows
    truth = R.post_grad_truth(X, y, hyp, xs[probes], kernel)
    ref = R.post_grad64(R.fit64(X, y, hyp, kernel), xs[probes])
    gs = 1.0 / math.sqrt(float(np.min(hyp["lenscale_sq"])))
    ms, vs = math.sqrt(hyp["amp"]) + abs(hyp["mean"]), hyp["amp"]
    worst = 0.0
    for name, g, r, t, scale in zip(("mean", "var", "dmean", "dvar"), got, ref, truth, (ms, vs, ms * gs, vs * gs)):
        bar = E.gp_bar(R.err_vs_truth(r, t), scale)
        err = R.err_vs_truth(g[probes], t)
        worst = max(worst, _ratio(err, bar))
        print("gp_grad_at N=%d d=%d M1=%d %s %s: device %.3e reference %.3e bar %.3e" % (N, d, M1, kernel, name, err,
                                                                                        R.err_vs_truth(r, t), bar))
        assert np.all(np.isfinite(g)) and err <= bar
        if name in ("mean", "var"):          # ... and b7_gp_predict_at's, within the same bar
            p = mu_p[:, 0] if name == "mean" else var_p
            dp = float(np.max(np.abs(p[probes] - g[probes])))
            print("   against b7_gp_predict_at: %.3e" % dp)
            assert dp <= bar
    print("gp_grad_at N=%d d=%d %s worst error / bar %.3f" % (N, d, kernel, worst))


# ---- 2. b7_score_grad_compute against 50 digits ---------------------------------------------------------------------------------
def _score_inputs(rng, S, P, d, z=None, fmin=-0.5):
    var = rng.uniform(0.05, 1.0, (S, P))
    mu = rng.normal(size=(S, P)) if z is None else fmin - z * np.sqrt(var)
    return mu, var, rng.normal(size=(S, P, d)), rng.normal(size=(S, P, d)) * 0.1


def _check_score(ctx, kind, S, mu, var, dmu, dvar, spec, kw, label):
    v, g = ctx.score_grad_compute(mu, var, dmu, dvar, score=kind, **kw)
    rv, rg = R.score_value_grad64(kind, mu, var, dmu, dvar, spec)
    assert np.all(np.isfinite(rv)) and np.all(np.isfinite(rg)), "the inputs must keep the reference finite"
    tv, tg = R.score_value_grad_mp(kind, mu, var, dmu, dvar, spec)
    bar_v = E.gp_bar(R.err_vs_truth(rv, tv), max(1.0, float(np.max(np.abs(rv)))))
    bar_g = E.gp_bar(R.err_vs_truth(rg, tg), float(np.max(np.abs(R.truth_to_float(tg)))))
    ev, eg = R.err_vs_truth(v, tv), R.err_vs_truth(g, tg)
    print("score_grad %s S=%d %s: value %.3e (reference %.3e, bar %.3e)  gradient %.3e (reference %.3e, bar %.3e)" % (
        kind, S, label, ev, R.err_vs_truth(rv, tv), bar_v, eg, R.err_vs_truth(rg, tg), bar_g))
    assert ev <= bar_v and eg <= bar_g
    return v, max(_ratio(ev, bar_v), _ratio(eg, bar_g))


@pytest.mark.parametrize("kind", ["ei", "cb"])
@pytest.mark.parametrize("S", [1, 3])
def test_score_grad_linear_kinds(ctx, kind, S):
    rng = np.random.default_rng(17 + S)
    mu, var, dmu, dvar = _score_inputs(rng, S, 8, 5)
    spec = {"fmin": -0.5, "tradeoff": 0.01} if kind == "ei" else {"tradeoff": 1.7, "upper": S == 3, "sign": -1.0}
    kw = dict(spec, fmin=[-0.5]) if kind == "ei" else spec
    v, worst = _check_score(ctx, kind, S, mu, var, dmu, dvar, spec, kw, "")
    print("score_grad %s S=%d worst error / bar %.3f" % (kind, S, worst))
    if S == 1:    # the value is the score kernels' own, bit for bit
        want = ctx.ei_compute(mu[0], var[0], [-0.5], 0.01) if kind == "ei" else ctx.cb_compute(mu[0], var[0], 1.7, False, -1.0)
        assert v.tobytes() == want.tobytes()


@pytest.mark.parametrize("S", [1, 2])
def test_score_grad_logei_buckets(ctx, S):
    """z in buckets over [-30, 8], each with its own bar: the cancellation in 1 + z Phi/phi grows like z^2 and the reference
    suffers it equally."""
    rng = np.random.default_rng(23 + S)
    worst = 0.0
    for lo, hi in ((-30.0, -20.0), (-20.0, -10.0), (-10.0, -3.0), (-3.0, 0.0), (0.0, 8.0)):
        z = rng.uniform(lo, hi, (S, 8))
        mu, var, dmu, dvar = _score_inputs(rng, S, 8, 4, z=z)
        spec = {"fmin": -0.5, "tradeoff": 0.0}
        v, w = _check_score(ctx, "logei", S, mu, var, dmu, dvar, spec, {"fmin": [-0.5], "tradeoff": 0.0}, "z in [%g, %g]" % (lo, hi))
        worst = max(worst, w)
        if S == 1:
            assert v.tobytes() == ctx.logei_compute(mu[0], var[0], [-0.5], 0.0).tobytes()
    print("score_grad logei S=%d worst error / bar %.3f" % (S, worst))


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------
def _problem(N, d, M, S, seed, dup=False):
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    if dup:
        X[7], X[N - 5] = X[3], X[N // 3]
    y = np.sin(3.0 * X[:, :2].sum(axis=1)) + X[:, -1] ** 2 + (0.0 if dup else 0.05) * rng.standard_normal(N)
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.05 * s} for s in range(S)]
    if dup:
        hyps[-1] = dict(hyps[-1], noise=0.0)
    return X, y.reshape(-1, 1), Xc, hyps


def _specs(kind, y):
    if kind == "cb":
        return {"score": "cb", "tradeoff": 1.0, "upper": False, "sign": -1.0}, {"tradeoff": 1.0, "upper": False, "sign": -1.0}
    return {"score": kind, "fmin": [float(y.min())], "tradeoff": 0.0}, {"fmin": float(y.min()), "tradeoff": 0.0}


#            N    d   rows  S   kind     kernel         starts iters seed dup
E2E_CASES = [(20, 2, 2000, 1, "ei", "ardse", 16, 8, 20, False),
             (20, 2, 2000, 1, "cb", "ardmatern52", 3, 8, 20, False),
             (100, 6, 4096, 10, "logei", "ardse", 16, 8, 100, False),
             (100, 6, 4096, 10, "ei", "ardmatern52", 3, 8, 100, False),
             (130, 33, 4096, 2, "cb", "ardse", 16, 6, 130, False),
             (300, 8, 4096, 3, "logei", "ardse", 3, 8, 300, False),
             (130, 33, 4096, 2, "logei", "ardse", 1, 6, 130, False),
             (300, 8, 4096, 3, "ei", "ardse", 3, 6, 301, True)]        # ... through the jitter redo


def _truth_values(X, y, hyps, jit, kernel, kind, rspec, pts):
    """The marginal score and its gradient at the rows of pts from the truth's posterior of every sample."""
    parts = [R.post_grad_truth(X, y, h, pts, kernel, jitter=float(j)) for h, j in zip(hyps, jit)]
    return R.score_value_grad_mp(kind, *(np.stack([p[i] for p in parts]) for i in range(4)), rspec)


@pytest.mark.parametrize("N,d,M,S,kind,kernel,P,iters,seed,dup", E2E_CASES)
def test_refine_end_to_end(ctx, N, d, M, S, kind, kernel, P, iters, seed, dup):
    X, y, Xc, hyps = _problem(N, d, M, S, seed, dup)
    kw, rspec = _specs(kind, y)
    lo, hi = np.zeros(d), np.ones(d)
    ctx.gp_set_kernel(kernel)
    try:
        ctx.grid_upload(Xc)
        ctx.gp_set_data(X, y)
        v0, i0, rep0 = ctx.eval_nominate(hyps, want_report=True, **kw)
        acc = ctx.score_finish(1.0, download=True)[2]
        ctx.refine_trace_enable(True)
        out = ctx.eval_nominate_refine(hyps, starts=P, iters=iters, want_report=True, **kw)
        last = ctx.refine_last()
        traces = [ctx.refine_trace(p) for p in range(P)]
        acc_after = ctx.score_finish(1.0, download=True)[2]
        out2 = ctx.eval_nominate_refine(hyps, starts=P, iters=iters, want_report=True, **kw)
        last2 = ctx.refine_last()
        traces2 = [ctx.refine_trace(p) for p in range(P)]
        ctx.refine_trace_enable(False)
        grid_after = ctx.grid_download()
        v1, i1 = ctx.eval_nominate(hyps, **kw)
    finally:
        ctx.refine_trace_enable(False)
        ctx.gp_set_kernel("ardse")
    bv, bi, x_out, val_out, start1, rep = out
    # a. b7_eval_nominate's bits
    assert np.float64(bv).tobytes() == np.float64(v0).tobytes() and bi == i0
    assert np.array_equal(rep["jitter"], rep0["jitter"]) and np.array_equal(rep["info"], rep0["info"])
    if dup:
        assert rep["jitter"][-1] > 0 and rep["info"][-1] > 0
    # afterwards: the accumulator, the grid and a plain nomination are what they were
    assert acc_after.tobytes() == acc.tobytes() and np.array_equal(grid_after, Xc)
    assert np.float64(v1).tobytes() == np.float64(v0).tobytes() and i1 == i0
    # b. the starts are TH's rule applied P times to the accumulator
    starts0 = R.th_top(acc, P)
    assert [int(i) - 1 for i in last["start_idx1"]] == starts0 and starts0[0] == i0 - 1
    # i. the same call twice gives the same bits, trace included
    assert out2[0] == out[0] and out2[1] == out[1] and out2[2].tobytes() == x_out.tobytes() and out2[4] == start1
    assert np.float64(out2[3]).tobytes() == np.float64(val_out).tobytes()
    for k in last:
        assert last[k].tobytes() == last2[k].tobytes()
    for a, b in zip(traces, traces2):
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
    # the reference and the bars of the case: the truth at 8 points -- the first (up to four) starts, where the device's marginal
    # gradient is known too (iteration 0 of their traces), then the first rungs the first start evaluated
    fits = [R.fit64(X, y, h, kernel, jitter=float(j)) for h, j in zip(hyps, rep["jitter"])]
    vg = lambda pts: R.value_grad64(fits, kind, rspec, pts)
    t0, ng = traces[0], min(P, 4)
    pts, dev = [Xc[starts0[p]] for p in range(ng)], [traces[p]["val"][0] for p in range(ng)]
    for t in range(1, iters + 1):
        c = R.ladder_candidates(t0["x"][t - 1], t0["grad"][t - 1], t0["eta"][t], lo, hi)
        if c is not None and not np.isnan(t0["cand"][t]).all():
            pts += list(c)
            dev += list(t0["cand"][t])
    pts, dev_pts = np.array(pts[:8]), np.array(dev[:8])
    tv, tg = _truth_values(X, y, hyps, rep["jitter"], kernel, kind, rspec, pts)
    rv, rg = vg(pts)
    err_ref = R.err_vs_truth(rv, tv)
    bar = E.gp_bar(err_ref, max(1.0, float(np.max(np.abs(rv)))))
    err_dev = R.err_vs_truth(dev_pts, tv)
    # the marginal gradient (every sample's dmu / dvar through the softmax or the mean): scale = its largest entry at these points
    err_gref = R.err_vs_truth(rg[:ng], tg[:ng])
    bar_g = E.gp_bar(err_gref, float(np.max(np.abs(R.truth_to_float(tg[:ng])))))
    err_gdev = R.err_vs_truth(np.array([traces[p]["grad"][0] for p in range(ng)]), tg[:ng])
    print("refine N=%d d=%d S=%d %s %s: at the truth's points value: device %.3e reference %.3e bar %.3e  gradient: device %.3e "
          "reference %.3e bar %.3e" % (N, d, S, kind, kernel, err_dev, err_ref, bar, err_gdev, err_gref, bar_g))
    assert err_dev <= bar and err_gdev <= bar_g
    worst = max(_ratio(err_dev, bar), _ratio(err_gdev, bar_g))
    # c. iteration 0's value at each start is the accumulator's entry at that row
    v_start, g_start = vg(Xc[starts0])
    for p in range(P):
        tr = traces[p]
        assert np.array_equal(tr["x"][0], Xc[starts0[p]]) and tr["rung"][0] == -1
        eg = float(np.max(np.abs(tr["grad"][0] - g_start[p])))       # every start's gradient against the reference's
        worst = max(worst, _ratio(eg, bar_g))
        assert eg <= bar_g
        e0 = abs(tr["val"][0] - acc[starts0[p]])
        worst = max(worst, _ratio(e0, bar), _ratio(abs(tr["val"][0] - v_start[p]), bar))
        assert e0 <= bar and abs(tr["val"][0] - v_start[p]) <= bar
        # d. replay from the trace; e. values never decrease
        assert np.all(np.diff(tr["val"]) >= 0.0)
        for t in range(1, iters + 1):
            eta = tr["eta"][t]
            cands = R.ladder_candidates(tr["x"][t - 1], tr["grad"][t - 1], eta, lo, hi)
            ran = not np.isnan(tr["cand"][t]).all()
            rung = int(tr["rung"][t])
            if not ran:      # no ladder: the start is flat, converged or not run, and stays
                assert cands is None or (tr["status"][t - 1] & (R.NOT_RUN | R.CONVERGED))
                assert rung == -1 and tr["x"][t].tobytes() == tr["x"][t - 1].tobytes() and tr["val"][t] == tr["val"][t - 1]
                if t < iters:
                    assert tr["eta"][t + 1] == eta
                continue
            assert cands is not None
            rc = vg(cands)[0]
            ec = float(np.max(np.abs(tr["cand"][t] - rc)))
            worst = max(worst, _ratio(ec, bar))
            assert ec <= bar, (p, t, tr["cand"][t], rc)
            want = R.ladder_decide(tr["val"][t - 1], eta, tr["cand"][t])
            assert rung == want[0] and tr["val"][t] == want[1]
            if rung >= 0:
                assert tr["x"][t].tobytes() == cands[rung].tobytes()       # the device's next x IS the taken candidate
                assert rc[rung] >= np.max(rc) - 2.0 * bar
                assert tr["status"][t] & R.MOVED
            else:
                assert tr["x"][t].tobytes() == tr["x"][t - 1].tobytes() and np.max(rc) <= tr["val"][t - 1] + 2.0 * bar
            if t < iters:
                assert tr["eta"][t + 1] == want[2]
            assert bool(tr["status"][t] & R.CONVERGED) == bool(want[3] or (tr["status"][t - 1] & R.CONVERGED))
        assert np.array_equal(last["x"][p], tr["x"][-1]) and last["val"][p] == tr["val"][-1] and last["status"][p] == tr["status"][-1]
    # f, g. the winner
    moved = bool(np.any(last["status"] & R.MOVED))
    ok = [p for p in range(P) if not (last["status"][p] & R.NOT_RUN) and np.isfinite(last["val"][p])]
    win = max(ok, key=lambda p: (last["val"][p], -p)) if moved else 0
    assert val_out == last["val"][win] and (not moved or val_out == np.max(last["val"][ok]))
    assert x_out.tobytes() == traces[win]["x"][-1].tobytes() and start1 == last["start_idx1"][win]
    assert np.all(x_out >= lo) and np.all(x_out <= hi)
    # h. at least half the gain of the float64 run from the same starts
    ref = R.refine_run(vg, Xc[starts0], iters, 1.0 / 16.0, lo, hi, grid_scores=acc[starts0])
    gain_ref, gain = ref["val"][ref["winner"]] - ref["val0"][0], val_out - traces[0]["val"][0]
    print("refine N=%d d=%d S=%d %s %s starts=%d: gain %.4g (float64 run %.4g), worst error / bar %.3f" % (N, d, S, kind, kernel, P,
                                                                                                         gain, gain_ref, worst))
    if kind == "logei":
        assert gain_ref > 0.1, "inputs: the reference gain must exceed 0.1 in log EI"
    assert gain >= 0.5 * gain_ref


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
def test_iters_zero_and_one_start(ctx):
    X, y, Xc, hyps = _problem(20, 2, 2000, 1, 20)
    kw, _ = _specs("ei", y)
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    v0, i0 = ctx.eval_nominate(hyps, **kw)
    for P in (1, 16):
        bv, bi, x, val, start = ctx.eval_nominate_refine(hyps, starts=P, iters=0, **kw)
        assert (bv, bi, start) == (v0, i0, i0) and x.tobytes() == Xc[i0 - 1].tobytes()
        assert val == ctx.refine_last()["val"][0]          # (its size against the accumulator's entry: check c of the end-to-end test)
        last = ctx.refine_last()
        assert len(last["val"]) == P and not np.any(last["status"] & R.MOVED)
    bv, bi, x, val, start = ctx.eval_nominate_refine(hyps, starts=1, iters=8, **kw)
    assert (bv, bi, start) == (v0, i0, i0) and val > v0 and ctx.refine_last()["status"][0] & R.MOVED


def test_flat_score_returns_the_nominee(ctx):
    """EI identically 0 over the grid (fmin far below the data): the nominee is row 1, every start is flat, x_out is that row."""
    X, y, Xc, hyps = _problem(20, 2, 2000, 1, 20)
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    bv, bi, x, val, start = ctx.eval_nominate_refine(hyps, starts=3, iters=4, score="ei", fmin=[-1e6], tradeoff=0.0)
    last = ctx.refine_last()
    assert (bv, bi, start, val) == (0.0, 1, 1, 0.0) and x.tobytes() == Xc[0].tobytes()
    assert np.all(last["status"] & R.FLAT) and not np.any(last["status"] & (R.MOVED | R.NOT_RUN))
    assert [int(i) for i in last["start_idx1"]] == [1, 2, 3]


def test_start_at_an_observed_point_is_not_run(ctx):
    """Zero noise (Matern: the zero-noise K stays well conditioned) and eight grid rows that ARE observations: the latent variance
    there is 0 up to rounding, on either side; where it came out below 0 the grid's score is NaN, TH's max names those rows
    first, and such a start is not run -- beside runnable ones, one of which wins."""
    X, y, Xc, hyps = _problem(20, 2, 2000, 1, 20)
    hyps = [dict(hyps[0], noise=0.0)]
    kw, _ = _specs("logei", y)
    Xc = Xc.copy()
    Xc[5:13] = X[:8]
    ctx.gp_set_kernel("ardmatern52")
    try:
        ctx.grid_upload(Xc)
        ctx.gp_set_data(X, y)
        v0, i0 = ctx.eval_nominate(hyps, **kw)
        acc = ctx.score_finish(1.0, download=True)[2]
        bv, bi, x, val, start = ctx.eval_nominate_refine(hyps, starts=16, iters=4, **kw)
        last = ctx.refine_last()
    finally:
        ctx.gp_set_kernel("ardse")
    bad = np.isnan(acc[last["start_idx1"] - 1])
    print("not-run starts: %d of 16 (NaN rows of the grid: %d)" % (int(bad.sum()), int(np.isnan(acc).sum())))
    assert bad.any() and not bad.all(), "inputs: some observed rows must score NaN, and fewer than sixteen"
    assert np.float64(bv).tobytes() == np.float64(v0).tobytes() and bi == i0
    assert np.all((last["status"][bad] & R.NOT_RUN) != 0) and np.all((last["status"][~bad] & R.NOT_RUN) == 0)
    w = list(last["start_idx1"]).index(start)
    assert np.isfinite(val) and not bad[w] and val == np.max(last["val"][~bad])


def test_box_face_is_reached(ctx):
    """A tight box around the nominee: the first rungs are clipped at a face, the point stays inside and the value still rises."""
    X, y, Xc, hyps = _problem(20, 2, 2000, 1, 20)
    kw, _ = _specs("ei", y)
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    v0, i0 = ctx.eval_nominate(hyps, **kw)
    x0 = Xc[i0 - 1]
    lo, hi = x0 - 2.0 ** -9, x0 + 2.0 ** -9
    bv, bi, x, val, start = ctx.eval_nominate_refine(hyps, starts=1, iters=6, eta0=1.0, lo=lo, hi=hi, **kw)
    assert np.all(x >= lo) and np.all(x <= hi) and (np.any(x == lo) or np.any(x == hi)) and val > v0


def test_refusals_leave_the_context_usable():
    import bot7_amd
    from bot7_amd import _lib
    X, y, Xc, hyps = _problem(20, 2, 2000, 3, 20)
    kw, _ = _specs("ei", y)
    c = bot7_amd.Context(0)
    try:
        for call in (c.refine_last, lambda: c.refine_trace(0)):                   # before any successful call
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call()
            assert e.value.code == -4
        c.grid_upload(Xc[:9])
        c.gp_set_data(X, y)
        usual = c.eval_nominate(hyps, **kw)

        def refused(code, word, **over):
            args = dict(kw, starts=3, iters=2)
            args.update(over)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                c.eval_nominate_refine(hyps, **args)
            assert e.value.code == code and word in str(e.value), str(e.value)
            assert c.eval_nominate(hyps, **kw) == usual

        refused(-1, "starts", starts=0), refused(-1, "starts", starts=17), refused(-1, "starts", starts=10)     # M = 9 rows
        refused(-1, "iters", iters=-1), refused(-1, "iters", iters=257)
        refused(-1, "eta0", eta0=0.0), refused(-1, "eta0", eta0=1.5), refused(-1, "eta0", eta0=float("nan"))
        refused(-1, "box", lo=[0.0, 0.5], hi=[1.0, 0.5]), refused(-1, "box", lo=[0.0, 0.0], hi=[1.0, float("inf")])
        refused(-5, "entropy", score="mes", fmin=None)
        c.gp_set_opts(var_with_noise=1)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.eval_nominate_refine(hyps, starts=3, iters=2, **kw)
        assert e.value.code == -5 and "var_with_noise" in str(e.value)
        c.gp_set_opts(var_clamp=1)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.eval_nominate_refine(hyps, starts=3, iters=2, **kw)
        assert e.value.code == -5
        c.gp_set_opts()
        c.gp_set_data(X, np.hstack([y, y + 1.0]))                                # two response columns
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.eval_nominate_refine(hyps, starts=3, iters=2, score="ei", fmin=[float(y.min()), float(y.min()) + 1.0])
        assert e.value.code == -5 and "response columns" in str(e.value)
        c.gp_set_data(X, y)
        spec, _ = c._pack_spec("ei", [float(y.min())], 0.0, False, -1.0)           # NULL arguments, straight at the C entry
        arr, _keep = c._pack_hyps(hyps, 2)
        assert c._L.b7_eval_nominate_refine(c._h, 3, arr, spec, None, None, None, None, None, None, None, None) == -1
        assert c.eval_nominate(hyps, **kw) == usual
        got = c.eval_nominate_refine(hyps, starts=3, iters=2, **kw)
        assert (got[0], got[1]) == usual
        c.comm_init(0, 1, _lib.comm_unique_id())                                 # a world of one: accepted, same bits
        again = c.eval_nominate_refine(hyps, starts=3, iters=2, **kw)
        assert again[:2] == got[:2] and again[2].tobytes() == got[2].tobytes() and again[3:] == got[3:]
        g = bot7_amd.Group([0, 0])                                               # a member of a group: B7_ERR_STATE
        try:
            g.grid_upload(Xc[:9])
            g.gp_set_data(X, y)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                g.members[0].eval_nominate_refine(hyps, starts=3, iters=2, **kw)
            assert e.value.code == -4 and "group" in str(e.value)
            assert g.eval_nominate(hyps, **kw) == usual
        finally:
            g.close()
    finally:
        c.close()


def test_world_of_two_is_refused(ctx, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub): b7_eval_nominate_refine answers B7_ERR_UNSUPPORTED,
    naming the communicator, on both, without a collective, and the b7_eval_nominate that follows gives the single-context
    nomination of the union."""
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7rf_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_refine_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, y, Xc, hyps = _problem(20, 2, 2000, 3, 20)
    kw, _ = _specs("ei", y)
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, y)
    want = ctx.eval_nominate(hyps, **kw)
    for o in outs:
        res = json.load(open(o))
        assert res["code"] == -5 and "communicator of 2 ranks" in res["message"] and (res["value"], res["index"]) == want


# ---- 5. the trial loop ------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, refine, seed=4):
    import bot7_amd
    from harness import benchmarks, bots
    grid = bot7_amd.grids.sobol({"size": 2000, "dims": 6, "mins": np.zeros(6), "maxes": np.ones(6)}, context=ctx)()
    cfg = {"bot": {"verbose": 0, "budget": 9, "nInitial": 5, "nSamples": 3, "seed": seed, "refine": refine},
           "grid": {"type": "sobol", "size": 2000, "dims": 6}, "score": {"type": "expected_improvement"}}
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    return bots.bayesopt(benchmarks.hartmann6, [_H("x%d" % k) for k in range(6)], cfg, cache={"candidates": grid, "model": model})


def test_trial_loop_with_refine(ctx):
    """harness bayesopt on hartmann6 (2000 Sobol candidates, nInitial 5, budget 9, nSamples 3, EI) with config.bot.refine on: the
    initial trials are the parent loop's; every model-based trial steals the grid row the winner started from, evaluates the
    objective at the refined point and observes that point; the resident grid follows; the run is deterministic.  No
    optimisation-quality claim."""
    from harness import benchmarks
    plain = _bot(ctx, False)
    first = np.array([plain.run_trial()[0] for _ in range(5)])
    runs = []
    for rep in range(2):
        bot = _bot(ctx, {"starts": 8, "iters": 6})
        assert bot.config["bot"]["refine"] == {"starts": 8, "iters": 6, "eta0": 1.0 / 16.0}
        inner, calls = ctx.eval_nominate_refine, []
        ctx.eval_nominate_refine = lambda *a, **k: calls.append(inner(*a, **k)) or calls[-1]
        try:
            rows = []
            for t in range(9):
                before = np.asarray(bot.candidates).copy()
                x, yv = bot.run_trial()
                rows.append(np.array(x))
                after = np.asarray(bot.candidates)
                if t < 5:
                    assert not calls and any(np.array_equal(x, r) for r in before)      # a grid row, as in the parent's loop
                    continue
                bv, bi, x_out, val, start = calls[-1][:5]
                assert len(calls) == t - 4 and np.array_equal(x, x_out) and np.array_equal(bot.observed[-1], x_out)
                assert np.array_equal(after, np.delete(before, start - 1, axis=0))          # the grid lost row start_idx1
                assert np.array_equal(bot.responses[-1], np.ravel(benchmarks.hartmann6(x_out.reshape(1, -1))))
                assert np.all(x_out >= 0.0) and np.all(x_out <= 1.0) and np.isfinite(val)
                assert bot.pending is None or len(bot.pending) == 0
        finally:
            del ctx.eval_nominate_refine
        assert np.array_equal(np.array(rows[:5]), first)
        assert bot.observed.shape == (9, 6) and np.asarray(bot.candidates).shape == (2000 - 9, 6)
        assert np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
        runs.append(np.array(rows))
    assert runs[0].tobytes() == runs[1].tobytes()
