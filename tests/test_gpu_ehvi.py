"""b7_eval_posterior / b7_posterior_get / b7_ehvi_compute / b7_ehvi_nominate on the GPU: two-objective nomination by the exact
expected hypervolume improvement.

The score kernel is measured against the marginal formula at 50 digits (tests/_ehvi_ref.ehvi_mp) with the project's bar,
tests/_exact.gp_bar: per row 8 x the error of the float64 restatement (ehvi_numpy) against the same 50 digits + 16 eps x the row's
scale, the EHVI against an empty front Psi1(r1) Psi2(r2) at 50 digits, which bounds every EHVI of the row.  The kept posterior, the
accumulator and the nominee are compared bit for bit with the calls they restate.  Every test prints its achieved figure; the
docstrings carry the MI355X figures."""
import numpy as np
import pytest

import _ehvi_ref as R
import _exact as E

pytestmark = pytest.mark.gpu


def bar_ratio(got, mu1, var1, mu2, var2, front, ref):
    """Row classes exactly; the worst |got - 50 digits| / bar over the rows, bar = gp_bar(ehvi_numpy's error, scale) per row (a bar
    of 0 -- the restatement exact and the scale 0 -- admits an error of 0 alone)."""
    hi, lo = R.ehvi_mp(mu1, var1, mu2, var2, front, ref)
    assert np.array_equal(np.isnan(got), np.isnan(hi)), "row classes differ"
    ok = ~np.isnan(hi)
    assert np.isfinite(got[ok]).all() and (got[ok] >= 0.0).all()
    err_np = R.err_vs_mp(R.ehvi_numpy(mu1, var1, mu2, var2, front, ref), hi, lo)[ok]
    scale = R.empty_scale_mp(mu1, var1, mu2, var2, ref)[ok]
    bar = E.gp_bar(err_np, scale)
    err = R.err_vs_mp(got, hi, lo)[ok]
    assert (err[bar == 0.0] == 0.0).all()
    live = bar > 0.0
    return float((err[live] / bar[live]).max()) if live.any() else 0.0


# ---- 1. the kernel against 50 digits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,S1,S2", R.KERNEL_CASES)
def test_kernel_against_50_digits(ctx, M, P, S1, S2):
    """b7_ehvi_compute on synthetic posteriors (_ehvi_ref.make_rows: mu from far below the front to far beyond ref, z down to -40
    and past the point where float64 gives 0; sigma 1e-8 .. 1e2 of the front's extent; var == 0 in one sample and in all; the NaN
    and var < 0 classes) against fronts whose first two points are one ulp apart in the first objective.  M = 1000 spans sixteen
    workgroups and ends inside one; (S1, S2) = (11, 1) puts one sample in LDS, (32, 32) twenty-two of each.  Bar: module docstring.
    On an MI355X the worst ratio to the bar over the eight cases is 0.32 (M = 1000)."""
    mu1, var1, mu2, var2 = R.make_rows(M, S1, S2)
    front = R.make_front(P)
    got = ctx.ehvi_compute(mu1, var1, mu2, var2, front, R.REF)
    assert got.shape == (M,)
    worst = bar_ratio(got, mu1, var1, mu2, var2, front, R.REF)
    print("ehvi kernel M=%d P=%d S=(%d, %d): worst error / bar %.3g" % (M, P, S1, S2, worst))
    assert worst <= 1.0
    assert ctx.ehvi_compute(mu1, var1, mu2, var2, front, R.REF).tobytes() == got.tobytes()      # the same call twice: the same bits
    if M >= 128:    # a row's value does not depend on where in the launch it sits
        part = ctx.ehvi_compute(mu1[:, 37:101], var1[:, 37:101], mu2[:, 37:101], var2[:, 37:101], front, R.REF)
        assert part.tobytes() == got[37:101].tobytes()


def test_compute_refusals(ctx):
    mu, var = np.zeros((1, 4)), np.ones((1, 4))
    ok_front = np.array([[0.2, 0.8], [0.5, 0.3]])

    def refused(code, word, fn):
        import bot7_amd
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    refused(-1, "not sorted", lambda: ctx.ehvi_compute(mu, var, mu, var, ok_front[::-1], [1.0, 1.0]))
    refused(-1, "dominated", lambda: ctx.ehvi_compute(mu, var, mu, var, [[0.2, 0.3], [0.5, 0.8]], [1.0, 1.0]))
    refused(-1, "strictly inside", lambda: ctx.ehvi_compute(mu, var, mu, var, [[0.2, 1.0]], [1.0, 1.0]))
    refused(-1, "not finite", lambda: ctx.ehvi_compute(mu, var, mu, var, ok_front, [np.inf, 1.0]))
    big = np.zeros((R.SMAX + 1, 4))
    refused(-1, "hyper samples", lambda: ctx.ehvi_compute(big, big + 1.0, mu, var, ok_front, [1.0, 1.0]))
    k = np.arange(R.PMAX + 1, dtype=np.float64)
    refused(-1, "front of %d points" % (R.PMAX + 1), lambda: ctx.ehvi_compute(mu, var, mu, var, np.stack([k / 1000, 1 - k / 1000], 1), [2.0, 2.0]))
    assert ctx.ehvi_compute(np.zeros((1, 0)), np.zeros((1, 0)), np.zeros((1, 0)), np.zeros((1, 0)), ok_front, [1.0, 1.0]).shape == (0,)


# ---- 2. the kept posterior = the per-sample predict, bit for bit, on every route ---------------------------------------------------
def problem(N, d, M, S, seed, dup=0):
    """tests/test_gpu_believer_routes.py's problem; dup > 0 repeats the first dup observations at the end."""
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    if dup:
        X[N - dup:] = X[:dup]
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rng.standard_normal(N)
    if dup:
        y[N - dup:] = y[:dup]
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.05 * s} for s in range(S)]
    return X, y.reshape(-1, 1), Xc, hyps


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def _diag_context():
    import bot7_amd
    return bot7_amd.Context(0, lib="diag")


@pytest.fixture(scope="module")
def dctx():
    """The diagnostic build: the route switches (B7_POTRF_SCHED) are read there only."""
    c = _diag_context()
    yield c
    c.close()


def _counted_posterior(c, hyps):
    c.profile_enable(True)
    try:
        c.profile_reset()
        rep = c.eval_posterior(hyps, want_report=True)
        counts = {ph: c.profile_get(ph)[1] for ph in ("kxx", "ksx", "post", "kpost")}
    finally:
        c.profile_enable(False)
    return rep, counts


def check_kept(c, hyps, counts_ok, label):
    """eval_posterior's report equals eval_nominate's, the kept posterior of every sample equals gp_predict_hyp's download bit for
    bit, and eval_posterior leaves no accumulator."""
    import bot7_amd
    M = c.grid_shape()[0]
    _, _, want_rep = c.eval_nominate(hyps, score="cb", want_report=True)
    rep, counts = _counted_posterior(c, hyps)
    assert counts_ok(counts), (label, counts)
    assert rep["jitter"].tobytes() == want_rep["jitter"].tobytes() and np.array_equal(rep["info"], want_rep["info"]), label
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        c.score_finish(1.0)
    assert e.value.code == -4
    kept = [c.posterior_get(s) for s in range(len(hyps))]
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        c.posterior_get(len(hyps))
    assert e.value.code == -1
    for s, h in enumerate(hyps):
        out = c.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], download=True)
        assert kept[s][0].shape == (M,) and kept[s][0].tobytes() == out["mean"][:, 0].tobytes(), (label, s)
        assert kept[s][1].tobytes() == out["var"].tobytes(), (label, s)
        assert out["jitter"] == rep["jitter"][s] and out["info"] == rep["info"][s]
    c.eval_posterior(hyps)
    assert [c.posterior_get(s)[1].tobytes() for s in range(len(hyps))] == [k[1].tobytes() for k in kept]    # the same call twice
    return rep


ROUTE_COUNTS = {"small": lambda n, S: n["kpost"] == 1 and n["post"] == 0,
                "B": lambda n, S: n["kxx"] == 1 and n["post"] == 1 and n["kpost"] == 0,
                "C": lambda n, S: n["kxx"] == 1 and n["post"] >= S and n["ksx"] >= S and n["kpost"] == 0,
                "D": lambda n, S: n["kxx"] == S and n["post"] == S and n["kpost"] == 0}


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("route,S", [("small", 3), ("small", 1), ("B", 3), ("B", 1), ("C", 3), ("D", 3)])
def test_kept_posterior_is_the_per_sample_predict(dctx, monkeypatch, route, S, kernel):
    """The routes of eval_enqueue, told apart by their phase counters: the one-launch small route (N = 40, d = 3: one "kpost"
    phase), side-by-side fits with the batched K* (N = 150, d = 5: one "kxx", one "post"), the same fits with per-sample
    posteriors because the workspace (128 KiB) does not hold K* ("post" >= S), and a context on the launch schedule
    (B7_POTRF_SCHED=1) that fits one sample after the other in its own slot ("kxx" == S); S = 1 takes the in-turn fit on the general
    layout.  M = 200, both covariance kernels."""
    N, d = (40, 3) if route == "small" else (150, 5)
    X, y, Xc, hyps = problem(N, d, 200, S, 4)
    c = dctx
    if route == "D":
        monkeypatch.setenv("B7_POTRF_SCHED", "1")
        c = _diag_context()
        monkeypatch.delenv("B7_POTRF_SCHED")
    try:
        stage(c, X, y, Xc, kernel)
        if route == "C":
            c.set_workspace(128 << 10)
        counts_ok = (lambda n: ROUTE_COUNTS[route](n, S)) if S > 1 or route == "small" else (lambda n: n["kxx"] == 1 and n["kpost"] == 0)
        rep = check_kept(c, hyps, counts_ok, "%s S=%d %s" % (route, S, kernel))
        assert not rep["jitter"].any() and not rep["info"].any()
    finally:
        if route == "C":
            c.set_workspace(4 << 30)
        if route == "D":
            c.close()


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("N,d,S", [(40, 3, 3), (150, 5, 3)])
def test_kept_posterior_through_the_jitter_redo(dctx, N, d, S, kernel):
    """Duplicated observations with noise = 0 under the second sample: the posteriors are redone through the jitter schedule, and
    what is kept is the redo's; jitter_out / info_out are b7_eval_nominate's."""
    X, y, Xc, hyps = problem(N, d, 200, S, 9 if N == 40 else 2, dup=3)
    hyps[1] = dict(hyps[1], noise=0.0)
    stage(dctx, X, y, Xc, kernel)
    rep = check_kept(dctx, hyps, lambda n: True, "redo N=%d %s" % (N, kernel))
    print("redo N=%d %s: jitter %s info %s" % (N, kernel, rep["jitter"].tolist(), rep["info"].tolist()))
    assert rep["jitter"][1] > 0.0 and rep["info"][1] > 0
    assert not np.delete(rep["jitter"], 1).any() and not np.delete(rep["info"], 1).any()


def test_kept_posterior_respects_the_gp_opts(ctx):
    """var_with_noise and var_clamp reach the kept posterior exactly as they reach b7_gp_predict_hyp."""
    X, y, Xc, hyps = problem(40, 3, 200, 2, 4)
    stage(ctx, X, y, Xc)
    ctx.eval_posterior(hyps)
    plain = ctx.posterior_get(1)[1]
    try:
        ctx.gp_set_opts(var_with_noise=True, var_clamp=True, var_min=0.5 * float(np.median(plain)))
        ctx.eval_posterior(hyps)
        for s, h in enumerate(hyps):
            kept = ctx.posterior_get(s)
            out = ctx.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], download=True)
            assert kept[0].tobytes() == out["mean"][:, 0].tobytes() and kept[1].tobytes() == out["var"].tobytes()
        assert ctx.posterior_get(1)[1].tobytes() != plain.tobytes() and ctx.posterior_get(1)[1].min() >= 0.5 * float(np.median(plain))
    finally:
        ctx.gp_set_opts()


# ---- 3. the nomination end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx2():
    import bot7_amd
    c = bot7_amd.Context(0)
    yield c
    c.close()


def two_objective_problem(N=30, d=2, M=333, seed=11):
    from harness import benchmarks as B
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    Y = B.two_spheres(X)
    hyps = []
    for col, S in ((0, 3), (1, 2)):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, 0.5 + 0.25 * s), "amp": amp * (1.0 + 0.3 * s), "noise": 1e-4 * amp,
                      "mean": float(np.mean(Y[:, col])) + 0.02 * s} for s in range(S)])
    return X, Y, Xc, hyps[0], hyps[1]


def kept(c, S):
    got = [c.posterior_get(s) for s in range(S)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def test_nomination_end_to_end(ctx, ctx2):
    """Two contexts, N = 30, d = 2, M = 333, S1 = 3, S2 = 2, responses from two_spheres.  The accumulator of b7_ehvi_nominate equals
    b7_ehvi_compute on the downloaded posteriors bit for bit and is within test 1's bar of the 50-digit marginal; the nominee is
    score:max(1) of it and its value is within the bar of the reference's maximum; other == ctx; the same call twice; the grid in
    two halves gives the same per-row bits.  On an MI355X: worst error / bar 0.0018."""
    from bot7_amd import _lib
    X, Y, Xc, h1, h2 = two_objective_problem()
    M = len(Xc)
    ref = np.array([0.9, 0.9])
    front, rows = _lib.pareto_front2(Y, ref)
    assert 2 <= len(front) < len(Y)
    stage(ctx, X, Y[:, :1], Xc)
    stage(ctx2, X, Y[:, 1:], Xc)
    ctx.eval_posterior(h1)
    ctx2.eval_posterior(h2)
    val, idx = ctx.ehvi_nominate(ctx2, front, ref)
    v2, i2, acc = ctx.score_finish(1.0, download=True)
    mu1, var1 = kept(ctx, 3)
    mu2, var2 = kept(ctx2, 2)
    want = ctx.ehvi_compute(mu1, var1, mu2, var2, front, ref)
    assert acc.tobytes() == want.tobytes()
    assert idx == i2 == R.nominee_ref(acc) + 1 and np.float64(val).tobytes() == np.float64(v2).tobytes() == acc[idx - 1].tobytes()
    worst = bar_ratio(acc, mu1, var1, mu2, var2, front, ref)
    hi, lo = R.ehvi_mp(mu1, var1, mu2, var2, front, ref)
    best = int(np.argmax(hi))
    bar_best = E.gp_bar(R.err_vs_mp(R.ehvi_numpy(mu1, var1, mu2, var2, front, ref), hi, lo)[[idx - 1, best]].max(),
                        R.empty_scale_mp(mu1, var1, mu2, var2, ref)[[idx - 1, best]].max())
    print("ehvi nomination: worst error / bar %.3g; nominee %d (reference's %d), value %.6g against %.6g" % (worst, idx, best + 1, val, hi[best]))
    # the values, not the indices, so a near-tie cannot fail: acc[idx] >= acc[best] and truth[best] >= truth[idx] put val - truth[best]
    # between -bar[best] and +bar[idx] whenever both rows are within their bars
    assert worst <= 1.0 and abs((val - hi[best]) - lo[best]) <= bar_best
    # the same call twice
    assert ctx.ehvi_nominate(ctx2, front, ref) == (val, idx) and ctx.score_finish(1.0, download=True)[2].tobytes() == acc.tobytes()
    # the second context's posterior is untouched and its stream goes on
    assert kept(ctx2, 2)[0].tobytes() == mu2.tobytes()
    # other == ctx: the same posterior for both objectives
    vs, is_ = ctx.ehvi_nominate(ctx, front, ref)
    same = ctx.score_finish(1.0, download=True)[2]
    assert same.tobytes() == ctx.ehvi_compute(mu1, var1, mu1, var1, front, ref).tobytes() and is_ == R.nominee_ref(same) + 1
    # an empty front: Psi1(r1) Psi2(r2), finite everywhere
    v0, i0 = ctx.ehvi_nominate(ctx2, np.zeros((0, 2)), ref)
    acc0 = ctx.score_finish(1.0, download=True)[2]
    assert np.isfinite(acc0).all() and (acc0 >= acc * (1.0 - 1e-12)).all() and bar_ratio(acc0, mu1, var1, mu2, var2, np.zeros((0, 2)), ref) <= 1.0
    # grid-size independence: the two halves of the grid give the rows' bits
    for lo_, hi_ in ((0, 170), (170, M)):
        ctx.grid_upload(Xc[lo_:hi_])
        ctx2.grid_upload(Xc[lo_:hi_])
        ctx.eval_posterior(h1)
        ctx2.eval_posterior(h2)
        ctx.ehvi_nominate(ctx2, front, ref)
        assert ctx.score_finish(1.0, download=True)[2].tobytes() == acc[lo_:hi_].tobytes(), (lo_, hi_)


# ---- 4. state and refusals ----------------------------------------------------------------------------------------------------------
def test_state_and_refusals(ctx, ctx2):
    import bot7_amd
    X, Y, Xc, h1, h2 = two_objective_problem(M=64)
    ref = np.array([0.9, 0.9])
    front = bot7_amd._lib.pareto_front2(Y, ref)[0]

    def refused(code, word, fn):
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    stage(ctx, X, Y[:, :1], Xc)
    stage(ctx2, X, Y[:, 1:], Xc)
    # no kept posterior, on either side
    refused(-4, "no kept posterior", lambda: ctx.posterior_get(0))
    refused(-4, "first objective", lambda: ctx.ehvi_nominate(ctx2, front, ref))
    ctx.eval_posterior(h1)
    refused(-4, "second objective", lambda: ctx.ehvi_nominate(ctx2, front, ref))
    ctx2.eval_posterior(h2)
    val, idx = ctx.ehvi_nominate(ctx2, front, ref)
    # a non-canonical front, a bad reference point: by code and message, and nothing moved
    refused(-1, "not sorted", lambda: ctx.ehvi_nominate(ctx2, front[::-1], ref))
    dominated = np.array([[0.1, 0.2], [0.3, 0.4]])
    refused(-1, "dominated", lambda: ctx.ehvi_nominate(ctx2, dominated, ref))
    refused(-1, "strictly inside", lambda: ctx.ehvi_nominate(ctx2, np.array([[0.1, 0.95]]), ref))
    refused(-1, "not finite", lambda: ctx.ehvi_nominate(ctx2, front, [np.nan, 1.0]))
    assert ctx.ehvi_nominate(ctx2, front, ref) == (val, idx)
    # mismatched M
    ctx2.grid_upload(Xc[:40])
    refused(-4, "second objective", lambda: ctx.ehvi_nominate(ctx2, front, ref))          # the grid change forgot it
    ctx2.eval_posterior(h2)
    refused(-1, "40 rows, this one 64", lambda: ctx.ehvi_nominate(ctx2, front, ref))
    # a grid change forgets the kept posterior: upload, removal; so does new data
    ctx.grid_remove(3)
    refused(-4, "no kept posterior", lambda: ctx.posterior_get(0))
    ctx.eval_posterior(h1)
    ctx.gp_set_data(X[:20], Y[:20, :1])
    refused(-4, "first objective", lambda: ctx.ehvi_nominate(ctx2, front, ref))
    # two response columns
    ctx.gp_set_data(X, Y)
    refused(-5, "2 response columns", lambda: ctx.eval_posterior(h1))
    ctx.gp_set_data(X, Y[:, :1])
    refused(-1, "S >= 1", lambda: ctx.eval_posterior([]))
    # more samples than the kernel takes are refused by the nomination, not by the posterior
    many = [dict(h1[0], amp=h1[0]["amp"] * (1.0 + 0.01 * s)) for s in range(R.SMAX + 1)]
    ctx.eval_posterior(many)
    refused(-1, "hyper samples", lambda: ctx.ehvi_nominate(ctx, front, ref))
    # a group member
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(Xc)
        g.gp_set_data(X, Y[:, :1])
        refused(-4, "group", lambda: g.members[0].eval_posterior(h1))
        ctx.grid_upload(Xc[:32])
        ctx.eval_posterior(h1)
        refused(-4, "group", lambda: ctx.ehvi_nominate(g.members[0], front, ref))
    finally:
        g.close()


# ---- 5. the loop ----------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name, lo=0.0, hi=1.0):
        self.name, self.min, self.max, self.size = name, lo, hi, 1


def test_the_bot_with_two_objectives(ctx):
    """harness bayesopt with config.bot.objectives on two_spheres, d = 2, 256 Sobol candidates, 3 random + 6 model-based trials,
    S = 3, the slice sampler: the hypervolume against a fixed reference point never decreases; every model-based nominee is the
    arg-max of the score recomputed (b7_ehvi_compute) from that trial's downloaded posteriors; both resident grids stay
    row-identical."""
    import bot7_amd
    from bot7_amd import _lib
    from bot7_amd.grids.abstract import DeviceGrid
    from harness import benchmarks as B, bots
    mcfg ={"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    ref = [1.2, 1.2]
    cfg = {"bot": {"verbose": 0, "budget": 9, "nInitial": 3, "nSamples": 3, "seed": 2, "objectives": {"ref": ref, "model": dict(mcfg, seed=6)}},
           "grid": {"type": "sobol", "size": 256, "dims": 2}, "score": {"type": "expected_hypervolume_improvement"}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 256, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    bot = bots.bayesopt(B.two_spheres, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})
    hv = []
    try:
        for t in range(9):
            before = np.asarray(bot.candidates).copy()
            x, y = bot.run_trial()
            bot.update_best(x, y)
            assert np.asarray(y).shape == (1, 2)
            front, _ = _lib.pareto_front2(bot.responses, ref)
            hv.append(_lib.hypervolume2(front, ref))
            assert hv[-1] == bot.best["hv"] and len(front) == len(bot.best["front"])
            if t < 3:
                assert bot.objective2 is None or bot.objective2["grid"] is None
                continue
            last, o2 = bot.last_objectives, bot.objective2
            # both grids lost the nominee; before that they held the same rows, and the kept posteriors were of those rows
            assert np.array_equal(before[last["index"] - 1], x)
            assert np.array_equal(ctx.grid_download(), np.asarray(bot.candidates)) and np.array_equal(o2["ctx"].grid_download(), np.asarray(bot.candidates))
            # the nominee again, from this trial's hyper samples on two fresh stagings of the grid as it stood
            n = t
            want_front, _ = _lib.pareto_front2(bot.responses[:n], ref)
            assert np.array_equal(last["front"], want_front)
            post = []
            for c, hyps, col in ((ctx, last["hyps"], 0), (o2["ctx"], last["hyps2"], 1)):
                c.grid_upload(before)
                c.gp_set_data(bot.observed[:n], bot.responses[:n, col:col + 1])
                c.eval_posterior(hyps)
                post.append(kept(c, 3))
            score = ctx.ehvi_compute(post[0][0], post[0][1], post[1][0], post[1][1], last["front"], ref)
            assert last["index"] == R.nominee_ref(score) + 1 and last["value"] == score[last["index"] - 1]
            assert ctx.ehvi_nominate(o2["ctx"], last["front"], ref) == (last["value"], last["index"])
            # put the grids back as the bot left them
            for c in (ctx, o2["ctx"]):
                c.grid_remove(last["index"])
            bot.candidates = DeviceGrid(np.asarray(bot.candidates), ctx, ctx.grid_version)
            o2["grid"] = DeviceGrid(np.asarray(bot.candidates), o2["ctx"], o2["ctx"].grid_version)
        print("two objectives: hypervolume per trial %s, front of %d" % (["%.4f" % h for h in hv], len(bot.best["front"])))
        assert all(b >= a for a, b in zip(hv, hv[1:])) and hv[-1] > hv[2]
    finally:
        if bot.objective2 is not None:
            bot.objective2["ctx"].close()
