"""Log-space expected improvement (B7_SCORE_LOGEI) on the device, through every route that takes a score kind, against 50-digit
arithmetic (tests/_logei_ref.py).  Bar everywhere: |err| <= 1e-13 * max(1, |ref|).

Achieved on an MI355X: 1.9e-15 on single scores, 2.3e-15 on marginals over three hyper samples (each test prints its figure)."""
import functools

import mpmath
import numpy as np
import pytest

import bot7_amd
from conftest import make_network, make_problem
from harness import benchmarks as B
from harness import bots

import _logei_ref as R

pytestmark = pytest.mark.gpu
INF = np.inf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


# ---- 1. values --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _value_rows():
    rng = np.random.default_rng(4096)
    mu = rng.uniform(-2.0, 2.0, 4096)
    sigma = np.exp(rng.uniform(np.log(1e-6), 0.0, 4096))
    var = sigma * sigma
    return mu, var, {xi: R.logei_mp(mu, var, 0.0, xi) for xi in (0.0, 0.5)}


def test_values_against_50_digits(ctx):
    """b7_logei_compute, M = 4096, c = 1: mu in [-2, 2], sigma log-uniform in [1e-6, 1], fmin = 0, xi in {0, 0.5} (z from about
    -2e6 to +2e6), against mpmath on the exact inputs; then c = 3 columns against log(mean_k EI_k).  Bar 1e-13 * max(1, |ref|).
    Measured on an MI355X: c = 1 worst 1.9e-15 (at z = -38.6), c = 3 worst 1.1e-15; the marginal of test 4 worst 2.3e-15 (the scipy
    restatement of the formula on the host: 1.1e-15)."""
    mu, var, refs = _value_rows()
    for xi, ref in refs.items():
        got = ctx.logei_compute(mu, var, [0.0], xi)
        err = R.scaled_errors(got, ref)
        z = (-mu - xi) / np.sqrt(var)
        print("LogEI device xi %.1f: worst scaled error %.3g at z = %.6g (z in [%.3g, %.3g])" % (xi, err.max(), z[err.argmax()], z.min(), z.max()))
        assert np.isfinite(got).all()
        assert err.max() <= R.BAR, "xi %.1f: %.3g at z = %g" % (xi, err.max(), z[err.argmax()])
    rng = np.random.default_rng(3)
    M, c = 1024, 3
    mu3 = rng.uniform(-2.0, 2.0, (M, c))
    v3 = np.exp(rng.uniform(np.log(1e-6), 0.0, M)) ** 2
    fm = np.array([0.0, -0.5, 0.25])
    got = ctx.logei_compute(mu3, v3, fm, 0.0)
    err = R.scaled_errors(got, R.logei_mean_mp(mu3, v3, fm, 0.0))
    print("LogEI device c = 3: worst scaled error %.3g" % err.max())
    assert err.max() <= R.BAR


def test_edge_rows_are_exact(ctx):
    """var in {0, -1, NaN}, mu NaN, imprv in {< 0, 0, > 0} at var == 0: NaN-ness and +-inf as score.hip's header says, the finite
    row against log(imprv); z = +inf at sigma > 0 gives log(imprv) as well."""
    nan = np.nan
    mu = np.array([3.0, 0.0, -2.0, 0.0, 0.0, nan, nan, -1e300, 0.5])
    var = np.array([0.0, 0.0, 0.0, -1.0, nan, 1.0, 0.0, 1e-320, 1.0])
    got = ctx.logei_compute(mu, var, [0.0], 0.0)
    assert got[0] == -INF and got[1] == -INF
    assert abs(got[2] - np.log(2.0)) <= 2 ** -52
    assert np.isnan(got[3:7]).all()
    assert abs(got[7] - np.log(1e300)) <= 2 ** -52 * np.log(1e300)
    assert np.isfinite(got[8])
    # the same rows as one of three columns: a NaN column (or variance) poisons its row, the others stay finite
    m3 = np.stack([mu, np.full(9, 0.5), np.full(9, 0.5)], axis=1)
    g3 = ctx.logei_compute(m3, np.where(np.isnan(var) | (var < 0), var, 1.0), [0.0, 0.0, 0.0], 0.0)
    assert np.isnan(g3[3:7]).all() and np.isfinite(g3[[0, 1, 2, 8]]).all()


def test_far_tail_is_never_nan(ctx):
    """z in [-1e12, -1e7], where t sqrt(pi/2) erfcx(t/sqrt2) is within an ulp of 1 and log1p of its negative is NaN or -inf in turns:
    the device's tail (t >= 1e5: -2 log t + log1p(-3/t^2)) is finite, strictly decreasing in t at fixed sigma, and within the bar of
    the 50-digit value; the arg-max over such rows is the smallest t, not the first NaN.  sigma = 1e-8 with |imprv| in [0.1, 1e4] is
    what a zero var_min leaves next to an observation.  Beyond t ~ 1.3e154 the score is -inf."""
    t = R.far_tail_t(np.random.default_rng(7), 2048)
    for sigma in (1.0, 1e-8):
        var = np.full(t.size, sigma * sigma)
        mu = (t * sigma)[::-1].copy()                  # decreasing t down the rows: row 1 is the WORST candidate
        tt = mu / np.sqrt(var)
        assert tt.min() >= 9.9e6 and tt.max() <= 1.01e12
        got = ctx.logei_compute(mu, var, [0.0], 0.0)
        assert np.isfinite(got).all()
        assert (np.diff(got[np.diff(tt, append=0.0) < 0]) > 0).all()
        err = R.scaled_errors(got[::16], R.logei_mp(mu[::16], var[::16], 0.0, 0.0))
        print("LogEI device, far tail, sigma %g: worst scaled error %.3g" % (sigma, err.max()))
        assert err.max() <= R.BAR
        val, idx = ctx.argmax(got)
        assert idx == int(np.argmin(tt)) + 1 and idx != 1 and val == got[idx - 1]
    out = ctx.logei_compute(np.array([1e13, 1e100, 1e154, 1e155, 1e300]), np.ones(5), [0.0], 0.0)
    assert not np.isnan(out).any() and np.isfinite(out[:3]).all() and (out[3:] == -INF).all() and (np.diff(out[:3]) < 0).all()
    # S = 2 samples of +inf (var = +inf) marginalise to +inf, not NaN; -inf with -inf stays -inf
    two = ctx.logei_compute(np.zeros((3, 2)), np.array([INF, 0.0, 1.0]), [0.0, 0.0], 0.0)
    assert two[0] == INF and two[1] == -INF and np.isfinite(two[2])


# ---- 2. the plateau: EI says nothing, LogEI ranks -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plateau():
    rng = np.random.default_rng(2000)
    mu = rng.uniform(1.0, 2.0, 4096)
    var = rng.uniform(1e-3, 1e-2, 4096) ** 2
    ref = R.logei_mp(mu, var, 0.0, 0.0)
    return mu, var, ref


def test_plateau_ei_is_silent_logei_ranks(ctx):
    """mu in [1, 2], sigma in [1e-3, 1e-2], fmin = 0: z in [-2000, -100].  EI is exactly 0 everywhere and its arg-max is row 1 (the
    statement of the problem); log EI's arg-max is the 50-digit one (top-2 gap checked > 1e-6)."""
    mu, var, ref = _plateau()
    z = -mu / np.sqrt(var)
    assert z.max() < -100.0 and z.min() >= -2000.0
    ei = ctx.ei_compute(mu, var, [0.0], 0.0)
    assert not ei.any()
    assert ctx.argmax(ei) == (0.0, 1)
    with mpmath.workdps(R.DPS):
        order = sorted(range(len(ref)), key=lambda j: ref[j], reverse=True)
        gap = float(ref[order[0]] - ref[order[1]])
    assert gap > 1e-6
    lei = ctx.logei_compute(mu, var, [0.0], 0.0)
    val, idx = ctx.argmax(lei)
    assert idx == order[0] + 1 and idx != 1
    assert abs(val - float(ref[order[0]])) <= R.BAR * abs(float(ref[order[0]]))


# ---- 3. where EI is sound the two agree ---------------------------------------------------------------------------------------
def test_agrees_with_ei_where_ei_is_sound(ctx):
    """z in [-3, 5]: exp(log EI) within 1e-6 * max(sigma, |imprv|) of b7_ei_compute (the A&S bound the EI tests use), same arg-max."""
    rng = np.random.default_rng(35)
    M = 4096
    z = rng.uniform(-3.0, 5.0, M)
    sigma = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), M))
    var = sigma * sigma
    mu = -(z * np.sqrt(var))
    zz = -mu / np.sqrt(var)
    assert zz.min() >= -3.0 - 1e-9 and zz.max() <= 5.0 + 1e-9
    ei = ctx.ei_compute(mu, var, [0.0], 0.0)
    lei = ctx.logei_compute(mu, var, [0.0], 0.0)
    assert np.all(np.abs(np.exp(lei) - ei) <= 1e-6 * np.maximum(np.sqrt(var), np.abs(mu)))
    assert ctx.argmax(ei)[1] == ctx.argmax(lei)[1]


# ---- 4. one call = the loop, bit for bit -------------------------------------------------------------------------------------
def _hyps(hyp, S):
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.25 * s), amp=hyp["amp"] * (1.0 + 0.1 * s)) for s in range(S)]


def _loop(c, X_obs, Y, hyps, fmin, xi, kind="logei"):
    """{b7_gp_predict_hyp; b7_score_logei} x S + b7_score_finish(S) -> value, index, scores, [(mean, var)] per sample"""
    c.gp_set_data(X_obs, Y)
    mv = []
    for s, h in enumerate(hyps):
        out = c.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], download=True)
        mv.append((out["mean"][:, 0].copy(), out["var"].copy()))
        if s == 0:
            c.score_reset()
        (c.score_logei if kind == "logei" else c.score_ei)(fmin, xi)
    val, idx, scores = c.score_finish(float(len(hyps)), download=True)
    return val, idx, scores, mv


def _objective(X):
    return np.sin(3.0 * X).sum(axis=1, keepdims=True)


@pytest.mark.parametrize("N,d,M,S", [(24, 3, 2048, 1), (24, 3, 2048, 3), (150, 5, 2048, 3)])
def test_eval_nominate_is_the_per_sample_loop_bit_for_bit(ctx, orc, N, d, M, S):
    """b7_eval_nominate(B7_SCORE_LOGEI) against the separate calls: equal winner, equal best_val bits, equal accumulator bits (the
    first two shapes: small-problem kernels + the fused kernel's LogEI instance; the third: general schedule + score_batch_kernel; the phase
    counters say which ran), and the
    scores equal logsumexp_s(logEI_s) - log S in 50 digits from the downloaded mean / variance, within the bar."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, d, N, M, _objective)
    hyps, fmin = _hyps(hyp, S), [float(Y.min())]
    ctx.grid_upload(X_hid)
    val0, idx0, sc0, mv = _loop(ctx, X_obs, Y, hyps, fmin, 0.0)
    ctx.gp_set_data(X_obs, Y)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        val1, idx1, rep = ctx.eval_nominate(hyps, score="logei", fmin=fmin, want_report=True)
        n_score, n_argmax = ctx.profile_get("score")[1], ctx.profile_get("argmax")[1]
    finally:
        ctx.profile_enable(False)
    # which kernels ran: the fused launch is one "score" phase and no "argmax" phase (score, division, arg-max and record in
    # score_finish_slot_kernel<B7_SCORE_LOGEI>); the batch route is one "score" phase (score_batch_kernel, all S samples) and one "argmax"
    # phase (finish_kernel); the per-sample fall-back would show S "score" phases
    assert (n_score, n_argmax) == ((1, 0) if N <= 128 else (1, 1)), (n_score, n_argmax)
    _, _, sc1 = ctx.score_finish(1.0, download=True)      # a log accumulator: a - log(1) = a
    assert not rep["jitter"].any() and not rep["info"].any()
    assert idx1 == idx0 and _bits([val1]) == _bits([val0]) and _bits(sc1) == _bits(sc0)
    assert _bits([val1]) == _bits([sc1[idx1 - 1]])
    ref = R.logmeanexp_mp([R.logei_mp(m, v, fmin[0], 0.0) for m, v in mv])
    err = R.scaled_errors(sc1, ref)
    print("LogEI marginal N %d S %d: worst scaled error %.3g" % (N, S, err.max()))
    assert err.max() <= R.BAR
    assert ctx.eval_nominate(hyps, score="logei", fmin=fmin, global_row_offset=1000)[1] == idx0 + 1000


# ---- 5. end to end on the plateau ----------------------------------------------------------------------------------------------
def test_nomination_on_the_plateau(ctx, orc):
    """(N, d, M) = (24, 3, 2048), responses of size 1e-2 and tradeoff = 1.0: every z < -40, phi underflows, EI nominates index 1 with
    value 0; LogEI nominates the 50-digit winner."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 2048, lambda X: 1e-2 * _objective(X))
    hyps, fmin = _hyps(hyp, 3), [float(Y.min())]
    ctx.grid_upload(X_hid)
    _, _, _, mv = _loop(ctx, X_obs, Y, hyps, fmin, 1.0)
    assert max(float((((fmin[0] - m) - 1.0) / np.sqrt(v)).max()) for m, v in mv) < -40.0
    ctx.gp_set_data(X_obs, Y)
    assert ctx.eval_nominate(hyps, score="ei", fmin=fmin, tradeoff=1.0) == (0.0, 1)
    val, idx = ctx.eval_nominate(hyps, score="logei", fmin=fmin, tradeoff=1.0)
    ref = R.logmeanexp_mp([R.logei_mp(m, v, fmin[0], 1.0) for m, v in mv])
    with mpmath.workdps(R.DPS):
        order = sorted(range(len(ref)), key=lambda j: ref[j], reverse=True)
        gap = float(ref[order[0]] - ref[order[1]])
    assert gap > 10.0 * R.BAR * abs(float(ref[order[0]]))    # the winner is decided well outside the bar on either score
    assert idx == order[0] + 1 and np.isfinite(val)
    assert abs(val - float(ref[order[0]])) <= R.BAR * abs(float(ref[order[0]]))


# ---- 6. every route ------------------------------------------------------------------------------------------------------------
def test_group_of_two_virtual_ranks(ctx, orc):
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 2048, _objective)
    hyps, fmin = _hyps(hyp, 3), [float(Y.min())]
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    val, idx = ctx.eval_nominate(hyps, score="logei", fmin=fmin)
    _, _, sc = ctx.score_finish(1.0, download=True)
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(X_hid)
        g.gp_set_data(X_obs, Y)
        gval, gidx = g.eval_nominate(hyps, score="logei", fmin=fmin)
        gsc = np.concatenate([m.score_finish(1.0, download=True)[2] for m in g.members])
    finally:
        g.close()
    assert gidx == idx and _bits([gval]) == _bits([val]) and _bits(gsc) == _bits(sc)


def test_blr_marginalised_heads(ctx, orc):
    """b7_blr_eval_nominate_marg, S = 2 heads on a 5 -> 16 -> 16 tanh basis, N = 32, M = 2048, against the per-head loop
    {b7_blr_fit_x; b7_blr_predict; b7_score_logei} x 2 + b7_score_finish(2).  The one-launch heads and the per-head fit factor the
    same 16 x 16 system by different schedules, and the means are summed in different orders: mean and sigma of the two routes
    differ by rounding amplified by the system's condition, taken as 1e-10 of the response scale at most (cond <= 1e5 at eps 1e-16
    with a decade to spare).  d logEI / d mu = -Phi/(sigma h) and d logEI / d sigma are bounded by (1 + |z|)^2 / sigma (h'/h = Phi/h
    <= 1 + |z| for z < 0 and <= 1 above), hence the bar below on top of the arithmetic's own 1e-13 max(1, |ref|)."""
    d, N, M = 5, 32, 2048
    W, b = make_network(d, (16, 16), seed=11)
    X_obs, Y, X_hid, _ = make_problem(ctx, orc, d, N, M, lambda X: np.sin(3 * X.sum(axis=1, keepdims=True)))
    al, be = [1.0, 2.0], [1.0 / (1e-2 * float(np.var(Y))), 1.0 / (2e-2 * float(np.var(Y)))]
    mn, fmin = [float(np.mean(Y))] * 2, [float(Y.min())]
    ctx.grid_upload(X_hid)
    bound = np.zeros(M)
    for s in range(2):
        ctx.blr_fit_x(W, b, "Tanh", X_obs, Y, al[s], be[s], mn[s])
        ctx.blr_basis(W, b, "Tanh")
        mu, var = ctx.blr_predict()
        sg = np.sqrt(var)
        z = (fmin[0] - mu[:, 0]) / sg
        bound = np.maximum(bound, 2e-10 * max(1.0, float(np.abs(Y).max())) * (1.0 + np.abs(z)) ** 2 / sg)
        if s == 0:
            ctx.score_reset()
        ctx.score_logei(fmin, 0.0)
    val0, idx0, sc0 = ctx.score_finish(2.0, download=True)
    val1, idx1, jit = ctx.blr_eval_nominate_marg(W, b, "Tanh", X_obs, Y, al, be, mn, score="logei", fmin=fmin)
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    assert jit == 0.0 and np.isfinite(sc1).all()
    tol = bound + R.BAR * np.maximum(1.0, np.abs(sc0))
    assert np.all(np.abs(sc1 - sc0) <= tol)
    # the winner: a row can beat the loop's winner on the other route only if its score is within the two rows' bars of it.  For
    # this seed no row is, so the two routes must name the same candidate
    rivals = np.flatnonzero(sc0 + tol >= sc0[idx0 - 1] - tol[idx0 - 1])
    top = np.sort(sc0)[-2:]
    print("LogEI BLR marg: worst |diff| %.3g, bound max %.3g (median %.3g), top-2 gap %.3g, rivals within their bars %d"
          % (np.abs(sc1 - sc0).max(), bound.max(), np.median(bound), top[1] - top[0], rivals.size))
    assert list(rivals) == [idx0 - 1], "the fixed seed no longer decides the winner outside the bars"
    assert idx1 == idx0
    assert val1 == sc1[idx1 - 1]
    # one head, written (not accumulated): b7_blr_eval_nominate
    v, i = ctx.blr_eval_nominate(W, b, "Tanh", X_obs, Y, al[0], be[0], mn[0], score="logei", fmin=fmin)
    _, _, sc = ctx.score_finish(1.0, download=True)
    assert np.isfinite(sc).all() and v == sc[i - 1] == sc.max()


def test_mixing_linear_and_log_accumulators_is_a_state_error(ctx, orc):
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 300, _objective)
    fmin = [float(Y.min())]
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    ctx.gp_predict_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
    for first, second in ((ctx.score_logei, ctx.score_ei), (ctx.score_ei, ctx.score_logei),
                          (ctx.score_logei, lambda f, x: ctx.score_cb())):
        ctx.score_reset()
        first(fmin, 0.0)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            second(fmin, 0.0)
        assert e.value.code == -4
        first(fmin, 0.0)                       # the accumulator is still usable with its own kind
    ctx.score_reset()                          # ... and a reset frees it for the other
    ctx.score_ei(fmin, 0.0)
    # a reset with no add at all is a linear accumulator of zeros, as before
    ctx.score_reset()
    assert not ctx.score_finish(1.0, download=True)[2].any()


def test_jitter_redo_keeps_the_loops_winner(ctx, orc):
    """Duplicated observations, zero noise: the plain factorisation fails, the nomination is redone through the jitter schedule;
    under LogEI it returns what the per-sample loop returns, bit for bit."""
    X = orc.c.sobol(40, 3, 1)
    X[7] = X[3]
    Y = _objective(X)
    X_hid = orc.c.sobol(2048, 3, 100)
    good = dict(lenscale_sq=np.full(3, 0.4), amp=1.0, noise=1e-3, mean=0.1)
    hyps = [good, dict(good, noise=0.0, mean=0.0), dict(good, amp=1.3)]
    fmin = [float(Y.min())]
    ctx.grid_upload(X_hid)
    val0, idx0, sc0, _ = _loop(ctx, X, Y, hyps, fmin, 0.0)
    ctx.gp_set_data(X, Y)
    val1, idx1, rep = ctx.eval_nominate(hyps, score="logei", fmin=fmin, want_report=True)
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    assert rep["info"][1] > 0 and rep["jitter"][1] != 0
    assert idx1 == idx0 and _bits([val1]) == _bits([val0]) and _bits(sc1) == _bits(sc0)


# ---- 7. the trial loop ---------------------------------------------------------------------------------------------------------
def test_trial_loop_runs_on_log_expected_improvement(ctx, orc):
    class H(object):
        def __init__(self, name):
            self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1

    cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 3, "nSamples": 2, "seed": 2},
           "grid": {"type": "sobol", "size": 512, "dims": 6}, "score": {"type": "log_expected_improvement"},
           "model": {"type": "gp_regressor", "sample": True, "nBurnin": 2, "seed": 5}}
    bot = bots.bayesopt(B.hartmann6, [H("x%d" % k) for k in range(6)], cfg)
    assert type(bot.score) is bot7_amd.scores.log_expected_improvement
    bot.model._ctx = ctx
    bot.candidates = bot7_amd.grids.sobol(bot.config["grid"], context=ctx)()
    grid0 = np.asarray(bot.candidates).copy()
    bot.run_experiment()
    obs = np.asarray(bot.observed)
    assert obs.shape == (12, 6) and np.asarray(bot.candidates).shape == (500, 6)
    rows = {r.tobytes() for r in grid0}
    assert len({r.tobytes() for r in obs}) == 12 and all(r.tobytes() in rows for r in obs)
    scores, val, idx = bot.eval()
    assert scores.shape == (500,) and not np.isnan(scores).any() and not (scores == INF).any()
    assert val == scores[idx - 1] == scores.max()
