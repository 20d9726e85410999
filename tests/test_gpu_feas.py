"""Constrained nomination on the device: the log probability of improvement (B7_SCORE_LOGPI) against 50-digit arithmetic
(tests/_feas_ref.py; bar |err| <= 1e-13 * max(1, |ref|)), the feasibility column (b7_feas_*), the weighted arg-max
(b7_eval_nominate_feasible) on every route, its state and refusals, the constrained toy end to end and the bot.

Achieved on an MI355X: 3.9e-16 on single scores, 3.0e-16 over three columns, 4.6e-16 on marginals over hyper samples; the EI weight
within 3.7e-16 of A exp(L) relative (bar 8.9e-16) (each test prints its figure)."""
import functools

import numpy as np
import pytest

import bot7_amd
from conftest import make_problem
from harness import benchmarks as B
from harness import bots

import _feas_ref as R

pytestmark = pytest.mark.gpu
INF, NAN = np.inf, np.nan
SHAPES = [(24, 3, 2048, 1), (24, 3, 2048, 3), (150, 5, 2048, 3)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _same(a, b):
    """Equal bit for bit where neither is NaN, NaN in the same rows."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and _bits(a[~na]) == _bits(b[~nb])


@pytest.fixture(scope="module")
def ctx2():
    """A second context on the same device: a constraint's model."""
    c = bot7_amd.Context(0)
    yield c
    c.close()


def _objective(X):
    return np.sin(3.0 * X).sum(axis=1, keepdims=True)


def _constraint(X):
    return np.cos(2.0 * X).sum(axis=1, keepdims=True)


def _hyps(hyp, S):
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.25 * s), amp=hyp["amp"] * (1.0 + 0.1 * s)) for s in range(S)]


def _hyp_of(Y, d):
    amp = float(np.var(Y))
    return {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(Y))}


def _redo_problem(orc):
    """Duplicated observations and a zero-noise hyper sample: the plain factorisation fails and the nomination is redone."""
    X = orc.c.sobol(40, 3, 1)
    X[7] = X[3]
    good = dict(lenscale_sq=np.full(3, 0.4), amp=1.0, noise=1e-3, mean=0.1)
    return X, _objective(X), orc.c.sobol(2048, 3, 100), [good, dict(good, noise=0.0, mean=0.0), dict(good, amp=1.3)]


# ---- 1. values --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _value_rows():
    mu, var = R.z_set(np.random.default_rng(4096), 4096)
    return mu, var, R.logpi_mp(mu, var, 0.0, 0.0)


def test_values_against_50_digits(ctx):
    """b7_logpi_compute, M = 4096, c = 1, over z uniform [-40, 8], log-uniform [-1e6, -1], uniform [8, 40], the branch points -1,
    its neighbours and 0, sigma log-uniform in [1e-6, 1], against mpmath on the exact inputs; then c = 3 columns against
    log(mean_k Phi(z_k)).  Bar 1e-13 * max(1, |ref|).
    Measured on an MI355X: c = 1 worst 3.9e-16 (at z = -2134), c = 3 worst 3.0e-16; the marginals of the one-call test worst
    4.6e-16 (the scipy restatement of the formula on the host: 4.6e-16)."""
    mu, var, ref = _value_rows()
    got = ctx.logpi_compute(mu, var, [0.0], 0.0)
    err = R.scaled_errors(got, ref)
    z = -mu / np.sqrt(var)
    print("LogPI device: worst scaled error %.3g at z = %.6g (z in [%.3g, %.3g])" % (err.max(), z[err.argmax()], z.min(), z.max()))
    assert np.isfinite(got).all() and (got <= 0.0).all()
    assert err.max() <= R.BAR, "%.3g at z = %g" % (err.max(), z[err.argmax()])
    rng = np.random.default_rng(3)
    M, c = 1024, 3
    v3 = np.exp(rng.uniform(np.log(1e-6), 0.0, M)) ** 2
    mu3 = -(rng.uniform(-40.0, 8.0, (M, c)) * np.sqrt(v3)[:, None])
    fm = np.array([0.0, -0.5, 0.25])
    got = ctx.logpi_compute(mu3, v3, fm, 0.0)
    err = R.scaled_errors(got, R.logpi_mean_mp(mu3, v3, fm, 0.0))
    print("LogPI device c = 3: worst scaled error %.3g" % err.max())
    assert err.max() <= R.BAR


# ---- 2. edge rows -----------------------------------------------------------------------------------------------------------
def test_edge_rows_are_exact(ctx):
    """The row classes of score.hip's header, exactly: var NaN or < 0 or mu NaN: NaN; var == 0: imprv >= 0 gives 0.0, else -inf;
    z = +inf gives 0.0, z = -inf gives -inf; beyond |z| ~ 1.3e154 -inf; a finite input with var >= 0 never scores NaN."""
    #              0     1    2    3    4    5    6      7       8      9     10     11
    mu = np.array([-2.0, 0.0, 3.0, 0.0, 0.0, NAN, NAN, -1e300, 1e300, 1e155, 1e154, -1e155])
    var = np.array([0.0, 0.0, 0.0, -1.0, NAN, 1.0, 0.0, 1e-320, 1e-320, 1.0, 1.0, 1.0])
    got = ctx.logpi_compute(mu, var, [0.0], 0.0)
    assert _bits(got[[0, 1]]) == _bits([0.0, 0.0]) and got[2] == -INF
    assert np.isnan(got[3:7]).all()
    assert _bits(got[7]) == _bits([0.0]) and got[8] == -INF
    assert got[9] == -INF and np.isfinite(got[10]) and got[10] < -1e307 and got[11] == 0.0
    # the same rows as one of three columns: a NaN column (or variance) poisons its row, the others stay finite
    m3 = np.stack([mu, np.full(12, 0.5), np.full(12, 0.5)], axis=1)
    g3 = ctx.logpi_compute(m3, np.where(np.isnan(var) | (var < 0), var, 1.0), [0.0, 0.0, 0.0], 0.0)
    assert np.isnan(g3[3:7]).all() and np.isfinite(np.delete(g3, [3, 4, 5, 6])).all()
    # finite inputs, var >= 0: never NaN
    rng = np.random.default_rng(11)
    m = rng.normal(size=4096) * 10.0 ** rng.integers(-300, 300, 4096)
    v = 10.0 ** rng.uniform(-320, 300, 4096)
    v[::7] = 0.0
    assert not np.isnan(ctx.logpi_compute(m, v, [0.0], 0.0)).any()


# ---- 3. one call = the loop, bit for bit --------------------------------------------------------------------------------------
def _loop(c, X_obs, Y, hyps, fmin, xi=0.0):
    """{b7_gp_predict_hyp; b7_score_logpi} x S + b7_score_finish(S) -> value, index, scores, [(mean, var)] per sample"""
    c.gp_set_data(X_obs, Y)
    mv = []
    for s, h in enumerate(hyps):
        out = c.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], download=True)
        mv.append((out["mean"][:, 0].copy(), out["var"].copy()))
        if s == 0:
            c.score_reset()
        c.score_logpi(fmin, xi)
    val, idx, scores = c.score_finish(float(len(hyps)), download=True)
    return val, idx, scores, mv


def _profiled(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        return out, (ctx.profile_get("score")[1], ctx.profile_get("argmax")[1])
    finally:
        ctx.profile_enable(False)


@pytest.mark.parametrize("N,d,M,S", SHAPES)
def test_eval_nominate_is_the_per_sample_loop_bit_for_bit(ctx, orc, N, d, M, S):
    """b7_eval_nominate(B7_SCORE_LOGPI) against the separate calls: equal winner, equal best_val bits, equal accumulator bits (the
    first two shapes: the fused kernel's LogPI instance, one "score" phase and no "argmax" phase; the third: score_batch_kernel and
    finish_kernel, one of each), and the scores equal log((1/S) sum_s Phi_s) in 50 digits from the downloaded mean / variance."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, d, N, M, _objective)
    hyps, fmin = _hyps(hyp, S), [float(np.median(Y))]
    ctx.grid_upload(X_hid)
    val0, idx0, sc0, mv = _loop(ctx, X_obs, Y, hyps, fmin)
    ctx.gp_set_data(X_obs, Y)
    (val1, idx1, rep), phases = _profiled(ctx, lambda: ctx.eval_nominate(hyps, score="logpi", fmin=fmin, want_report=True))
    assert phases == ((1, 0) if N <= 128 else (1, 1)), phases
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    assert not rep["jitter"].any() and not rep["info"].any()
    assert idx1 == idx0 and _bits([val1]) == _bits([val0]) and _bits(sc1) == _bits(sc0)
    assert _bits([val1]) == _bits([sc1[idx1 - 1]])
    ref = R.logmeanexp_mp([R.logpi_mp(m, v, fmin[0], 0.0) for m, v in mv])
    err = R.scaled_errors(sc1, ref)
    print("LogPI marginal N %d S %d: worst scaled error %.3g" % (N, S, err.max()))
    assert err.max() <= R.BAR
    assert ctx.eval_nominate(hyps, score="logpi", fmin=fmin, global_row_offset=1000)[1] == idx0 + 1000


def test_jitter_redo_keeps_the_loops_winner(ctx, orc):
    """Duplicated observations, zero noise: the nomination is redone through the jitter schedule; under LogPI it returns what the
    per-sample loop returns, bit for bit."""
    X, Y, X_hid, hyps = _redo_problem(orc)
    fmin = [float(np.median(Y))]
    ctx.grid_upload(X_hid)
    val0, idx0, sc0, _ = _loop(ctx, X, Y, hyps, fmin)
    ctx.gp_set_data(X, Y)
    val1, idx1, rep = ctx.eval_nominate(hyps, score="logpi", fmin=fmin, want_report=True)
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    assert rep["info"][1] > 0 and rep["jitter"][1] != 0
    assert idx1 == idx0 and _same([val1], [val0]) and _same(sc1, sc0)


# ---- 4. the weighted nomination -------------------------------------------------------------------------------------------------
def _weighted_case(ctx, ctx2, X_obs, Y, X_hid, hyps, small):
    d = X_obs.shape[1]
    Y2 = _constraint(X_obs)
    hyps2 = _hyps(_hyp_of(Y2, d), len(hyps))
    worst = 0.0
    for M in (X_hid.shape[0], X_hid.shape[0] - 37):
        Xh = X_hid[:M]
        ctx2.grid_upload(Xh)
        ctx2.gp_set_data(X_obs, Y2)
        ctx2.eval_nominate(hyps2, score="logpi", fmin=[float(np.median(Y2))], tradeoff=0.0)
        host = np.random.default_rng(M).normal(size=M) * 0.25
        host[5], host[M - 1] = -INF, -3.0
        ctx.grid_upload(Xh)
        ctx.gp_set_data(X_obs, Y)
        for kind in ("logei", "logpi", "ei"):
            kw = dict(score=kind, fmin=[float(Y.min()) if kind != "logpi" else float(np.median(Y))])
            v0, i0, rep0 = ctx.eval_nominate(hyps, want_report=True, **kw)
            A = ctx.score_finish(1.0, download=True)[2]
            ctx.feas_reset()
            ctx.feas_add_acc(ctx2)
            ctx.feas_add(host)
            L = ctx.feas_get()
            (v1, i1, rep1), phases = _profiled(ctx, lambda: ctx.eval_nominate_feasible(hyps, want_report=True, **kw))
            W = ctx.score_finish(1.0, download=True)[2]
            if not rep0["info"].any():                       # (the redo goes through the per-sample path: S score phases)
                assert phases == ((1, 0) if small else (1, 1)), phases
            assert _bits(ctx.feas_get()) == _bits(L)          # L is read, not modified
            assert np.array_equal(rep1["jitter"], rep0["jitter"]) and np.array_equal(rep1["info"], rep0["info"])
            assert L[5] == -INF and np.isfinite(np.delete(L, 5)).all()
            with np.errstate(all="ignore"):
                if kind == "ei":
                    want = R.feas_weight_np(A, L, False)
                    ok = ~np.isnan(want)
                    assert np.array_equal(np.isnan(W), ~ok) and (np.isnan(A[5]) or W[5] == 0.0)
                    rel = np.abs(W[ok] - want[ok]) - 4.0 * 2.0 ** -52 * np.abs(want[ok])
                    worst = max(worst, float((np.abs(W[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max()))
                    assert (rel <= 0.0).all(), "EI: |W - A exp(L)| above 4 ulp of A exp(L) by %.3g" % rel.max()
                else:
                    assert _same(W, R.feas_weight_np(A, L, True)) and _same(W, A + L) and (np.isnan(A[5]) or W[5] == -INF)
            j = R.first_max(W)
            assert i1 == j + 1 and _same([v1], [W[j]]), (kind, M, i1, j + 1)
    return worst


@pytest.mark.parametrize("N,d,M,S", SHAPES)
def test_weighted_nomination(ctx, ctx2, orc, N, d, M, S):
    """b7_eval_nominate_feasible for LogEI, LogPI and EI at M and M - 37 (a ragged tail block): L from a second context's LogPI
    nomination on another response over the same X plus a host vector with a -inf; A = the accumulator after b7_eval_nominate, W
    after b7_eval_nominate_feasible.  Log kinds: W == A + L bit for bit; EI: within 4 ulp of A exp(L); the winner is the first
    maximum of the device's own W, best_val its bits; jitter / info are b7_eval_nominate's; L is unchanged."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, d, N, M, _objective)
    worst = _weighted_case(ctx, ctx2, X_obs, Y, X_hid, _hyps(hyp, S), N <= 128)
    print("weighted nomination N %d S %d: EI worst |W - A exp(L)| / |A exp(L)| = %.3g (bar %.3g)" % (N, S, worst, 4 * 2.0 ** -52))


def test_weighted_nomination_behind_a_jitter_redo(ctx, ctx2, orc):
    X, Y, X_hid, hyps = _redo_problem(orc)
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X, Y)
    rep = ctx.eval_nominate(hyps, score="logei", fmin=[float(Y.min())], want_report=True)[2]
    assert rep["info"][1] > 0 and rep["jitter"][1] != 0
    _weighted_case(ctx, ctx2, X, Y, X_hid, hyps, True)


# ---- 5. the column ----------------------------------------------------------------------------------------------------------------
def test_the_column(ctx, ctx2, orc):
    N, d, M, S = SHAPES[1]
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, d, N, M, _objective)
    hyps, Y2 = _hyps(hyp, S), _constraint(X_obs)
    ctx2.grid_upload(X_hid)
    ctx2.gp_set_data(X_obs, Y2)
    ctx2.eval_nominate(_hyps(_hyp_of(Y2, d), S), score="logpi", fmin=[float(np.median(Y2))])
    src = ctx2.score_finish(1.0, download=True)[2]
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    # feas_add_acc == feas_add of the downloaded source accumulator, bit for bit (onto a non-trivial column)
    base = np.random.default_rng(5).normal(size=M)
    cols = []
    for add in (lambda: ctx.feas_add_acc(ctx2), lambda: ctx.feas_add(src)):
        ctx.feas_reset()
        assert not ctx.feas_get().any()
        ctx.feas_add(base)
        add()
        cols.append(ctx.feas_get())
    assert _bits(cols[0]) == _bits(cols[1]) == _bits(base + src) and np.isfinite(cols[0]).all()
    # L = 0: the plain nomination, exactly for the log kinds, in winner and value for EI
    for kind in ("logei", "logpi", "ei"):
        kw = dict(score=kind, fmin=[float(Y.min())])
        v0, i0 = ctx.eval_nominate(hyps, **kw)
        A = ctx.score_finish(1.0, download=True)[2]
        ctx.feas_reset()
        v1, i1 = ctx.eval_nominate_feasible(hyps, **kw)
        W = ctx.score_finish(1.0, download=True)[2]
        assert (i1, _bits([v1])) == (i0, _bits([v0])), kind
        if kind != "ei":
            assert _bits(W) == _bits(A)
        # -inf on the unconstrained winner's row: the runner-up of A
        mask = np.zeros(M)
        mask[i0 - 1] = -INF
        ctx.feas_add(mask)
        runner = R.first_max(np.where(np.arange(M) == i0 - 1, -INF, A))
        v2, i2 = ctx.eval_nominate_feasible(hyps, **kw)
        assert i2 == runner + 1 and i2 != i0 and _bits([v2]) == _bits([A[runner]]), kind
        # -inf on every row but one: that row
        ctx.feas_reset()
        only = np.full(M, -INF)
        only[777] = 0.0
        ctx.feas_add(only)
        v3, i3 = ctx.eval_nominate_feasible(hyps, **kw)
        assert i3 == 778 and _bits([v3]) == _bits([A[777]]), kind
        # a NaN in L wins, as a NaN wins everywhere
        poison = np.zeros(M)
        poison[1234] = NAN
        ctx.feas_add(poison)
        v4, i4 = ctx.eval_nominate_feasible(hyps, **kw)
        assert i4 == 1235 and np.isnan(v4), kind
    # feas_nominate: the first maximum of L alone; L untouched
    ctx.feas_reset()
    Lh = np.random.default_rng(8).normal(size=M)
    Lh[[100, 900]] = Lh.max() + 1.0
    ctx.feas_add(Lh)
    v, i = ctx.feas_nominate()
    assert i == 101 and v == Lh[100] and _bits(ctx.feas_get()) == _bits(Lh)
    Lh2 = np.zeros(M)
    Lh2[1500] = NAN
    ctx.feas_add(Lh2)
    v, i = ctx.feas_nominate()
    assert i == 1501 and np.isnan(v)


# ---- 6. state and refusals ------------------------------------------------------------------------------------------------------
def _raises(code, *words):
    class Guard(object):
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert et is bot7_amd.Bot7HipError, "no error raised (expected %d: %s)" % (code, " ".join(words))
            assert ev.code == code, (ev.code, str(ev))
            for w in words:
                assert w in str(ev), (w, str(ev))
            return True
    return Guard()


def test_state_and_refusals(ctx, ctx2, orc):
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 300, _objective)
    hyps, fmin = _hyps(hyp, 2), [float(Y.min())]
    kw = dict(score="logei", fmin=fmin)
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    # no column
    for call in (lambda: ctx.eval_nominate_feasible(hyps, **kw), ctx.feas_get, ctx.feas_nominate, lambda: ctx.feas_add(np.zeros(300)),
                 lambda: ctx.feas_add_acc(ctx2)):
        with _raises(-4, "no feasibility column", "b7_feas_reset"):
            call()
    # a column is forgotten by every change of the grid
    for change in (lambda: ctx.grid_upload(X_hid), lambda: ctx.grid_remove(7), lambda: ctx.nominate_commit(3, 0),
                   lambda: ctx.grid_remove_rows([1, 2])):
        ctx.feas_reset()
        ctx.eval_nominate_feasible(hyps, **kw)
        change()
        with _raises(-4, "no feasibility column"):
            ctx.eval_nominate_feasible(hyps, **kw)
        with _raises(-4, "no feasibility column"):
            ctx.feas_get()
    ctx.grid_upload(X_hid)
    ctx.feas_reset()
    # M mismatch
    with _raises(-1, "299 log-weights", "300 rows"):
        ctx.feas_add(np.zeros(299))
    ctx2.grid_upload(X_hid[:200])
    ctx2.gp_set_data(X_obs, Y)
    with _raises(-4, "holds no accumulator"):
        ctx.feas_add_acc(ctx2)
    ctx2.eval_nominate(hyps, score="logpi", fmin=fmin)
    with _raises(-1, "200 rows", "300"):
        ctx.feas_add_acc(ctx2)
    # a linear source accumulator
    ctx2.grid_upload(X_hid)
    ctx2.eval_nominate(hyps, score="ei", fmin=fmin)
    with _raises(-4, "linear sum", "log"):
        ctx.feas_add_acc(ctx2)
    ctx2.eval_nominate(hyps, score="logpi", fmin=fmin)
    ctx.feas_add_acc(ctx2)                                   # ... and the log one is taken
    # CB and MES
    with _raises(-5, "confidence bound", "signed"):
        ctx.eval_nominate_feasible(hyps, score="cb")
    with _raises(-5, "max-value entropy search"):
        ctx.eval_nominate_feasible(hyps, score="mes")
    # two response columns
    ctx.gp_set_data(X_obs, np.concatenate([Y, Y + 1.0], axis=1))
    with _raises(-5, "2 response columns"):
        ctx.eval_nominate_feasible(hyps, score="logei", fmin=[float(Y.min()), float(Y.min()) + 1.0])
    ctx.gp_set_data(X_obs, Y)
    # the refinement has no gradient piece for LogPI
    with _raises(-5, "eval_nominate_refine", "LogPI", "no gradient piece"):
        ctx.eval_nominate_refine(hyps, score="logpi", fmin=fmin, starts=2, iters=1)
    with _raises(-5, "LogPI", "no gradient piece"):
        ctx.score_grad_compute(np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 4, 3)), np.zeros((1, 4, 3)), score="logpi", fmin=fmin)
    # every refusal left the context usable, the column included
    ctx.eval_nominate_feasible(hyps, **kw)
    # the believer batch simply takes the kind: pick 1 is b7_eval_nominate's
    v, i = ctx.eval_nominate(hyps, score="logpi", fmin=fmin)
    vals, idx = ctx.eval_nominate_batch(hyps, 3, score="logpi", fmin=fmin)
    assert idx[0] == i and _bits([vals[0]]) == _bits([v]) and len(set(int(k) for k in idx)) == 3


def test_group_of_two_virtual_ranks_takes_logpi(ctx, orc):
    """b7_group_eval_nominate is a template over the kind: two members on one GPU give the single context's winner and bits."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 2048, _objective)
    hyps, fmin = _hyps(hyp, 3), [float(np.median(Y))]
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    val, idx = ctx.eval_nominate(hyps, score="logpi", fmin=fmin)
    sc = ctx.score_finish(1.0, download=True)[2]
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(X_hid)
        g.gp_set_data(X_obs, Y)
        gval, gidx = g.eval_nominate(hyps, score="logpi", fmin=fmin)
        gsc = np.concatenate([m.score_finish(1.0, download=True)[2] for m in g.members])
        with _raises(-4, "belongs to a group"):
            g.members[0].feas_reset()
    finally:
        g.close()
    assert gidx == idx and _bits([gval]) == _bits([val]) and _bits(gsc) == _bits(sc)


def test_blr_nominations_take_logpi(ctx, orc):
    """b7_blr_eval_nominate_marg (S = 2 heads on a 5 -> 16 -> 16 tanh basis, N = 32, M = 2048) and b7_blr_eval_nominate with
    B7_SCORE_LOGPI against the per-head loop {b7_blr_fit_x; b7_blr_basis; b7_blr_predict; b7_score_logpi} x S + b7_score_finish(S).
    The two routes factor the same 16 x 16 system by different schedules: mean and sigma differ by rounding amplified by the system's
    condition, taken as 1e-10 of the response scale at most (tests/test_gpu_logei.py's argument for the same heads), and
    |d log Phi / d mu| = phi / (sigma Phi) <= (1 + |z|) / sigma, |d log Phi / d sigma| <= |z| (1 + |z|) / sigma: the bound below, on
    top of the arithmetic's own 1e-13 max(1, |ref|)."""
    from conftest import make_network
    d, N, M = 5, 32, 2048
    W, b = make_network(d, (16, 16), seed=11)
    X_obs, Y, X_hid, _ = make_problem(ctx, orc, d, N, M, lambda X: np.sin(3 * X.sum(axis=1, keepdims=True)))
    al, be = [1.0, 2.0], [1.0 / (1e-2 * float(np.var(Y))), 1.0 / (2e-2 * float(np.var(Y)))]
    mn, fmin = [float(np.mean(Y))] * 2, [float(np.median(Y))]
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
            one = R.logpi_np(mu[:, 0], var, fmin[0], 0.0)    # head 0 alone, float64 restatement on this route's mean / variance
        ctx.score_logpi(fmin, 0.0)
    val0, idx0, sc0 = ctx.score_finish(2.0, download=True)
    val1, idx1, jit = ctx.blr_eval_nominate_marg(W, b, "Tanh", X_obs, Y, al, be, mn, score="logpi", fmin=fmin)
    sc1 = ctx.score_finish(1.0, download=True)[2]
    tol = bound + R.BAR * np.maximum(1.0, np.abs(sc0))
    print("LogPI BLR marg: worst |diff| %.3g, bound max %.3g" % (np.abs(sc1 - sc0).max(), bound.max()))
    assert jit == 0.0 and np.isfinite(sc1).all() and (sc1 <= 0.0).all()
    assert np.all(np.abs(sc1 - sc0) <= tol)
    assert val1 == sc1[idx1 - 1] and idx1 == R.first_max(sc1) + 1
    assert sc0[idx1 - 1] + tol[idx1 - 1] >= sc0[idx0 - 1] - tol[idx0 - 1]     # the loop's winner, or a row within the two bars of it
    # one head, written (not accumulated): b7_blr_eval_nominate
    v, i = ctx.blr_eval_nominate(W, b, "Tanh", X_obs, Y, al[0], be[0], mn[0], score="logpi", fmin=fmin)
    sc = ctx.score_finish(1.0, download=True)[2]
    assert np.isfinite(sc).all() and v == sc[i - 1] == sc.max()
    assert np.all(np.abs(sc - one) <= bound + R.BAR * np.maximum(1.0, np.abs(one)))


# ---- 7. the meaning, end to end --------------------------------------------------------------------------------------------------
TOY_SEED = 3


def _toy(orc, seed):
    pool = orc.c.sobol(1024 + 20, 2, seed)
    X_obs, X_hid = pool[::52][:20].copy(), np.delete(pool, np.arange(20) * 52, axis=0)
    Rz = B.gardner1(X_obs)
    Y, Cobs = np.ascontiguousarray(Rz[:, :1]), np.ascontiguousarray(Rz[:, 1:])
    ok = Cobs[:, 0] <= B.GARDNER1_THRESHOLD
    return X_obs, Y, Cobs, X_hid, _hyps(_hyp_of(Y, 2), 3), _hyps(_hyp_of(Cobs, 2), 3), float(Y[ok, 0].min())


def toy_gap(orc, seed):
    """(top-2 gap of the float64 restatement's weighted score, its winner, the unconstrained winner): the CPU side of test 7."""
    X_obs, Y, Cobs, X_hid, ho, hc, fmin = _toy(orc, seed)
    a, L = R.constrained_scores(orc, X_obs, Y, Cobs, X_hid, ho, hc, B.GARDNER1_THRESHOLD, fmin)
    w = a + L
    top = np.sort(w)[-2:]
    return float(top[1] - top[0]), R.first_max(w), R.first_max(a)


def test_constrained_toy_end_to_end(ctx, ctx2, orc):
    """Gardner et al. 2014's first simulation at (N, d, M) = (20, 2, 1024), objective and constraint with S = 3 hyper samples each,
    LogEI + the constraint's marginal log probability of feasibility: the device's nominee is that of a float64 restatement built
    on the oracle's posterior, and differs from the unconstrained eval_nominate's.  Sobol skip (seed) 3, chosen on the CPU among 1..6
    (toy_gap): the restatement's top-2 gap is 3.8e-2 (> 1e-6), its winner row 792 against the unconstrained 290."""
    gap, want, free = toy_gap(orc, TOY_SEED)
    print("constrained toy: restatement top-2 gap %.3g, winner row %d, unconstrained winner row %d" % (gap, want + 1, free + 1))
    assert gap > 1e-6 and want != free, "inputs: the seed no longer separates the winner"
    X_obs, Y, Cobs, X_hid, ho, hc, fmin = _toy(orc, TOY_SEED)
    ctx2.grid_upload(X_hid)
    ctx2.gp_set_data(X_obs, Cobs)
    ctx2.eval_nominate(hc, score="logpi", fmin=[B.GARDNER1_THRESHOLD], tradeoff=0.0)
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    v0, i0 = ctx.eval_nominate(ho, score="logei", fmin=[fmin])
    ctx.feas_reset()
    ctx.feas_add_acc(ctx2)
    v1, i1 = ctx.eval_nominate_feasible(ho, score="logei", fmin=[fmin])
    assert i0 == free + 1
    assert i1 == want + 1 and i1 != i0
    L = ctx.feas_get()
    assert L[i1 - 1] >= L[i0 - 1]                            # what the weight bought: a nominee at least as likely to be feasible


# ---- 8. the bot --------------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, seed=2):
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    cfg = {"bot": {"verbose": 0, "budget": 8, "nInitial": 3, "nSamples": 3, "seed": seed,
                   "constraints": [{"threshold": B.GARDNER1_THRESHOLD, "model": dict(mcfg, seed=6)}]},
           "grid": {"type": "sobol", "size": 512, "dims": 2}, "score": {"type": "log_expected_improvement"}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 512, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    return bots.bayesopt(B.gardner1, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})


def test_the_bot_under_constraints(ctx, ctx2):
    """harness bayesopt with config.bot.constraints on the toy (budget 8, nInitial 3, 512 Sobol candidates, nSamples 3, the slice
    sampler): the run completes; the first model-based nominee, recomputed through the separate Context calls from the bot's own
    hyper samples, is the bot's; every context's grid has lost the same rows; the same seed gives the same trials."""
    runs = []
    for rep in range(2):
        bot = _bot(ctx)
        grid0 = np.asarray(bot.candidates).copy()
        for t in range(8):
            before = np.asarray(bot.candidates).copy()
            X_before = None if bot.observed is None else np.asarray(bot.observed).copy()
            R_before = None if bot.responses is None else np.asarray(bot.responses).copy()
            x, y = bot.run_trial()
            bot.update_best(x, y)
            assert np.asarray(y).shape == (1, 2)
            if t == 3 and rep == 0:                          # the first model-based trial
                last = bot.last_constrained
                Yb, Cb = R_before[:, :1].copy(), R_before[:, 1:].copy()
                ctx2.grid_upload(before)
                ctx2.gp_set_data(X_before, Cb)
                ctx2.eval_nominate(last["constraint_hyps"][0], score="logpi", fmin=[B.GARDNER1_THRESHOLD], tradeoff=0.0)
                chk = bot7_amd.Context(0)
                try:
                    chk.grid_upload(before)
                    chk.gp_set_data(X_before, Yb)
                    chk.feas_reset()
                    chk.feas_add_acc(ctx2)
                    if last["fmin"] is None:
                        v, i = chk.feas_nominate()
                    else:
                        v, i = chk.eval_nominate_feasible(last["hyps"], score="logei", fmin=last["fmin"])
                finally:
                    chk.close()
                assert i == last["index"] and _same([v], [last["value"]])
                assert _bits(before[i - 1]) == _bits(x)
        assert bot.observed.shape == (8, 2) and bot.responses.shape == (8, 2) and np.asarray(bot.candidates).shape == (504, 2)
        rows = {r.tobytes() for r in grid0}
        assert len({r.tobytes() for r in bot.observed}) == 8 and all(r.tobytes() in rows for r in bot.observed)
        host = np.asarray(bot.candidates)
        assert _bits(ctx.grid_download()) == _bits(host)
        for con in bot.constraints:
            assert _bits(con["ctx"].grid_download()) == _bits(host)
            con["ctx"].close()
        runs.append((np.asarray(bot.observed).copy(), np.asarray(bot.responses).copy()))
    assert _bits(runs[0][0]) == _bits(runs[1][0]) and _bits(runs[0][1]) == _bits(runs[1][1])
