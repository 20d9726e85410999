"""b7_kg_nominate / b7_kg_last / b7_kg_compute on the GPU: the knowledge gradient.

The envelope arithmetic is measured against Frazier's sort-and-prune algorithm at 50 digits, with the numpy float64 restatement of
the library's own O(L^2) form as the yardstick; the slopes against a numpy long-double posterior covariance at the project's
posterior bar, 1e-5 relative to sqrt(amp); the nomination against the reference value vector by the rule of
test_gpu_ts.check_nominees, with twice the bar so that no near-tie needs an exclusion; everything else bit for bit.  Every test
prints its achieved figure; the docstrings carry the MI355X figures."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _kg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5   # the posterior bar


def _objective(X):
    return np.sin(3.0 * X.sum(axis=1, keepdims=True)) + X[:, -1:] ** 2


def problem(N, d, M, seed=0, noise=1e-2):
    """Uniform points (the oracle's Sobol stops at 39 dims), a noisy response: the setting the knowledge gradient is for."""
    rng = np.random.default_rng(1000 * seed + 7 * N + d)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    y = _objective(X) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(y)) if N > 1 else 1.0
    return X, y, Xc, {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": noise * amp, "mean": float(np.mean(y))}


def hyper_samples(hyp, S):
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.3 * s), amp=hyp["amp"] * (1.0 + 0.2 * s), mean=hyp["mean"] + 0.05 * s,
                 noise=hyp["noise"] * (1.0 + 0.5 * s)) for s in range(S)]


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def lines_of(last, s):
    """Sample s of a kg_last as b7_kg_compute takes it: alpha M x (n + 1) with the own intercept in column 0, and the slopes."""
    M, n = last["values"].shape[1], last["alpha"].shape[1]
    a = np.empty((M, n + 1))
    a[:, 0], a[:, 1:] = last["own_alpha"][s], last["alpha"][s][None, :]
    return a, last["slopes"][s]


def fold(values):
    """The marginal as the library folds it: the samples added in order, then one division."""
    acc = values[0].copy()
    for s in range(1, len(values)):
        acc = acc + values[s]
    return acc / float(len(values))


# ---- 1. the envelope arithmetic ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def envelope():
    """The cases, their 50-digit values and the numpy form's error against them, computed once."""
    out = {}
    for name, (a, b) in R.envelope_cases().items():
        hi, lo = R.kg_mp_rows(a, b)
        out[name] = (a, b, hi, lo, R.err_vs_mp(R.kg_numpy(a, b), hi, lo))
    return out


ENVELOPE_CASES = ["L1", "L2", "L3", "L16", "L17", "duplicated slopes", "duplicated lines", "three lines through one point", "all slopes zero",
                  "slope scales 1e-8 .. 1e8", "one dominated line far above"]


@pytest.mark.parametrize("name", ENVELOPE_CASES)
def test_envelope_against_sort_and_prune(ctx, envelope, name):
    """b7_kg_compute, 65 rows per case, against Frazier's algorithm at 50 digits.  Bar per row: 8 x the error of the numpy float64
    restatement of the same form on the same row + 16 eps max(1, |ref|).  Never negative, never NaN; L = 1 and all-zero slopes give
    exactly 0.0; L = 2 also against the closed form |b_0 - b_1| f(-|alpha_0 - alpha_1| / |b_0 - b_1|).
    MI355X: worst error / bar 0.083 over all cases (duplicated lines); the device's error is 3.1e-16 ... 9.4e-16 where the values are
    of order one (numpy's: 3.1e-16 ... 9.4e-16) and 2.1e-8 at a value of 1.4e8 (slope scale 1e8; numpy's 2.1e-8)."""
    a, b, hi, lo, e_np = envelope[name]
    got = ctx.kg_compute(a, b)
    assert got.shape == (65,) and np.isfinite(got).all() and (got >= 0.0).all()
    e_dev = R.err_vs_mp(got, hi, lo)
    bar = 8.0 * e_np + 16.0 * 2.0 ** -52 * np.maximum(1.0, np.abs(hi))
    k = int(np.argmax(e_dev / bar))
    print("envelope %-32s worst error / bar %.3g (row %d: device %.3g, numpy %.3g, ref %.6g); max device error %.3g"
          % (name, (e_dev / bar).max(), k, e_dev[k], e_np[k], hi[k], e_dev.max()))
    assert (e_dev <= bar).all()
    if name in ("L1", "all slopes zero"):
        assert (got == 0.0).all()
    if name == "L2":
        chi, clo = R.closed_form_two(a, b)
        assert (R.err_vs_mp(got, chi, clo) <= bar).all()


def test_envelope_without_an_own_line(ctx, envelope):
    """A NaN slope in column 0 means "no own line" (b7_kg_last's convention for the rows of A): the result is that of the other
    lines alone, whatever the intercept there."""
    a, b, hi, lo, _ = envelope["L17"]
    b0 = b.copy()
    b0[:, 0] = np.nan
    got = ctx.kg_compute(a, b0)
    rhi, rlo = R.kg_mp_rows(a[:, 1:], b[:, 1:])
    e_np = R.err_vs_mp(R.kg_numpy(a, b0), rhi, rlo)
    assert np.isfinite(got).all() and (R.err_vs_mp(got, rhi, rlo) <= 8.0 * e_np + 16.0 * 2.0 ** -52 * np.maximum(1.0, np.abs(rhi))).all()


# ---- 2. the slopes against the long-double posterior covariance --------------------------------------------------------------
#         N    d   kernel         n  S     both regimes (Npad 64 / 128 | 256, 384), every dpad slab class (4, 8 | 48, 96)
CASES = [(5, 1, "ardse", 1, 1), (64, 6, "ardmatern52", 5, 3), (65, 33, "ardse", 16, 1), (128, 6, "ardse", 16, 3),
         (129, 65, "ardmatern52", 5, 1), (300, 6, "ardse", 16, 1), (300, 33, "ardmatern52", 1, 3)]
M_COV = 200   # not a multiple of 64


@pytest.mark.parametrize("N,d,kernel,n,S", CASES)
def test_slopes_against_long_double(ctx, N, d, kernel, n, S):
    """b7_kg_last's alpha and slopes against k(x, a) - K* inv(K) k(X, a) (and var / sqrt(t) in column 0) in numpy long double, first
    with rows1 = NULL -- the chosen rows must be the n lowest of the reference's marginal mean, whose n-th and (n + 1)-th values are
    checked to differ by more than twice the bar --, then with caller's rows.  Bar: 1e-5 sqrt(amp).  A row of A has no own line
    (NaN in column 0, and only there); nothing of the padding columns shows: the values equal b7_kg_compute of the n + 1 lines.
    MI355X: slopes within 1.7e-15 (N = 129, d = 65) ... 2.0e-14 (N = 300, d = 6) sqrt(amp), alpha and the mean within 2.7e-13, nine orders
    below the bar; the library's rows are the reference's in every case; no jitter."""
    X, y, Xc, hyp = problem(N, d, M_COV)
    hyps = hyper_samples(hyp, S)
    stage(ctx, X, y, Xc, kernel)
    rng = np.random.default_rng(N + d)
    given = np.sort(rng.choice(M_COV, size=n, replace=False))
    for rows in (None, given + 1):
        val, idx, rep = ctx.kg_nominate(hyps, points=n, rows=rows, want_report=True, trace=True)
        last = ctx.kg_last(slopes=True)
        rows0, alpha, slopes, mu = R.slopes_ref(X, y, Xc, hyps, kernel, rows0=None if rows is None else given, n=n, jitter=rep["jitter"])
        if rows is None:
            mbar = np.sort(mu.mean(axis=0))
            assert n == M_COV or mbar[n] - mbar[n - 1] > 2.0 * BAR * max(1.0, abs(mbar[n - 1])), "inputs whose n-th and (n+1)-th means are apart"
        assert last["rows"].tolist() == (rows0 + 1).tolist()
        scale = np.sqrt(np.array([h["amp"] for h in hyps]))[:, None, None]
        own = np.ones(M_COV, dtype=bool)
        own[rows0] = False
        assert np.isnan(last["slopes"][:, rows0, 0]).all() and np.isfinite(last["slopes"][:, own, 0]).all() and np.isfinite(last["slopes"][:, :, 1:]).all()
        e_b = float(np.nanmax(np.abs(last["slopes"] - slopes) / scale))
        e_a = float(np.max(np.abs(last["alpha"] - alpha) / np.maximum(1.0, np.abs(alpha))))
        e_m = float(np.max(np.abs(last["own_alpha"] - mu) / np.maximum(1.0, np.abs(mu))))
        print("slopes N=%d d=%d %s n=%d S=%d rows=%s: slopes %.3g sqrt(amp), alpha %.3g, mean %.3g (bar %.0e); jitter %s"
              % (N, d, kernel, n, S, "library" if rows is None else "caller", e_b, e_a, e_m, BAR, rep["jitter"].tolist()))
        assert e_b <= BAR and e_a <= BAR and e_m <= BAR
        for s in range(S):
            assert ctx.kg_compute(*lines_of(last, s)).tobytes() == last["values"][s].tobytes()
        marg = fold(last["values"])
        assert idx - 1 == R.nominee_ref(marg) and np.float64(val).tobytes() == marg[idx - 1].tobytes()
    ctx.gp_set_kernel("ardse")


# ---- 3. the nomination end to end ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    X, y, Xc, hyp = problem(37, 3, 1000, seed=1)
    rows = np.array([3, 17, 42, 77, 101, 150, 199])   # 0-based, inside the first 200 rows
    return X, y, Xc, hyper_samples(hyp, 3), rows


@pytest.fixture(scope="module")
def small_ref(small):
    """The reference value vector of the shared problem (S = 3, the fixed rows), computed once."""
    X, y, Xc, hyps, rows = small
    rows0, alpha, slopes, mu = R.slopes_ref(X, y, Xc, hyps, "ardse", rows0=rows)
    return R.values_ref(alpha, slopes, mu)


def test_values_are_the_envelope_of_the_devices_own_lines(ctx, small, small_ref):
    """values == b7_kg_compute(alpha, slopes) bit for bit (the same code on the same operands); best_val / best_idx1 are the fold's
    arg-max bit for bit, and against the reference value vector the returned row is within 2 x 1e-5 max(1, |max|) of the maximum.
    MI355X: row 21 is the reference's own maximum (slack 0, value 0.0345786); max |values - reference| 8.8e-15."""
    X, y, Xc, hyps, rows = small
    stage(ctx, X, y, Xc)
    val, idx = ctx.kg_nominate(hyps, rows=rows + 1, trace=True)
    last = ctx.kg_last(slopes=True)
    for s in range(3):
        assert ctx.kg_compute(*lines_of(last, s)).tobytes() == last["values"][s].tobytes()
    assert (last["values"] >= 0.0).all()
    marg = fold(last["values"])
    assert idx - 1 == R.nominee_ref(marg) and np.float64(val).tobytes() == marg[idx - 1].tobytes()
    ref = small_ref.mean(axis=0)
    best = ref.max()
    slack = float(best - ref[idx - 1])
    err = float(np.abs(last["values"] - small_ref).max())
    print("nomination: row %d, value %.6g; reference maximum %.6g at row %d, slack %.3g; max |values - reference| %.3g"
          % (idx, val, best, int(ref.argmax()) + 1, slack, err))
    assert slack <= 2.0 * BAR * max(1.0, abs(best))


def test_same_call_twice_same_bits(ctx, small):
    X, y, Xc, hyps, rows = small
    stage(ctx, X, y, Xc)
    out = []
    for _ in range(2):
        v, i = ctx.kg_nominate(hyps, points=16)
        out.append((np.float64(v).tobytes(), i, ctx.kg_last()["values"].tobytes(), ctx.kg_last()["rows"].tobytes()))
    assert out[0] == out[1]


def test_values_do_not_depend_on_the_grids_size(ctx, small):
    """M = 200 and M = 1000, the first 200 rows shared, rows1 fixed: the same bits on the shared rows."""
    X, y, Xc, hyps, rows = small
    stage(ctx, X, y, Xc)
    ctx.kg_nominate(hyps, rows=rows + 1)
    big = ctx.kg_last()["values"]
    stage(ctx, X, y, Xc[:200])
    ctx.kg_nominate(hyps, rows=rows + 1)
    sub = ctx.kg_last()["values"]
    assert sub.shape == (3, 200) and sub.tobytes() == np.ascontiguousarray(big[:, :200]).tobytes()


def test_marginal_is_the_mean_of_the_samples_in_order(ctx, small):
    """S = 3 against three S = 1 calls: every sample's values bit for bit, and best_val the arg-max of ((v_0 + v_1) + v_2) / 3."""
    X, y, Xc, hyps, rows = small
    stage(ctx, X, y, Xc)
    val, idx = ctx.kg_nominate(hyps, rows=rows + 1)
    all3 = ctx.kg_last()["values"]
    singles = []
    for h in hyps:
        ctx.kg_nominate([h], rows=rows + 1)
        singles.append(ctx.kg_last()["values"][0])
    for s in range(3):
        assert all3[s].tobytes() == singles[s].tobytes()
    marg = fold(np.stack(singles))
    assert idx - 1 == R.nominee_ref(marg) and np.float64(val).tobytes() == marg[idx - 1].tobytes()


def test_jitter_redo(ctx, small):
    """Duplicated observation rows with zero noise: the plain factorisation fails, the nomination is redone through the jitter
    schedule, jitter_out reports it and t(x) carries it: slopes against the reference built with that jitter.
    MI355X: info [39, 39], jitter 1.1e-8 for both samples, slopes within 4.0e-12 sqrt(amp)."""
    X, y, Xc, hyps, rows = small
    Xd, yd = np.concatenate([X, X[:7]]), np.concatenate([y, y[:7]])
    hard = [dict(h, noise=0.0) for h in hyps[:2]]
    stage(ctx, Xd, yd, Xc[:200])
    val, idx, rep = ctx.kg_nominate(hard, rows=rows + 1, want_report=True, trace=True)
    assert (rep["info"] != 0).all() and (rep["jitter"] > 0).all()
    last = ctx.kg_last(slopes=True)
    rows0, alpha, slopes, mu = R.slopes_ref(Xd, yd, Xc[:200], hard, "ardse", rows0=rows, jitter=rep["jitter"])
    scale = np.sqrt(np.array([h["amp"] for h in hard]))[:, None, None]
    err = float(np.nanmax(np.abs(last["slopes"] - slopes) / scale))
    print("jitter %s info %s: slopes within %.3g sqrt(amp)" % (rep["jitter"].tolist(), rep["info"].tolist(), err))
    assert err <= BAR and np.isfinite(last["values"]).all() and 1 <= idx <= 200


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(small):
    import ctypes as C
    import bot7_amd
    X, y, Xc, hyps, rows = small
    hyps = hyps[:2]
    sp = {"score": "ei", "fmin": [float(y.min())]}
    c = bot7_amd.Context(0)
    try:
        def refused(code, what, call):
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call()
            assert e.value.code == code and what in str(e.value), str(e.value)

        refused(-4, "no successful b7_kg_nominate", lambda: c.kg_last())
        c.grid_upload(Xc[:9])
        arr, keep = c._pack_hyps(hyps, 3)
        out = np.zeros(2)
        optr = out.ctypes.data_as(C.c_void_p)
        assert c._L.b7_kg_nominate(c._h, 2, arr, 2, None, optr, optr, None, None) == -4   # (the wrapper asks for the data's d first)
        assert b"no resident data" in c._L.b7_last_error(c._h)
        c2 = bot7_amd.Context(0)
        try:
            c2.gp_set_data(X, y)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                c2.kg_nominate(hyps, points=2)
            assert e.value.code == -4 and "no candidate grid" in str(e.value)
        finally:
            c2.close()
        c.gp_set_data(X, y)
        usual = c.eval_nominate(hyps, **sp)
        for n, what in ((0, "n = 0"), (17, "n = 17"), (10, "exceeds the grid's 9 rows")):
            refused(-1, what, lambda: c.kg_nominate(hyps, points=n))
        refused(-1, "named twice", lambda: c.kg_nominate(hyps, rows=[1, 4, 1]))
        refused(-1, "not a row of the grid", lambda: c.kg_nominate(hyps, rows=[1, 10]))
        refused(-1, "not a row of the grid", lambda: c.kg_nominate(hyps, rows=[0, 2]))
        refused(-1, "S = 0", lambda: c.kg_nominate([], points=2))
        assert c._L.b7_kg_nominate(c._h, 2, arr, 2, None, None, optr, None, None) == -1
        assert b"NULL" in c._L.b7_last_error(c._h)
        assert c._L.b7_kg_nominate(c._h, 2, arr, 2, None, optr, None, None, None) == -1
        assert c._L.b7_kg_nominate(c._h, 2, None, 2, None, optr, optr, None, None) == -1
        assert c._L.b7_kg_nominate(None, 2, arr, 2, None, optr, optr, None, None) == -1
        refused(-1, "bad arguments", lambda: c.kg_compute(np.zeros((3, 18)), np.zeros((3, 18))))
        assert c.eval_nominate(hyps, **sp) == usual
        c.gp_set_data(X, np.hstack([y, y + 1.0]))
        refused(-5, "2 response columns", lambda: c.kg_nominate(hyps, points=2))
        c.gp_set_data(X, y)
        for opt in ("var_with_noise", "var_clamp"):
            c.gp_set_opts(**{opt: 1})
            refused(-5, "var_with_noise / var_clamp", lambda: c.kg_nominate(hyps, points=2))
            c.gp_set_opts()
        assert c.eval_nominate(hyps, **sp) == usual
        # a successful call leaves later nominations alone and the fit slot empty; slopes only when they were asked for
        v, i = c.kg_nominate(hyps, points=3)
        refused(-4, "no GP fit", lambda: c.gp_predict())
        refused(-4, "kept no slopes", lambda: c.kg_last(slopes=True))
        assert c.kg_last()["values"].shape == (2, 9)
        assert c.eval_nominate(hyps, **sp) == usual
        g = bot7_amd.Group([0, 0])
        try:
            g.grid_upload(Xc[:9])
            g.gp_set_data(X, y)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                g.members[0].kg_nominate(hyps, points=2)
            assert e.value.code == -4 and "group" in str(e.value)
            assert g.eval_nominate(hyps, **sp) == usual
        finally:
            g.close()
    finally:
        c.close()


def test_world_of_two_is_refused(ctx, small, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub): b7_kg_nominate answers B7_ERR_UNSUPPORTED, naming the
    communicator, on both, and the b7_eval_nominate that follows gives the single-context nomination of the union."""
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7kg_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_kg_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, y, Xc, hyps, rows = small
    stage(ctx, X, y, Xc)
    want = ctx.eval_nominate(hyps[:2], score="ei", fmin=[float(y.min())])
    for o in outs:
        res = json.load(open(o))
        assert res["code"] == -5 and "communicator of 2 ranks" in res["message"] and (res["value"], res["index"]) == want


# ---- 5. the trial loop ---------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, discretisation, seed=4):
    import bot7_amd
    from harness import benchmarks, bots
    grid = bot7_amd.grids.sobol({"size": 256, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    cfg = {"bot": {"verbose": 0, "budget": 5, "nInitial": 2, "nSamples": 3, "seed": seed},
           "grid": {"type": "sobol", "size": 256, "dims": 2},
           "score": {"type": "knowledge_gradient", "points": 8, "discretisation": discretisation, "nFeatures": 256}}
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    return bots.bayesopt(benchmarks.braninhoo, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})


@pytest.mark.parametrize("discretisation", ["mean", "thompson"])
def test_trial_loop(ctx, discretisation):
    """harness bayesopt on braninhoo (256 Sobol candidates, five trials, two of them initial, nSamples 3, 8 discretisation rows):
    the nominees are distinct, and every model-based one equals a direct library call on the same state (same hyper samples, same
    rows of A under 'thompson'); under 'mean' the library's own rows are the 8 lowest of the device's marginal mean.
    MI355X: nominees 51, 99, 95 ('mean') and 241, 253, 126 ('thompson')."""
    B = importlib.import_module("harness.bots.bayesopt")
    bot = _bot(ctx, discretisation)
    assert B.kg_refusal(bot.config, bot.model.class_()) is None
    with pytest.raises(NotImplementedError):
        bot.score.add_to(ctx)
    direct = []
    inner = bot._kg_nominate

    def traced(cand):
        val, idx = inner(cand)
        used = bot.last_kg
        again = ctx.kg_nominate(used["hyps"], points=used["points"], rows=used["rows"])
        last = ctx.kg_last()
        assert again == (val, idx) and last["rows"].shape == (8,) and len(set(last["rows"].tolist())) == 8
        if discretisation == "thompson":
            assert last["rows"].tolist() == used["rows"]
        else:
            mbar = last["own_alpha"].mean(axis=0)
            assert sorted(last["rows"].tolist()) == sorted((np.argsort(mbar, kind="stable")[:8] + 1).tolist())
        direct.append(idx)
        return val, idx
    bot._kg_nominate = traced
    rows = [bot.run_trial()[0] for _ in range(5)]
    assert len(direct) == 3
    obs = bot.observed
    assert obs.shape == (5, 2) and len({r.tobytes() for r in obs}) == 5
    assert np.asarray(bot.candidates).shape == (251, 2) and np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
    scores, val, idx = bot.eval(want_scores=True)
    assert scores.shape == (251,) and (scores >= 0).all() and scores[idx - 1] == val == scores.max()
    print("trial loop %s: nominees %s, best response %.4f" % (discretisation, direct, float(bot.responses.min())))
