"""The probit GP classifier by Laplace's method on the device (b7_clf_*, csrc/laplace.hip): the probit pieces against 50 digits, the
fit against the 50-digit mode (N <= 24) and against the rule in numpy.longdouble (N > 24), convergence, the log accumulator that
b7_clf_eval_logfeas leaves, the fit slot, determinism, composition with the feasibility column, one-class labels, the refusals and
the bot on gardner1_hidden.  Needs an MI355X: run with -m gpu.

References and bars: tests/_laplace_ref.py (checked on the CPU by tests/test_laplace_host.py).  The fit's bar is the project's:
error <= 8 x the float64 restatement's own error against the same truth + 16 eps max|quantity|; each test prints its worst
error / bar.

Achieved on an MI355X: probit pieces 2.0e-16 / 6.8e-16 / 1.2e-14 of max(1, |ref|) (log Phi, phi/Phi, W; bar 1e-13); the fit's worst
error / bar 0.354 against the 50-digit mode (N <= 24) and 0.621 against the longdouble rule (N = 63 .. 128)."""
import json
import math
import os
import subprocess
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd

import _laplace_ref as R
from _feas_ref import first_max

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT = ("f", "a", "W", "nll", "mu", "var")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(scope="module")
def ctx2():
    """A second context on the same device: the constraint's classifier beside the objective's regressor."""
    c = bot7_amd.Context(0)
    yield c
    c.close()


def _hyp(ls, amp, mean, noise=0.0):
    return {"lenscale_sq": np.asarray(ls, dtype=np.float64), "amp": float(amp), "noise": float(noise), "mean": float(mean)}


def _device_fit(c, X, v, ls, amp, mean, kern, Xs):
    """clf_fit_hyp + the mode + the latent posterior at Xs, as the dict of quantities the bars are stated for."""
    c.gp_set_kernel(kern)
    try:
        c.gp_set_data(X, v)
        rep = c.clf_fit_hyp(ls, amp, 0.25, mean)   # (noise is ignored)
        f, a, W = c.clf_mode_get()
        mu, var = c.gp_predict_at(Xs)
    finally:
        c.gp_set_kernel(R.SE)
    return rep, {"f": f, "a": a, "W": W, "nll": [rep["nll"]], "mu": np.asarray(mu).ravel(), "var": np.asarray(var).ravel()}


# ---- 1. the probit pieces -----------------------------------------------------------------------------------------------------
def test_probit_pieces_against_50_digits(ctx):
    """log Phi, phi/Phi and W by the fit's own device functions over z in [-1e6, 40]: within 1e-13 max(1, |ref|) of 50 digits."""
    rng = np.random.default_rng(7)
    z = np.concatenate([-np.exp(rng.uniform(0.0, math.log(1e6), 160)), rng.uniform(-40.0, 40.0, 240), rng.uniform(-7.0, -5.0, 60),
                        [-1e6, -6.0, np.nextafter(-6.0, 0.0), np.nextafter(-6.0, -7.0), -1.0, np.nextafter(-1.0, 0.0), 0.0, -0.0, 40.0, 37.5]])
    got = ctx.probit_compute(z)
    worst = [0.0, 0.0, 0.0]
    with mpmath.workdps(R.DPS):
        for i, zi in enumerate(z):
            ref = R.pieces_mp(float(zi))
            for k in range(3):
                worst[k] = max(worst[k], float(abs(mpmath.mpf(float(got[k][i])) - ref[k]) / max(1, abs(ref[k]))))
    print("probit pieces: worst scaled error log Phi %.3g, phi/Phi %.3g, W %.3g (bar 1e-13)" % tuple(worst))
    assert max(worst) <= 1e-13, worst
    assert (got[2] >= 0.0).all() and (got[2] <= 1.0 + 1e-15).all()


# ---- 2. the fit at N <= 24 against the 50-digit mode ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.host_cases(), ids=lambda c: "N%d-d%d-amp%g-mean%g-%s-%s" % c)
def test_fit_against_50_digits(ctx, case):
    """f^, a, W (b7_clf_mode_get), nll and the latent mean / variance at 8 rows (b7_gp_predict_at after b7_clf_fit_hyp) inside the
    project's bar; converged wherever the restatement converges, within the cap."""
    sol = R.solved_case(case)
    rep, got = _device_fit(ctx, sol["X"], sol["v"], sol["ls"], sol["amp"], sol["mean"], sol["kern"], sol["Xs"])
    frac = {q: R.errors_against(sol, q, got[q]) / R.bar(sol, q) for q in QUANT}
    print("fit %s: iters %d (restatement %d), error / bar %s; restatement's own error %s" % (
        case, rep["iters"], sol["fit"]["iters"], {q: "%.3f" % frac[q] for q in QUANT}, {q: "%.2g" % sol["err"][q] for q in QUANT}))
    assert 1 <= rep["iters"] <= R.ITMAX
    assert not sol["fit"]["converged"] or rep["info"] == 0, rep
    assert all(frac[q] <= 1.0 for q in QUANT), frac


# ---- 3. the fit at N > 24 against the rule in longdouble ------------------------------------------------------------------------------
LARGE = [(63, 1, 1.0, 0.0, R.SE, "mixed"), (64, 6, 100.0, -1.0, R.MATERN, "mixed"), (65, 33, 1.0, 0.5, R.SE, "mixed"),
         (128, 6, 100.0, 0.0, R.SE, "mixed"), (128, 33, 1.0, -1.0, R.MATERN, "ones"), (128, 1, 1e4, 0.5, R.SE, "zeros")]


@pytest.mark.parametrize("case", LARGE, ids=lambda c: "N%d-d%d-amp%g-mean%g-%s-%s" % c)
def test_fit_against_longdouble(ctx, case):
    """Both Npad classes and their edges.  The truth is the rule run in numpy.longdouble with a hand-written Cholesky; the float64
    restatement's own error against it is measured here and is the yardstick; the bar has the same form."""
    N, d, amp, mean, kern, labels = case
    X, v, ls, amp, mean, Xs = R.case_inputs(*case)
    LD = np.longdouble
    tr = R.laplace_fit(R.cov(X, X, ls, amp, kern, LD), v, mean, LD)
    tmu, tvar = R.posterior(R.cov(Xs, X, ls, amp, kern, LD), amp, mean, tr)
    fl = R.laplace_fit(R.cov(X, X, ls, amp, kern), v, mean)
    fmu, fvar = R.posterior(R.cov(Xs, X, ls, amp, kern), amp, mean, fl)
    truth = {"f": tr["f"], "a": tr["a"], "W": tr["W"], "nll": np.array([tr["nll"]]), "mu": tmu, "var": tvar}
    host = {"f": fl["f"], "a": fl["a"], "W": fl["W"], "nll": np.array([fl["nll"]]), "mu": fmu, "var": fvar}
    rep, got = _device_fit(ctx, X, v, ls, amp, mean, kern, Xs)
    frac, own = {}, {}
    for q in QUANT:
        own[q] = float(np.max(np.abs(host[q].astype(LD) - truth[q])))
        err = float(np.max(np.abs(np.asarray(got[q], dtype=np.float64).astype(LD) - truth[q])))
        frac[q] = err / (8.0 * own[q] + 16.0 * R.EPS * float(np.max(np.abs(truth[q]))))
    print("fit %s: iters %d (restatement %d, longdouble %d), error / bar %s; restatement's own error %s" % (
        case, rep["iters"], fl["iters"], tr["iters"], {q: "%.3f" % frac[q] for q in QUANT}, {q: "%.2g" % own[q] for q in QUANT}))
    assert tr["converged"] and fl["converged"]
    assert 1 <= rep["iters"] <= R.ITMAX and rep["info"] == 0, rep
    assert all(frac[q] <= 1.0 for q in QUANT), frac


# ---- 4. the accumulator, the fit slot, determinism --------------------------------------------------------------------------------
def _clf_problem(N, d, M, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    v = (np.sin(5.0 * X[:, 0]) + X.sum(axis=1) / d > 1.0).astype(np.float64)
    if v.min() == v.max():
        v[0] = 1.0 - v[0]
    G = rng.random((M, d))
    hyps = [_hyp(np.full(d, 0.09 * d) * (1.0 + 0.3 * s), 2.0 + s, -0.25 + 0.2 * s) for s in range(3)]
    return X, v, G, hyps


@pytest.mark.parametrize("N,d,M", [(24, 6, 1037), (100, 6, 2048), (65, 33, 517)])
@pytest.mark.parametrize("S", [1, 3])
def test_accumulator_is_logpi_of_the_kept_posterior(ctx, N, d, M, S):
    """After clf_eval_logfeas the accumulator equals b7_logpi_compute(mean_s, var_s + 1.0, fmin = 0) of the downloaded per-sample
    latent posteriors folded by the library's log-sum-exp, BIT FOR BIT, and the returned arg-max is that accumulator's.  The fold is
    the library's own: b7_logpi_compute over S columns of standardised rows (mean = -z_s, var = 1, so that its z is z_s exactly:
    sqrt and the division are correctly rounded on both sides), which the one-column call is first shown to reproduce."""
    X, v, G, hyps = _clf_problem(N, d, M)
    ctx.grid_upload(G)
    ctx.gp_set_data(X, v)
    val, idx, rep = ctx.clf_eval_logfeas(hyps[:S], want_report=True)
    assert not rep["info"].any() and (rep["iters"] >= 1).all() and (rep["iters"] <= R.ITMAX).all(), rep
    acc = ctx.score_finish(1.0, download=True)[2]
    post = [ctx.posterior_get(s) for s in range(S)]
    per = [ctx.logpi_compute(m, vr + 1.0, [0.0], 0.0) for m, vr in post]
    Z = np.stack([(0.0 + (-m)) / np.sqrt(vr + 1.0) for m, vr in post], axis=1)
    for s in range(S):
        assert _bits(ctx.logpi_compute(-Z[:, s], np.ones(M), [0.0], 0.0)) == _bits(per[s]), "the standardised row is not the row"
    want = per[0] if S == 1 else ctx.logpi_compute(-Z, np.ones(M), [0.0] * S, 0.0)
    assert np.isfinite(acc).all() and (acc <= 0.0).all()
    assert _bits(acc) == _bits(want), "accumulator differs in %d rows" % int(np.sum(acc != want))
    j = first_max(acc)
    assert idx == j + 1 and _bits([val]) == _bits([acc[j]])
    # ... and the same call twice gives the same bits
    val2, idx2 = ctx.clf_eval_logfeas(hyps[:S])
    assert (idx2, _bits([val2])) == (idx, _bits([val])) and _bits(ctx.score_finish(1.0, download=True)[2]) == _bits(acc)


@pytest.mark.parametrize("N,d", [(24, 6), (100, 6), (65, 33)])
def test_fit_slot_is_the_posterior_half(ctx, N, d):
    """After clf_fit_hyp, gp_predict_at at rows that are no observations equals the posterior half of clf_eval_logfeas at S = 1,
    bit for bit; so does gp_predict over the grid."""
    X, v, G, hyps = _clf_problem(N, d, 517)
    h = hyps[1]
    ctx.grid_upload(G)
    ctx.gp_set_data(X, v)
    ctx.clf_eval_logfeas([h])
    m0, v0 = ctx.posterior_get(0)
    ctx.clf_fit_hyp(h["lenscale_sq"], h["amp"], 3.0, h["mean"])
    m1, v1 = ctx.gp_predict_at(G)
    assert _bits(np.ravel(m1)) == _bits(m0) and _bits(v1) == _bits(v0)
    m2, v2 = ctx.gp_predict()
    assert _bits(np.ravel(m2)) == _bits(m0) and _bits(v2) == _bits(v0)


def test_a_fits_bits_depend_on_nothing_but_the_fit(ctx):
    """The same call twice gives the same bits; a fit's bits depend neither on B, nor on its position in the batch, nor on M."""
    X, v, G, hyps = _clf_problem(100, 6, 2048)
    ctx.grid_upload(G)
    ctx.gp_set_data(X, v)
    n3, i3, f3 = ctx.clf_nll_batch(hyps, want_info=True)
    n3b, i3b, _ = ctx.clf_nll_batch(hyps, want_info=True)
    assert _bits(n3) == _bits(n3b) and np.array_equal(i3, i3b) and not f3.any()
    for s in range(3):
        assert _bits(ctx.clf_nll_batch([hyps[s]])) == _bits(n3[s:s + 1])
    rev = ctx.clf_nll_batch(hyps[::-1] + hyps)
    assert _bits(rev[:3][::-1]) == _bits(n3) and _bits(rev[3:]) == _bits(n3)
    h = hyps[2]
    assert _bits([ctx.clf_fit_hyp(h["lenscale_sq"], h["amp"], 0.0, h["mean"])["nll"]]) == _bits(n3[2:])
    mode = ctx.clf_mode_get()
    ctx.clf_eval_logfeas(hyps)
    big = [ctx.posterior_get(s) for s in range(3)]
    ctx.grid_upload(G[:301])
    ctx.clf_eval_logfeas(hyps[::-1])
    for s in range(3):
        m, vr = ctx.posterior_get(2 - s)
        assert _bits(m) == _bits(big[s][0][:301]) and _bits(vr) == _bits(big[s][1][:301])
    ctx.clf_fit_hyp(h["lenscale_sq"], h["amp"], 0.0, h["mean"])
    assert all(_bits(p) == _bits(q) for p, q in zip(mode, ctx.clf_mode_get()))


# ---- 5. composition with the feasibility column -----------------------------------------------------------------------------------
def test_composition_with_the_feasibility_column(ctx, ctx2):
    """feas_reset + feas_add_acc(classifier context) + eval_nominate_feasible(logei) equals the host replay from feas_get and the
    downloaded accumulators: L is the classifier's accumulator, W == A + L bit for bit, the winner is W's first maximum."""
    N, d, M = 40, 3, 1037
    X, v, G, hyps_c = _clf_problem(N, d, M, seed=11)
    Y = np.sin(3.0 * X).sum(axis=1, keepdims=True)
    amp = float(np.var(Y))
    hyps_o = [_hyp(np.full(d, d / 8.0) * (1.0 + 0.25 * s), amp * (1.0 + 0.1 * s), float(np.mean(Y)), 1e-4 * amp) for s in range(2)]
    ctx2.grid_upload(G)
    ctx2.gp_set_data(X, v)
    ctx2.clf_eval_logfeas(hyps_c)
    Lc = ctx2.score_finish(1.0, download=True)[2]
    ctx.grid_upload(G)
    ctx.gp_set_data(X, Y)
    kw = dict(score="logei", fmin=[float(Y.min())])
    ctx.eval_nominate(hyps_o, **kw)
    A = ctx.score_finish(1.0, download=True)[2]
    ctx.feas_reset()
    ctx.feas_add_acc(ctx2)
    L = ctx.feas_get()
    assert _bits(L) == _bits(0.0 + Lc)
    val, idx = ctx.eval_nominate_feasible(hyps_o, **kw)
    W = ctx.score_finish(1.0, download=True)[2]
    assert _bits(W) == _bits(A + L)
    j = first_max(W)
    assert idx == j + 1 and _bits([val]) == _bits([W[j]])
    assert _bits(ctx2.score_finish(1.0, download=True)[2]) == _bits(Lc)   # the source is read, not modified


# ---- 6. one-class labels and N = 1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,labels", [(1, "zeros"), (1, "ones"), (40, "zeros"), (40, "ones"), (128, "ones")])
def test_one_class_labels(ctx, N, labels):
    """All-0 labels, all-1 labels and N = 1: the fit converges, and the feasibility it leaves leans the way the labels say."""
    d, M = 3, 300
    rng = np.random.default_rng(N)
    X, G = rng.random((N, d)), rng.random((M, d))
    v = np.zeros(N) if labels == "zeros" else np.ones(N)
    ctx.grid_upload(np.concatenate([X, G]))
    ctx.gp_set_data(X, v)
    h = _hyp(np.full(d, 0.27), 4.0, 0.0)
    nll, it, info = ctx.clf_nll_batch([h], want_info=True)
    fl = R.laplace_fit(R.cov(X, X, h["lenscale_sq"], h["amp"], R.SE), v, 0.0)
    assert info[0] == 0 and 1 <= it[0] <= R.ITMAX and abs(nll[0] - fl["nll"]) <= 1e-10 * max(1.0, abs(fl["nll"]))
    ctx.clf_eval_logfeas([h])
    acc = ctx.score_finish(1.0, download=True)[2]
    at_obs = acc[:N]
    assert np.isfinite(acc).all()
    assert (at_obs > math.log(0.5)).all() if labels == "zeros" else (at_obs < math.log(0.5)).all()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_name_leave_the_context_usable(ctx):
    X, v, G, hyps = _clf_problem(24, 3, 300)
    h = hyps[0]
    calls = {"clf_nll_batch": lambda c: c.clf_nll_batch([h]), "clf_fit_hyp": lambda c: c.clf_fit_hyp(h["lenscale_sq"], h["amp"], 0.0, h["mean"]),
             "clf_eval_logfeas": lambda c: c.clf_eval_logfeas([h])}

    def refused(c, code, text):
        for name, call in calls.items():
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call(c)
            assert e.value.code == code and text in str(e.value) and name in str(e.value), (name, str(e.value))

    def usable(c):
        c.grid_upload(G)
        c.gp_set_data(X, v)
        n = c.clf_nll_batch([h])
        val, idx = c.clf_eval_logfeas([h])
        assert np.isfinite(n).all() and 1 <= idx <= len(G)
        return n

    ref = usable(ctx)
    fresh = bot7_amd.Context(0)
    try:
        refused(fresh, -4, "call b7_gp_set_data first")            # no resident data
        fresh.gp_set_data(X, v)
        with pytest.raises(bot7_amd.Bot7HipError) as e:             # no grid
            fresh.clf_eval_logfeas([h])
        assert e.value.code == -4 and "no candidate grid" in str(e.value)
        with pytest.raises(bot7_amd.Bot7HipError) as e:             # no Laplace fit yet
            fresh.clf_mode_get()
        assert e.value.code == -4 and "no Laplace fit" in str(e.value)
        assert _bits(fresh.clf_nll_batch([h])) == _bits(ref)
    finally:
        fresh.close()
    ctx.grid_upload(G)
    for bad in (0.5, 2.0, -1.0, np.nan):                            # labels other than exactly 0 or 1
        w = v.copy()
        w[7] = bad
        ctx.gp_set_data(X, w)
        refused(ctx, -1, "label 7 is not exactly 0 or 1")
    ctx.gp_set_data(X, np.stack([v, v], axis=1))                    # more than one response column
    refused(ctx, -5, "2 response columns")
    Xb = np.random.default_rng(0).random((129, 3))
    ctx.gp_set_data(Xb, (Xb[:, 0] > 0.5).astype(np.float64))        # N > 128
    refused(ctx, -5, "N = 129 > 128")
    ctx.gp_set_data(X, v)
    for kw, text in ((dict(amp=0.0), "amp > 0"), (dict(noise=np.inf), "finite"), (dict(mean=np.nan), "finite"),
                     (dict(lenscale_sq=np.array([0.1, -1.0, 0.1])), "lenscale_sq[1]")):
        for name, call in (("clf_nll_batch", lambda hh: ctx.clf_nll_batch([hh])), ("clf_eval_logfeas", lambda hh: ctx.clf_eval_logfeas([hh])),
                           ("clf_fit_hyp", lambda hh: ctx.clf_fit_hyp(hh["lenscale_sq"], hh["amp"], hh["noise"], hh["mean"]))):
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call(dict(h, **kw))
            assert e.value.code == -1 and text in str(e.value) and name in str(e.value), str(e.value)
    g = bot7_amd.Group([0, 0])                                      # a member of a group
    try:
        g.grid_upload(G)
        g.gp_set_data(X, v)
        refused(g.members[0], -4, "belongs to a group")
    finally:
        g.close()
    assert _bits(usable(ctx)) == _bits(ref)


def test_world_of_two_is_refused(ctx, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub): every classifier entry point answers
    B7_ERR_UNSUPPORTED, naming the communicator, on both ranks, without a collective; the b7_eval_nominate that follows gives the
    single-context nomination of the union."""
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7clf_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_laplace_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, v, G, hyps = _clf_problem(24, 3, 600)
    ctx.grid_upload(G)
    ctx.gp_set_data(X, v)
    want = ctx.eval_nominate(hyps[:2], score="ei", fmin=[0.0])
    for o in outs:
        res = json.load(open(o))
        assert res["codes"] == [-5, -5, -5] and all("communicator of 2 ranks" in m for m in res["messages"]), res
        assert (res["value"], res["index"]) == want


# ---- 8. the bot on gardner1_hidden ------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def test_the_bot_on_a_hidden_constraint(ctx):
    """harness bayesopt on gardner1_hidden -- the constraint reported as 0 / 1, the objective NaN where it is violated -- with 512
    Sobol candidates, nInitial 6, 12 trials, nSamples 2 and the slice sampler on both models: it runs; every model-based trial's
    objective data has only finite rows while the classifier sees every row; each nominee is the arg-max replayed through the
    separate Context calls from the bot's own hyper samples.  Quality is printed, not asserted."""
    from harness import benchmarks as B
    from harness import bots
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    ccfg = {"type": "gp_classifier", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 6}
    cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 6, "nSamples": 2, "seed": 2,
                   "constraints": [{"threshold": 0.5, "binary": True, "model": ccfg}]},
           "grid": {"type": "sobol", "size": 512, "dims": 2}, "score": {"type": "log_expected_improvement"}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 512, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    bot = bots.bayesopt(B.gardner1_hidden, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})
    staged = []
    stage0 = model.stage
    model.stage = lambda X, Y, g: (staged.append(np.asarray(Y, dtype=np.float64).copy()), stage0(X, Y, g))[1]
    chk_o, chk_c = bot7_amd.Context(0), bot7_amd.Context(0)
    feasible_picks = 0
    try:
        for t in range(12):
            before = np.asarray(bot.candidates).copy()
            Xb = None if bot.observed is None else np.asarray(bot.observed).copy()
            Rb = None if bot.responses is None else np.asarray(bot.responses).copy()
            n_staged = len(staged)
            x, y = bot.run_trial()
            bot.update_best(x, y)
            y = np.asarray(y)
            assert y.shape == (1, 2) and y[0, 1] in (0.0, 1.0) and np.isnan(y[0, 0]) == (y[0, 1] == 1.0)
            if t < 6:
                continue
            last = bot.last_constrained
            feasible_picks += int(y[0, 1] == 0.0)
            rows = np.isfinite(Rb[:, 0])
            if rows.any():
                assert len(staged) == n_staged + 1 and np.isfinite(staged[-1]).all() and _bits(staged[-1]) == _bits(Rb[rows, :1])
            assert bot.constraints[0]["model"].last_fit["info"] == 0
            chk_c.grid_upload(before)
            chk_c.gp_set_data(Xb, Rb[:, 1:])
            chk_c.clf_eval_logfeas(last["constraint_hyps"][0])
            chk_o.grid_upload(before)
            chk_o.feas_reset()
            chk_o.feas_add_acc(chk_c)
            if last["fmin"] is None:
                v, i = chk_o.feas_nominate()
            else:
                chk_o.gp_set_data(Xb[rows], Rb[rows, :1])
                v, i = chk_o.eval_nominate_feasible(last["hyps"], score="logei", fmin=last["fmin"])
            assert i == last["index"] and _bits([v]) == _bits([last["value"]]), (t, i, last["index"])
            assert _bits(before[i - 1]) == _bits(x)
        assert bot.observed.shape == (12, 2) and np.asarray(bot.candidates).shape == (500, 2)
        host = np.asarray(bot.candidates)
        assert _bits(ctx.grid_download()) == _bits(host) and _bits(bot.constraints[0]["ctx"].grid_download()) == _bits(host)
        best = bot.best.get("y")
        print("gardner1_hidden, 12 trials (6 model-based): %d of 6 model-based nominees feasible; %d of 12 trials feasible; best feasible "
              "value %s" % (feasible_picks, int((bot.responses[:, 1] == 0.0).sum()), "none" if best is None else "%.6g" % float(np.ravel(best)[0])))
    finally:
        chk_o.close()
        chk_c.close()
        for con in bot.constraints or []:
            con["ctx"].close()
