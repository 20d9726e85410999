"""The likelihood gradient (csrc/nll_grad.hip: b7_gp_fit_hyp_grad, b7_gp_nll_grad) and the bounded fit on it (b7_gp_fit_map) on the
device, against the host statements of tests/_nllgrad_ref.py.

Worst figures measured on an MI355X are recorded in DESIGN section 8; every test prints its own."""
import json
import math
import os
import subprocess
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib
import _nllgrad_ref as R
from _nllgrad_ref import MATERN, SE
from test_nllgrad_host import _margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- 4. the gradient against truth ---------------------------------------------------------------------------------------------
# (N, d, amp, noise / amp, mean, kernel): every N class of the kernel (one tile, a padded tile, 2 x 2, both Npad classes above 128),
# d in {1, 6, 33} and 96 once, the amplitudes, the noise levels and both means and kernels, without their product
CASES = [
    (1, 1, 1.0, 1e-2, 0.5, SE), (1, 6, 1e2, 0.0, 0.5, MATERN), (2, 6, 1e2, 1e-6, -1.0, MATERN), (2, 1, 1.0, 1e-2, -1.0, SE),
    (12, 6, 1.0, 1e-2, -1.0, SE), (12, 1, 1e-2, 1e-2, 0.5, MATERN), (24, 6, 1.0, 1e-6, 0.5, SE), (24, 33, 1e2, 1e-2, -1.0, MATERN),
    (24, 6, 1.0, 0.0, 0.5, MATERN),
    (63, 6, 1.0, 1e-2, 0.5, SE), (63, 1, 1e2, 1e-2, -1.0, MATERN), (64, 6, 1e-2, 1e-6, 0.5, SE), (64, 33, 1.0, 1e-2, -1.0, MATERN),
    (64, 6, 1.0, 0.0, -1.0, MATERN),
    (65, 6, 1.0, 1e-2, -1.0, SE), (65, 96, 1.0, 1e-2, 0.5, SE), (65, 1, 1e-2, 1e-2, 0.5, MATERN), (65, 33, 1e2, 1e-6, -1.0, MATERN),
    (128, 6, 1.0, 1e-2, 0.5, SE), (128, 33, 1e-2, 1e-2, -1.0, MATERN), (128, 1, 1.0, 1e-2, -1.0, SE),
    (129, 6, 1e2, 1e-2, 0.5, MATERN), (129, 33, 1.0, 1e-6, -1.0, SE), (129, 6, 1.0, 0.0, 0.5, MATERN),
    (257, 6, 1.0, 1e-2, -1.0, SE), (257, 33, 1e2, 1e-2, 0.5, MATERN), (257, 1, 1e-2, 1e-2, 0.5, SE),
    (300, 6, 1e-2, 1e-6, -1.0, MATERN), (300, 33, 1.0, 1e-2, 0.5, SE), (300, 6, 1e2, 1e-2, 0.5, SE),
]
WORST = {"lenscale": 0.0, "amp": 0.0, "noise": 0.0, "mean": 0.0}


def _truth(X, y, h, kern, jitter=0.0):
    """(grad, scale) as float64 pairs (hi, lo) are not needed: the truth's own rounding to float64 is 2^-53 of its value, far inside
    16 eps x scale.  50 digits up to N = 24, long double above."""
    args = (X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern, jitter)
    if X.shape[0] <= 24:
        _, g, s = R.nll_grad_mp(*args)
        return g, [float(v) for v in s], lambda v, t: abs(float(mpmath.mpf(float(v)) - t))
    _, g, s = R.nll_grad_ld(*args)
    return g, [float(v) for v in s], lambda v, t: abs(float(np.longdouble(v) - t))


def _check_against_truth(got, X, y, h, kern, jitter, tag):
    d = X.shape[1]
    g_t, scale, dist = _truth(X, y, h, kern, jitter)
    _, g64, _ = R.nll_grad_f64(X, y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], kern, jitter)
    worst = {}
    for k in range(d + 3):
        err64, err = dist(g64[k], g_t[k]), dist(got[k], g_t[k])
        lim = 8.0 * err64 + 16.0 * R.EPS * scale[k]
        cls = "lenscale" if k < d else ("amp", "noise", "mean")[k - d]
        ratio = err / lim if lim > 0 else (0.0 if err == 0 else float("inf"))
        worst[cls] = max(worst.get(cls, 0.0), ratio)
        WORST[cls] = max(WORST[cls], ratio)
    print("%s err/bar lenscale %.3g amp %.3g noise %.3g mean %.3g | worst so far %s"
          % (tag, worst["lenscale"], worst["amp"], worst["noise"], worst["mean"], {k: float("%.3g" % v) for k, v in WORST.items()}))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-d%d-a%g-n%g-m%g-%s" % c)
def test_gradient_against_truth(ctx, case):
    """Per component: |device - truth| <= 8 |float64 restatement - truth| + 16 eps scale, scale the truth's sum of the absolute terms."""
    N, d, amp, nrel, mean, kern = case
    X, y, h = R.problem(N, d, 1000 + N + d, amp=amp, noise_rel=nrel, mean=mean)
    if nrel == 0.0:
        assert R.plain_factorisation_succeeds(X, h["lenscale_sq"], h["amp"], 0.0, kern), "noise == 0 needs a case the plain factorisation takes"
    ctx.gp_set_kernel(kern)
    try:
        ctx.gp_set_data(X, y)
        r = ctx.gp_fit_hyp_grad(h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    finally:
        ctx.gp_set_kernel(SE)
    assert r["jitter"] >= 0.0 and np.isfinite(r["grad"]).all(), r
    if nrel == 0.0:
        assert r["jitter"] == 0.0 and r["grad"][d + 1] == 0.0 and not np.signbit(r["grad"][d + 1])
    _check_against_truth(r["grad"], X, y, h, kern, r["jitter"], "N=%d d=%d amp=%g noise/amp=%g %s" % (N, d, amp, nrel, kern))


# ---- 5. bit-level properties ---------------------------------------------------------------------------------------------------
def _route_checks(c, N, d, seed):
    X, y, h = R.problem(N, d, seed)
    a = (h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    c.gp_set_data(X, y)
    f0 = c.gp_fit_hyp(*a, want_nll=True)
    dl0 = c.gp_download(N)
    g_sep = c.gp_nll_grad()
    f1 = c.gp_fit_hyp_grad(*a)
    dl1 = c.gp_download(N)
    assert np.float64(f1["nll"]).tobytes() == f0["nll"][0].tobytes() and (f1["jitter"], f1["info"]) == (f0["jitter"], f0["info"])
    for p, q in zip(dl0, dl1):
        assert p.tobytes() == q.tobytes()
    assert g_sep.tobytes() == f1["grad"].tobytes()                     # b7_gp_nll_grad after b7_gp_fit_hyp == the fused call
    assert c.gp_fit_hyp_grad(*a)["grad"].tobytes() == f1["grad"].tobytes() and c.gp_nll_grad().tobytes() == g_sep.tobytes()   # twice
    c.grid_upload(np.random.default_rng(seed).random((300, d)))       # a grid present changes nothing: not the held fit's gradient,
    assert c.gp_nll_grad().tobytes() == g_sep.tobytes()                # which is still served, nor the fused call
    assert c.gp_fit_hyp_grad(*a)["grad"].tobytes() == f1["grad"].tobytes()
    dl2 = c.gp_download(N)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(dl0, dl2))
    c.profile_enable(True)                                             # which route the fit takes: the one-workgroup fit forms K itself,
    c.profile_reset()                                                  # every other route assembles it in a launch of its own ("kxx")
    c.gp_fit_hyp_grad(*a)
    kxx = c.profile_get("kxx")[1]
    c.profile_enable(False)
    return f1, kxx


def test_fused_call_is_the_fit_bit_for_bit_on_the_one_workgroup_and_persistent_routes():
    c = bot7_amd.Context(0)
    try:
        for N in (100, 200):
            f, kxx = _route_checks(c, N, 6, 40 + N)
            print("N = %d: nll %.17g jitter %g info %d, %d K(X,X) launches, fused == fit + gradient, bit for bit"
                  % (N, f["nll"], f["jitter"], f["info"], kxx))
            assert kxx == (0 if N == 100 else 1)           # N = 100: the one-workgroup fit; N = 200: the general front end
    finally:
        c.close()


def test_fused_call_is_the_fit_bit_for_bit_on_the_launch_schedule(monkeypatch):
    """The launch schedule through the diagnostic build's switch (B7_POTRF_SCHED=1), at both sizes.  That the switch was read shows in
    the route: the same variable that selects the schedule turns the one-workgroup fit off (b7_create), so N = 100 assembles K in a
    launch of its own here and does not on a default context.  (Persistent against per-panel launches has no counter of its own: it
    is the value of that variable.)"""
    monkeypatch.setenv("B7_POTRF_SCHED", "1")
    c = bot7_amd.Context(0, lib="diag")
    monkeypatch.delenv("B7_POTRF_SCHED")
    try:
        for N in (100, 200):
            f, kxx = _route_checks(c, N, 6, 40 + N)
            print("launch schedule N = %d: nll %.17g, %d K(X,X) launches, fused == fit + gradient, bit for bit" % (N, f["nll"], kxx))
            assert kxx == 1                                # also at N = 100: not the one-workgroup fit
    finally:
        c.close()


def test_jitter_redo_gradient_against_truth_of_the_jittered_matrix(ctx):
    """Duplicate rows and noise == 0: the plain attempt fails, the schedule finds a jitter, and the gradient is that of
    K + jitter_used I with the jitter a constant (noise component exactly 0)."""
    X, y, h = R.problem(10, 2, 77, noise_rel=0.0)
    X, y = np.vstack([X, X]), np.concatenate([y, y + 1e-3])
    ctx.gp_set_data(X, y)
    r = ctx.gp_fit_hyp_grad(h["lenscale_sq"], h["amp"], 0.0, h["mean"])
    assert r["info"] > 0 and r["jitter"] > 0.0, r
    assert r["grad"][3] == 0.0
    f = ctx.gp_fit_hyp(h["lenscale_sq"], h["amp"], 0.0, h["mean"], want_nll=True)
    assert f["nll"][0].tobytes() == np.float64(r["nll"]).tobytes() and f["jitter"] == r["jitter"]
    assert ctx.gp_nll_grad().tobytes() == r["grad"].tobytes()
    _check_against_truth(r["grad"], X, y, dict(h, noise=0.0), SE, r["jitter"], "jitter %.3g" % r["jitter"])


def test_gradient_is_nan_after_the_identity_fallback(ctx):
    """Duplicate rows under amp = 1e-300 and noise == 0: the pivots fall below the smallest normal double, the first jitter of the
    schedule already exceeds |K|_F, and the factorisation falls back to chol(I) (jitter_used = -1): every component is NaN, from the
    fused call and from b7_gp_nll_grad alike."""
    X, y, h = R.problem(6, 2, 78, noise_rel=0.0)
    X, y = np.vstack([X, X]), np.concatenate([y, y])
    ctx.gp_set_data(X, y)
    r = ctx.gp_fit_hyp_grad(h["lenscale_sq"], 1e-300, 0.0, h["mean"])
    assert r["jitter"] == -1.0 and r["info"] > 0, r
    assert np.isnan(r["grad"]).all() and np.isnan(ctx.gp_nll_grad()).all()
    print("chol(I) fallback: jitter %g, gradient %s" % (r["jitter"], r["grad"]))


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _refused(call, code, word):
    with pytest.raises(_lib.Bot7HipError) as e:
        call()
    assert e.value.code == code and word in str(e.value), (e.value.code, str(e.value))


def test_refusals_by_code_and_word():
    X, y, h = R.problem(20, 2, 9)
    a = (h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    t0 = np.concatenate([np.log(h["lenscale_sq"]), [np.log(h["amp"]), np.log(h["noise"]), h["mean"]]])
    c = bot7_amd.Context(0)
    try:
        _refused(c.gp_nll_grad, -4, "no GP fit")
        c.gp_set_data(X, y)
        _refused(c.gp_nll_grad, -4, "no GP fit")
        c.gp_set_data(X, (y > np.median(y)).astype(np.float64))
        c.clf_fit_hyp(*a)
        _refused(c.gp_nll_grad, -4, "classifier")
        c.gp_fit_hyp(*a)
        assert np.isfinite(c.gp_nll_grad()).all()                       # a regressor's fit after the classifier's is served
        c.gp_set_data(X, np.stack([y, -y], axis=1))
        c.gp_fit_hyp(*a)
        _refused(c.gp_nll_grad, -5, "2 response columns")
        _refused(lambda: c.gp_fit_hyp_grad(*a), -5, "2 response columns")
        _refused(lambda: c.gp_fit_map(t0, t0 - 1, t0 + 1), -5, "2 response columns")
    finally:
        c.close()
    g = bot7_amd.Group([0, 0])
    try:
        g.gp_set_data(X, y)
        m = g.members[0]
        m._data_d, m._data_n, m.ycols = 2, 20, 1
        _refused(m.gp_nll_grad, -4, "group")
        _refused(lambda: m.gp_fit_hyp_grad(*a), -4, "group")
        _refused(lambda: m.gp_fit_map(t0, t0 - 1, t0 + 1), -4, "group")
    finally:
        g.close()


def test_world_of_two_is_refused(tmp_path):
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7ngr_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_nllgrad_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    for o in outs:
        res = json.load(open(o))
        assert res["codes"] == [-5, -5, -5] and all("communicator of 2 ranks" in m for m in res["messages"]), res
        assert res["nll"] == res["nll_before"]


# ---- 7. the bounded fit ------------------------------------------------------------------------------------------------------------
def _gp_draw(N, d, seed):
    """Data drawn from a GP with known hypers (ARD-SE, lenscale_sq = 0.15 d .. 0.5 d, amp 2, noise 0.02, mean 1)."""
    rng = np.random.default_rng([seed, N, d])
    X = rng.random((N, d))
    ls = np.linspace(0.15, 0.5, d) * d
    diff = X[:, None, :] - X[None, :, :]
    K = 2.0 * np.exp(-0.5 * np.sum(diff * diff / ls, axis=2)) + 0.02 * np.eye(N)
    return X, 1.0 + np.linalg.cholesky(K) @ rng.standard_normal(N)


def _oracle(X, y):
    def fun(t):
        d = X.shape[1]
        try:
            v, g, _ = R.nll_grad_f64(X, y, np.exp(t[:d]), math.exp(t[d]), math.exp(t[d + 1]), t[d + 2], SE)
            if np.isfinite(v) and np.isfinite(g).all():
                return v, g
        except Exception:
            pass
        return 1e10, np.zeros_like(t)
    return fun


@pytest.mark.parametrize("N,d", [(40, 2), (150, 3)])
def test_fit_map_on_data_drawn_from_a_gp(N, d):
    X, y = _gp_draw(N, d, 5)
    model = bot7_amd.models.gp_regressor({}, context=object())
    h0 = model.init(X, y)
    lo, hi = model._bounds(X, y.reshape(-1, 1))
    t0 = np.clip(model._to_theta(h0), lo, hi)
    c = bot7_amd.Context(0)
    try:
        c.gp_set_data(X, y)
        c.gp_fit_map_trace_enable(True)
        r = c.gp_fit_map(t0, lo, hi, max_iters=200)
        tr = c.gp_fit_map_trace()
        dl = c.gp_download(N)
        t = r["theta"]
        assert tr.shape == (r["iters"] + 1, d + 5) and np.array_equal(tr[0, :d + 3], t0) and np.array_equal(tr[-1, :d + 3], t)
        assert (np.diff(tr[:, d + 3]) <= 0.0).all() and tr[-1, d + 3] == r["nll"]                  # the trace's nll never increases
        assert ((t >= lo) & (t <= hi)).all()
        assert r["status"] in (_lib.LBFGSB_CONVERGED, _lib.LBFGSB_MAX_ITERS), r["status"]
        from scipy.optimize import minimize
        s = minimize(_oracle(X, y), t0, jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)))
        print("N=%d d=%d: nll %.10g in %d iterations, %d evaluations, status %d; scipy on the float64 oracle %.10g in %d, %d; start %.10g; "
              "ours - scipy %.3g (margin %.3g)" % (N, d, r["nll"], r["iters"], r["evals"], r["status"], s.fun, s.nit, s.nfev, tr[0, d + 3],
                                                   r["nll"] - s.fun, _margin(s.fun)))
        assert r["nll"] <= s.fun + _margin(s.fun)
        hyp = ([math.exp(v) for v in t[:d]], math.exp(t[d]), math.exp(t[d + 1]), float(t[d + 2]))
        f = c.gp_fit_hyp(*hyp, want_nll=True)                                                        # the fit left == the fit at theta_out
        assert f["nll"][0].tobytes() == np.float64(r["nll"]).tobytes()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(dl, c.gp_download(N)))
        assert c.gp_nll_grad().tobytes() == r["grad"].tobytes()
        r2 = c.gp_fit_map(t0, lo, hi, max_iters=200)                                                 # the same bits twice
        assert r2["theta"].tobytes() == t.tobytes() and (r2["nll"], r2["iters"], r2["evals"], r2["status"]) == (r["nll"], r["iters"], r["evals"], r["status"])
        z = c.gp_fit_map(t0, lo, hi, max_iters=0)                                                    # no iterations: theta0 and its value
        f0 = c.gp_fit_hyp([math.exp(v) for v in t0[:d]], math.exp(t0[d]), math.exp(t0[d + 1]), float(t0[d + 2]), want_nll=True)
        assert np.array_equal(z["theta"], t0) and np.float64(z["nll"]).tobytes() == f0["nll"][0].tobytes() and z["iters"] == 0
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[d + 1] = hi2[d + 1] = t0[d + 1]                                                           # a fixed noise comes back with its bits
        q = c.gp_fit_map(t0, lo2, hi2, max_iters=30)
        assert q["theta"][d + 1].tobytes() == t0[d + 1].tobytes() and q["nll"] <= z["nll"]
        assert not q["status"] & _lib.LBFGSB_LINESEARCH
    finally:
        c.close()


# ---- 8. the model, end to end --------------------------------------------------------------------------------------------------
def test_the_bot_with_fit_map_on_hartmann6(monkeypatch):
    """gp_regressor({'fit': 'map'}) through the harness bot on hartmann6, 12 trials (2 random, 10 model-based), 2000 Sobol candidates,
    twice on fresh contexts: every trial's estimate (the theta the fit returned) inside _bounds, its nll (the value the fit returned)
    at or below the heuristic's on the same data (the value the library returns at the heuristic's theta), no slack on either; and
    the two runs agree bit for bit."""
    from harness import default_regime as dr
    G = bot7_amd.models.gp_regressor
    fits, inner = [], G._fit_map

    def recording(self, X, Y):
        before = getattr(self, "_map_done", None)
        v = inner(self, X, Y)
        if self._map_done is not before:          # a new fit, not a repeated call of the same trial
            fits.append((dict(self.last_fit), X.copy(), Y.copy()))
        return v
    monkeypatch.setattr(G, "_fit_map", recording)
    runs = []
    for _ in range(2):
        c = bot7_amd.Context(0)
        try:
            runs.append(dr.run(c, trials=12, grid_size=2000, nSamples=1, fit="map", fit_opt={"max_iters": 30}))
        finally:
            c.close()
    a, b = runs
    assert a["nominees"] == b["nominees"] and len(a["nominees"]) == 12 and len(set(a["nominees"])) == 12
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a["draws"], b["draws"]))
    assert len(fits) == 20 and all(p[0]["theta"].tobytes() == q[0]["theta"].tobytes() for p, q in zip(fits[:10], fits[10:]))
    c = bot7_amd.Context(0)
    try:
        worst = -np.inf
        for lf, X, Y in fits[:10]:
            lo, hi = lf["bounds"]
            want_lo, want_hi = G({})._bounds(X, Y)
            assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
            assert ((lf["theta"] >= lo) & (lf["theta"] <= hi)).all(), (lf["theta"], lo, hi)
            assert not lf["status"] & _lib.LBFGSB_LINESEARCH
            t_h = np.clip(G._to_theta(G({}).init(X, Y)), lo, hi)
            c.gp_set_data(X, Y)
            n_heu = c.gp_fit_map(t_h, lo, hi, max_iters=0)["nll"]
            n_est = c.gp_fit_map(lf["theta"], lo, hi, max_iters=0)["nll"]
            assert n_est == lf["nll"][0]                                 # the value the model recorded is the fit's at its theta
            worst = max(worst, n_est - n_heu)
            assert n_est <= n_heu, (X.shape[0], n_est, n_heu)
        print("fit = 'map' on hartmann6: best %.6g; largest nll(estimate) - nll(heuristic) over the trials %.4g; started from the "
              "heuristic on %d of 10 trials" % (a["best"]["y"], worst, sum(bool(lf["from_heuristic"]) for lf, _, _ in fits[:10])))
    finally:
        c.close()
