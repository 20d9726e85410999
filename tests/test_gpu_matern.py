"""The ARD Matern-5/2 covariance (b7_gp_set_kernel(ctx, B7_KERNEL_MATERN52), config.model.kernel = 'ardmatern52') on the device,
on both paths: 'small' (the default library at N <= 128, d <= 32: gp_small_kernel, kpost_small_kernel) and 'general' (the
diagnostic build with B7_FIT_SMALL=0 B7_KPOST_SMALL=0 B7_NLL_SMALL=0: observation scaling, ksx_kernel, persistent Cholesky,
post_kernel), against 40-digit arithmetic at exact arguments and LAPACK on the host (tests/_matern_ref.py).  Every context here
is this module's own: the session's shared context never leaves ARD-SE."""
import functools
import math
import os

import mpmath
import numpy as np
import pytest

import _exact as E
import _matern_ref as R

pytestmark = pytest.mark.gpu
GENERAL = {"B7_FIT_SMALL": "0", "B7_KPOST_SMALL": "0", "B7_NLL_SMALL": "0"}
REL = 1e-5   # the project's contract for posterior mean / variance


def _diag_context(env):
    import bot7_amd
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return bot7_amd.Context(0, lib="diag")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def paths():
    import bot7_amd
    cs = {"small": bot7_amd.Context(0), "general": _diag_context(GENERAL)}
    for c in cs.values():
        c.gp_set_kernel("ardmatern52")
    yield cs
    for c in cs.values():
        c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def relerr(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))) if a.size else 0.0


# ---- 1. the covariance itself against 40-digit arithmetic --------------------------------------------------------------------
AMPS = (2.0 ** -40, 1e-3, 1.0, 3.0, 1e3, 2.0 ** 40)


@functools.lru_cache(maxsize=None)
def _ksx_points(d, dense):
    X, args = R.matern_points(d, dense=dense, seed=d)
    with mpmath.workdps(40):
        base, ss = [], []
        for a in args:
            s = mpmath.sqrt(-10 * mpmath.mpf(a.numerator) / a.denominator)
            base.append((1 + s + s * s / 3) * mpmath.exp(-s))
            ss.append(float(s))
    return X, base, np.array(ss)


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_cross_covariance_against_mpmath(paths, path, d):
    """K(X*, X) of one observation at the origin: mu = K* alpha for ~8 000 exact arguments per d (s = sqrt(-10 arg) over a dense
    sweep of [0, 1000], the band s in [700, 760] where amp m exp(-s) leaves the normal range, s near 0, the clamp at 1000 and
    beyond), amp in 2^-40 .. 2^40.  Bar: (4 + s) ulp of the truth where it is normal, 2^-1073 absolute plus the
    same inherent s 2^-52 |truth| below (tests/_matern_ref.py: within_matern_bar).  A NaN and an inf
    coordinate give non-finite results in their own rows and leave every other row's bits alone.  Measured on an MI355X, both
    paths: at most s + 2.14 ulp (d = 6, 32; s + 1.86 at d = 1) where the truth is normal, 2^-1074 beyond the s term below."""
    c = paths[path]
    Xc, base, s = _ksx_points(d, 5000)
    worst = (0.0, 0.0)
    for amp in AMPS:
        top = 4.0 ** math.ceil(math.log(amp, 4))
        noise = top - amp
        c.grid_upload(Xc)
        c.gp_fit(np.zeros((1, d)), np.array([[top]]), np.ones(d), amp, noise, 0.0)
        _, alpha, _ = c.gp_download(1)
        mu, var = c.gp_predict()
        a = float(alpha[0, 0])
        with mpmath.workdps(40):
            hi, lo = E.pairs([mpmath.mpf(amp) * b * mpmath.mpf(a) for b in base])
        ok, wu, wa = R.within_matern_bar(mu[:, 0], hi, lo, s)
        worst = (max(worst[0], wu), max(worst[1], wa))
        assert ok, "%s d %d amp %g: %.2f ulp beyond s, %.3g abs" % (path, d, amp, wu, wa)
        bad = Xc.copy()
        i0 = 1000
        bad[i0, d - 1] = np.nan
        bad[i0 + 1, 0] = np.inf
        c.grid_upload(bad)
        mu2, var2 = c.gp_predict()
        assert not np.isfinite(mu2[i0:i0 + 2, 0]).any() and not np.isfinite(var2[i0:i0 + 2]).any()
        keep = np.ones(len(Xc), dtype=bool)
        keep[i0:i0 + 2] = False
        assert _bits(mu2[keep]) == _bits(mu[keep]) and _bits(var2[keep]) == _bits(var[keep])
    print("Matern K(X*,X) %s d %d: worst %.3f ulp beyond s, %.3g absolute subnormal" % (path, d, worst[0], worst[1]))


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_observation_covariance_against_mpmath(paths, path, d):
    """K(X, X): observation 0 at the origin, amp = 3, noise = 1, so L00 = 2 and column 0 of L is K[:, 0] / 2, 127 exact arguments
    per fit; the last fit has an N that is no multiple of 16 (its padding must be exactly zero: the factor of the real rows
    would change otherwise).  Same bar as above; measured on an MI355X, both paths: at most s + 2.08 ulp, 2^-1073 beyond the s term."""
    c = paths[path]
    Xc, base, s = _ksx_points(d, 1500)
    with mpmath.workdps(40):
        hi, lo = E.pairs([3 * b for b in base])
    got = np.empty(len(base))
    for s0 in range(0, len(base), 127):
        rows = Xc[s0:s0 + 127]
        X = np.concatenate([np.zeros((1, d)), rows])
        rep = c.gp_fit(X, np.zeros((len(X), 1)), np.ones(d), 3.0, 1.0, 0.0)
        assert rep["jitter"] == 0
        L, _, _ = c.gp_download(len(X))
        assert L[0, 0] == 2.0
        got[s0:s0 + len(rows)] = 2.0 * L[1:, 0]
    assert (len(base) % 127 + 1) % 16 != 0
    ok, wu, wa = R.within_matern_bar(got, hi, lo, s)
    print("Matern K(X,X) %s d %d: worst %.3f ulp beyond s, %.3g absolute subnormal" % (path, d, wu, wa))
    assert ok, "%s d %d: %.2f ulp beyond s, %.3g abs" % (path, d, wu, wa)


# ---- 2. the small kernels give the general schedule's bits under Matern ------------------------------------------------------
@pytest.mark.parametrize("N,d", [(2, 2), (5, 1), (16, 3), (25, 2), (48, 6), (63, 6), (64, 6), (65, 6), (80, 6), (81, 5), (96, 6), (100, 6),
                                 (112, 6), (113, 9), (127, 16), (128, 32), (100, 32), (33, 31)])
def test_small_kernels_equal_the_general_schedule_bit_for_bit(paths, N, d):
    """As test_gpu_parity's ARD-SE test: gp_small_kernel, kpost_small_kernel and the fused score against the general schedule
    (B7_FIT_SMALL=0 B7_KPOST_SMALL=0 B7_NLL_SMALL=2: the likelihoods against round 3's four-wave kernel, which sums them in the
    same order) -- L, L^-1, alpha, the likelihoods, posterior mean and variance, scores and nominations, bit for bit."""
    ctx = paths["small"]
    ref = _diag_context({"B7_FIT_SMALL": "0", "B7_NLL_SMALL": "2", "B7_KPOST_SMALL": "0"})
    try:
        ref.gp_set_kernel("ardmatern52")
        rng = np.random.default_rng(1000 * N + d)
        X = rng.random((N, d))
        Y = np.sin(X.sum(1, keepdims=True) * 3.0) + 0.01 * rng.normal(size=(N, 1))
        ls = np.full(d, d / 8.0) * (0.5 + rng.random(d))
        hyps = [{"lenscale_sq": ls * (1 + 0.05 * s), "amp": 1.3, "noise": 1e-3, "mean": 0.1} for s in range(10)]
        outs = []
        for c in (ctx, ref):
            o = c.gp_fit(X, Y, ls, 1.3, 1e-3, 0.1, want_nll=True)
            L, al, Li = c.gp_download(N)
            c.gp_set_data(X, Y)
            nll5 = c.gp_nll_batch(np.outer(0.5 + 0.1 * np.arange(5), ls), 1.3, 1e-3, 0.1)
            nll1 = c.gp_nll_batch(ls, 1.3, 1e-3, 0.1)
            c.grid_sobol(3000 + N, d, 5, download=False)
            p = c.gp_predict_hyp(ls, 1.3, 1e-3, 0.1, download=True)
            b1 = c.eval_nominate(hyps[:1], score="ei", fmin=[float(Y.min())])
            s1 = c.score_finish(1.0, download=True)[2]
            b10 = c.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
            s10 = c.score_finish(1.0, download=True)[2]
            b3 = c.eval_nominate(hyps[:3], score="cb")
            s3 = c.score_finish(1.0, download=True)[2]
            outs.append({"L": L, "alpha": al, "Linv": Li, "fit_nll": np.asarray(o["nll"]), "nll5": nll5, "nll1": nll1, "mean": p["mean"],
                         "var": p["var"], "b1": np.array(b1), "s1": s1, "b10": np.array(b10), "s10": s10, "b3": np.array(b3), "s3": s3})
        for k in outs[0]:
            assert outs[0][k].tobytes() == outs[1][k].tobytes(), "N %d d %d: %s differs from the general schedule" % (N, d, k)
        f = R.lapack_fit(X, Y, ls, 1.3, 1e-3, 0.1, ctx.grid_download())
        assert abs(float(outs[0]["fit_nll"][0]) - f["nll"]) <= 1e-9 * max(1.0, abs(f["nll"]))
        assert relerr(outs[0]["mean"], f["mu"], floor=1e-3 * np.abs(f["mu"]).max()) < REL and relerr(outs[0]["var"], f["var"]) < REL
    finally:
        ref.close()


# ---- 3. fits against LAPACK --------------------------------------------------------------------------------------------------
def _problem(N, d, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    Y = (np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0]) + 0.05 * rng.normal(size=N)).reshape(-1, 1)
    amp = float(np.var(Y))
    return X, Y, rng.random((M, d)), {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(Y))}


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("N,d", [(2, 1), (25, 6), (100, 6), (128, 32), (129, 6), (300, 64), (2048, 32), (200, 96), (100, 1)])
def test_fit_posterior_and_likelihood_against_lapack(paths, path, N, d):
    """NLL, jitter, posterior mean and variance of b7_gp_fit / b7_gp_predict under Matern against LAPACK on the host's Matern K:
    mean and variance within the project's 1e-5 relative contract, the NLL within 1e-9; b7_gp_nll_batch (N = 100: the
    one-workgroup kernel; N = 200: the persistent launch) gives b7_gp_fit_hyp's likelihood (1e-10: the same K and factor, the
    final sums in another order, as under ARD-SE: tests/test_gpu_parity.py holds those two at 1e-12 relative too, not bits)."""
    c = paths[path]
    X, Y, Xs, h = _problem(N, d, 3000, 7 * N + d)
    out = c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
    f = R.lapack_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xs)
    assert out["info"] == f["info"] and out["jitter"] == f["jitter"] == 0.0
    assert abs(float(out["nll"][0]) - f["nll"]) <= 1e-9 * max(1.0, abs(f["nll"]))
    c.grid_upload(Xs)
    mu, var = c.gp_predict()
    assert relerr(mu[:, 0], f["mu"], floor=1e-3 * np.abs(f["mu"]).max()) < REL and relerr(var, f["var"]) < REL
    if N in (100, 200):
        c.gp_set_data(X, Y)
        for scale in (1.0, 0.7):
            ls = h["lenscale_sq"] * scale
            nb = c.gp_nll_batch(ls, h["amp"], h["noise"], h["mean"])[0]
            one = float(c.gp_fit_hyp(ls, h["amp"], h["noise"], h["mean"], want_nll=True)["nll"][0])
            assert nb == pytest.approx(one, rel=1e-10), (N, d, nb, one)


@pytest.mark.parametrize("path", ["small", "general"])
def test_duplicated_rows_without_noise_run_the_jitter_schedule(paths, path):
    c = paths[path]
    for N in (45, 200):
        X, Y, Xs, h = _problem(N - 5, 3, 500, N)
        X = np.concatenate([X, X[:5]])
        Y = np.concatenate([Y, Y[:5]])
        out = c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], 0.0, h["mean"], want_nll=True)
        f = R.lapack_fit(X, Y, h["lenscale_sq"], h["amp"], 0.0, h["mean"], Xs)
        assert out["info"] > 0 and out["jitter"] > 0 and f["jitter"] > 0
        # the device's K and the host's differ by a few ulp: the schedule may stop one step apart on a singular K
        assert abs(math.log(out["jitter"] / f["jitter"])) <= math.log(1.1) * 1.0001, (out["jitter"], f["jitter"])
        g = R.lapack_fit(X, Y, h["lenscale_sq"], h["amp"], 0.0, h["mean"], Xs, jitter=out["jitter"])
        c.grid_upload(Xs)
        mu, var = c.gp_predict()
        assert relerr(mu[:, 0], g["mu"], floor=1e-3 * np.abs(g["mu"]).max()) < 1e-4
        assert np.max(np.abs(var - g["var"])) <= 1e-6 * h["amp"]


# ---- 4. nomination, fantasies, append ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("score", ["ei", "cb"])
def test_eval_nominate_against_the_host(paths, path, score):
    """b7_eval_nominate with S = 10 hyper samples on a Sobol grid: the accumulator against the host's mean of the S acquisition
    vectors (LAPACK fits), and the nominee the host's arg-max unless the host's top-2 gap is below the score bar."""
    from oracle import cport
    c = paths[path]
    N, d, M = 60, 6, 4096
    X, Y, _, h = _problem(N, d, 1, 5)
    Xs = cport.sobol(M, d, 1)
    hyps = [dict(h, lenscale_sq=h["lenscale_sq"] * (0.6 + 0.1 * s), amp=h["amp"] * (1 + 0.05 * s)) for s in range(10)]
    c.grid_upload(Xs)
    c.gp_set_data(X, Y)
    kw = {"score": "ei", "fmin": [float(Y.min())]} if score == "ei" else {"score": "cb"}
    v, i = c.eval_nominate(hyps, **kw)
    acc = c.score_finish(1.0, download=True)[2]
    host = np.zeros(M)
    for hh in hyps:
        f = R.lapack_fit(X, Y, hh["lenscale_sq"], hh["amp"], hh["noise"], hh["mean"], Xs)
        host += R.ei(f["mu"], f["var"], float(Y.min())) if score == "ei" else R.cb(f["mu"], f["var"])
    host /= len(hyps)
    bar = 1e-6 * np.max(np.abs(host))
    assert np.max(np.abs(acc - host)) <= bar
    best = int(np.argmax(host)) + 1
    if i != best:
        assert host[best - 1] - host[i - 1] <= 2 * bar, (i, best)
    assert v == acc[i - 1]


@pytest.mark.parametrize("path", ["small", "general"])
def test_fantasize_and_append_against_the_host(paths, path):
    c = paths[path]
    X, Y, Xs, h = _problem(61, 6, 700, 11)
    ls, amp, noise, mean = h["lenscale_sq"], h["amp"], h["noise"], h["mean"]
    c.gp_fit(X[:60], Y[:60], ls, amp, noise, mean)
    Xp = Xs[[5, 300, 650]]
    _, mu_p, cov_p = c.gp_fantasize(Xp, 16, seed=7, want_moments=True)
    f = R.lapack_fit(X[:60], Y[:60], ls, amp, noise, mean, Xp)
    from scipy.linalg import solve_triangular
    V = solve_triangular(f["L"], R.matern52(Xp, X[:60], ls, amp).T, lower=True)
    cov_o = R.matern52(Xp, None, ls, amp) - V.T @ V
    assert np.allclose(mu_p, f["mu"], rtol=1e-7, atol=1e-9)
    assert np.allclose(cov_p, cov_o, rtol=1e-6, atol=1e-8 * amp)
    c.gp_append(X[60], Y[60])
    g = R.lapack_fit(X, Y, ls, amp, noise, mean, Xs)
    L, alpha, _ = c.gp_download(61)
    assert np.allclose(L, g["L"], rtol=1e-9, atol=1e-12)
    c.grid_upload(Xs)
    mu, var = c.gp_predict()
    assert relerr(mu[:, 0], g["mu"], floor=1e-3 * np.abs(g["mu"]).max()) < REL and relerr(var, g["var"]) < REL


# ---- 5. switching kernels ------------------------------------------------------------------------------------------------------
def test_switching_kernels_drops_the_fit_and_comes_back_to_the_same_bits():
    import bot7_amd
    c, fresh = bot7_amd.Context(0), bot7_amd.Context(0)
    try:
        X, Y, Xs, h = _problem(90, 6, 2000, 3)
        args = (h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
        for k in (c, fresh):
            k.grid_upload(Xs)
        c.gp_fit(X, Y, *args)
        se_mu, se_var = c.gp_predict()
        token = c.fit_token
        c.gp_set_kernel("ardmatern52")
        assert c.fit_token == token + 1
        for call in (lambda: c.gp_predict(), lambda: c.gp_download(90), lambda: c.gp_append(X[0], Y[0]),
                     lambda: c.gp_fantasize(Xs[:2], 4)):
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call()
            assert e.value.code == -4
        c.gp_set_kernel("ardmatern52")                 # the same kernel again: nothing changes
        assert c.fit_token == token + 1
        c.gp_fit(X, Y, *args)
        m_mu, m_var = c.gp_predict()
        f = R.lapack_fit(X, Y, *args, Xs=Xs)
        assert relerr(m_mu[:, 0], f["mu"], floor=1e-3 * np.abs(f["mu"]).max()) < REL and relerr(m_var, f["var"]) < REL
        assert not np.array_equal(m_mu, se_mu)
        c.gp_set_kernel("ardse")
        c.gp_fit(X, Y, *args)
        fresh.gp_fit(X, Y, *args)
        a, b = c.gp_predict(), fresh.gp_predict()
        assert _bits(a[0]) == _bits(b[0]) == _bits(se_mu) and _bits(a[1]) == _bits(b[1]) == _bits(se_var)
        assert all(_bits(p) == _bits(q) for p, q in zip(c.gp_download(90), fresh.gp_download(90)))
        assert c._L.b7_gp_set_kernel(c._h, 7) == -1 and c._L.b7_gp_set_kernel(c._h, -1) == -1   # unknown kernels
        with pytest.raises(bot7_amd.Bot7HipError):
            c.gp_set_kernel("foo")
    finally:
        c.close()
        fresh.close()


def test_group_of_virtual_ranks_nominates_what_one_context_does():
    import bot7_amd
    from oracle import cport
    c = bot7_amd.Context(0)
    g = bot7_amd.Group([0, 0, 0])
    try:
        X, Y, _, h = _problem(70, 6, 1, 9)
        Xs = cport.sobol(5000, 6, 1)
        hyps = [dict(h, lenscale_sq=h["lenscale_sq"] * (0.7 + 0.1 * s)) for s in range(4)]
        c.gp_set_kernel("ardmatern52")
        g.gp_set_kernel("ardmatern52")
        assert all(m.kernel == 1 for m in g.members)
        c.grid_upload(Xs)
        g.grid_upload(Xs)
        c.gp_set_data(X, Y)
        g.gp_set_data(X, Y)
        want = c.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
        got = g.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
        assert got == want
        g.gp_set_kernel("ardse")
        se = g.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
        c.gp_set_kernel("ardse")
        assert se == c.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
    finally:
        g.close()
        c.close()


# ---- 6. the harness's trial loop --------------------------------------------------------------------------------------------
def test_default_regime_loop_under_matern_runs_clean_and_repeats():
    """20 trials of the reference's default experiment (hartmann6, 2e4 Sobol candidates, slice-sampled hypers, S = 10, EI) with
    config.model.kernel = 'ardmatern52', twice on fresh contexts: the same nominees, the same draws."""
    import bot7_amd
    from harness import default_regime as dr
    runs = []
    for _ in range(2):
        c = bot7_amd.Context(0)
        try:
            runs.append(dr.run(c, trials=20, kernel="ardmatern52"))
            assert c.kernel == 1
        finally:
            c.close()
    a, b = runs
    assert a["nominees"] == b["nominees"] and len(a["nominees"]) == 20
    assert dr.agreement(a, b) == (20, 0.0)
    assert np.isfinite(a["Y"]).all()
    print("Matern default loop nominees", a["nominees"])
