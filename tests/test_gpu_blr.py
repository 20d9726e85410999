"""The Bayesian-linear head of the DNGO model on every route, against exact arithmetic.  Needs an MI355X: run with -m gpu.

  a  blr_head_small_kernel through b7_blr_eval_nominate at the edges of its 64-observation chunk and 16-wide tiles
  b  b7_blr_fit / b7_blr_fit_x + b7_blr_features / b7_blr_basis + b7_blr_predict, the evidence, and a tanh head
  c  heads of 65 .. 256 features (the nine-launch general fit, every basis kernel), 257 refused
  d  the tall ring kernel (post_kernel_w4t<2,16>) on heads: feature rows, sign +1, + 1/beta
  e  the marginalised heads of b7_blr_eval_nominate_marg, fast and head by head
  f  the feature buffer's zero padding as state (feat_alloc)
  g  the failed-pivot redo (jitter_used = -2), constructed in exact arithmetic

References and bars: tests/_blr_ref.py (host tests: tests/test_blr_host.py).  Three kinds of check.  Against the 50-digit truth of
the float64 inputs, within _exact.gp_bar of LAPACK's own error on the same algebra (z <= 70).  Against the EXACT evaluation of
what a kernel was given (the downloaded L^-1 and weights), within bars derived from the operation count: they need no Cholesky,
hold at any width and catch a dropped row, a stale feature column or a wrong 1/beta whatever the head's condition number.  And
backward errors of the factor, its inverse and the weights against an A that is exact in float64, within the multiples of LAPACK's
that tests/test_gpu_numerics.py uses.  Every test prints its worst error / bar ratio (DESIGN.md records them)."""
import numpy as np
import pytest

import _blr_ref as R
import _exact as E
from conftest import make_network, make_problem

pytestmark = pytest.mark.gpu
ACT = "ReLU"
M_SMALL = 300
ROWS32 = np.linspace(0, M_SMALL - 1, 32).astype(int)
# the device forms A = beta G + alpha I with two roundings per entry (<= 2^-52 relative) and the truth's A is rounded once more
# to float64 (<= 2^-53): the distance between the A the device factors and the one its factor is judged against
A_GAP = 2 * E.EPS
NEAR_SINGULAR_FACTOR = 8 * E.EPS      # tests/test_gpu_numerics.py, at cond >= 1e10
_TRUTHS = {}


def _truth(key, Z0, Y, hyp, rows):
    if key not in _TRUTHS:
        _TRUTHS[key] = (R.blr_truth(Z0, Y, *hyp, rows), R.lapack_blr(Z0, Y, *hyp, rows))
    return _TRUTHS[key]


def _diag(monkeypatch, **env):
    """A context of the diagnostic build under the given switches (read at b7_create)."""
    import bot7_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return bot7_amd.Context(0, lib="diag")
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _ratio(err, bar):
    return err / bar if bar > 0.0 else (0.0 if err == 0.0 else np.inf)


def _launches(c, phase):
    return c.profile_get(phase)[1]


def _exact_checks(z, m, Li, Z1, hyp, mu, var, rows=None):
    """mean and variance against the exact evaluation of the downloaded m and L^-1 over the feature rows: worst error / bar."""
    _, beta, mean = hyp
    rows = np.arange(Z1.shape[0]) if rows is None else rows
    invbeta = 1.0 / beta
    assert (np.asarray(var) >= invbeta).all()
    hi, lo = R.exact_var_rows(Li, Z1[rows], invbeta)
    rv = float((E.abs_errors(np.asarray(var)[rows], hi, lo) / R.var_bar(z, hi)).max())
    mh, ml, ab = R.exact_mean_rows(m, Z1[rows], mean)
    rm = float((E.abs_errors(np.asarray(mu).ravel()[rows], mh, ml) / R.mean_bar(z, mean, ab)).max())
    assert rv <= 1.0 and rm <= 1.0, ("exact evaluation", z, rv, rm)
    return rv, rm


def _check_small_head(c, key, Z0, Y, Z1, hyp):
    """The fit c holds (any route) over the resident features of Z1's rows: factor, inverse, weights, predictions."""
    alpha, beta, mean = hyp
    z = Z0.shape[1]
    t, o = _truth(key, Z0, Y, hyp, Z1[ROWS32])
    L, m, Li = c.gp_download(z)
    m = m[:, 0]
    assert not np.triu(L, 1).any() and not np.triu(Li, 1).any()          # lower triangular: nothing of the padding leaks in
    ratios = {}
    bar = E.gp_bar(R.err_pairs(o["m"], t.m), float(np.abs(t.m[0]).max()))
    ratios["m / truth"] = _ratio(R.err_pairs(m, t.m), bar)
    # backward errors against the truth's A, LAPACK on the same A the yardstick; the floors are what one rounding of every entry
    # of an exact factor (inverse) costs: sqrt(z) eps -- LAPACK can be better than that by luck only at z = 1, 2
    q = Z0.T @ (beta * (np.asarray(Y).ravel() - mean))
    Ll, Lli, _ = R.lapack_head(t.A, q)
    g, ol = E.backward_errors(t.A, L, Li), E.backward_errors(t.A, Ll, Lli)
    cond = np.linalg.cond(t.A)
    floor = np.sqrt(z) * E.EPS
    ratios["factor"] = g[0] / (max(4 * ol[0], NEAR_SINGULAR_FACTOR if cond >= 1e10 else 0.0, floor) + A_GAP)
    ratios["inverse"] = g[1] / max(4 * ol[1], floor)
    mu, var = c.blr_predict()
    rv, rm = _exact_checks(z, m, Li, Z1, hyp, mu, var)
    ratios["var / exact"], ratios["mean / exact"] = rv, rm
    bar = E.gp_bar(R.err_pairs(o["var"], t.var), float(t.var[0].max()))
    ratios["var / truth"] = _ratio(R.err_pairs(var[ROWS32], t.var), bar)
    assert all(v <= 1.0 for v in ratios.values()), (key, ratios)
    return ratios, cond, (t, o)


def _report(name, ratios):
    worst = max(ratios, key=ratios.get)
    print("%s: worst error / bar %.3f (%s)  %s" % (name, ratios[worst], worst, {k: round(float(v), 3) for k, v in ratios.items()}))


def _merge(into, new):
    for k, v in new.items():
        into[k] = max(into.get(k, 0.0), v)


# ---- a. the small head, every edge ---------------------------------------------------------------------------------------------
def _nominate_and_check(c, p, hyp, small_route):
    alpha, beta, mean = hyp
    c.grid_upload(p.Xg)
    # the features are exact in float64 in any order: every basis kernel must return the host's bits
    assert np.array_equal(c.blr_basis(p.W, p.b, ACT, download=True), p.Z1)
    assert np.array_equal(c.blr_basis(p.W, p.b, ACT, X=p.X), p.Z0)
    c.profile_enable(True)
    c.profile_reset()
    try:
        # CB with tradeoff 0 and sign +1 is the mean itself: the fused mean of the basis kernel, left in the accumulator
        v, i, jit = c.blr_eval_nominate(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean, score="cb", tradeoff=0.0, sign=1.0,
                                        want_jitter=True)
        mean_launches, potrf_launches = _launches(c, "mean"), _launches(c, "potrf")
    finally:
        c.profile_enable(False)
    assert jit == 0.0
    # the route: blr_head_small_kernel is ONE "potrf" launch and the mean comes fused from the basis kernel, so no matrix-vector
    # launch at all; the general fit forms q = Z'(beta (y - mean)) with launch_gemv_rows (phase "mean")
    assert (mean_launches == 0 and potrf_launches == 1) if small_route else mean_launches >= 1, (mean_launches, potrf_launches)
    _, _, fused = c.score_finish(1.0, download=True)
    assert v == fused.max() and i == int(np.argmax(fused)) + 1
    ratios, cond, _ = _check_small_head(c, (p.N, p.z), p.Z0, p.Y, p.Z1, hyp)
    _, m, _ = c.gp_download(p.z)
    mh, ml, ab = R.exact_mean_rows(m[:, 0], p.Z1, mean)
    ratios["fused mean / exact"] = float((E.abs_errors(fused, mh, ml) / R.mean_bar(p.z, mean, ab)).max())
    assert ratios["fused mean / exact"] <= 1.0
    return ratios


@pytest.mark.parametrize("N,z", R.SMALL_CASES)
def test_a_small_head_at_every_edge(ctx, N, z):
    """N = 1, 63, 64, 65, 129 around the 64-observation chunk, z = 1, 16, 17, 48, 49, 63, 64 around the 16-wide tiles of G and the
    identity padding, N < z (alpha alone holds the head up), dead features (A_ii = alpha exactly): weights against the 50-digit
    truth, factor and inverse by backward error, b7_blr_predict's and the fused mean and the variance of 300 rows against the
    exact evaluation of the downloaded L^-1 and m, the variance of 32 rows against the truth."""
    p = R.problem(N, z, M_SMALL)
    if z >= 48:
        assert (p.Z0 == 0.0).all(0).any()            # dead features are part of the case
    ratios = _nominate_and_check(ctx, p, R.SMALL_HYP, small_route=True)
    _report("a N %d z %d" % (N, z), ratios)


@pytest.mark.parametrize("env", [{"B7_BLR_SMALL": "0"}, {"B7_NPAD_SMALL": "0"}], ids=["general-launches", "padded-to-128"])
@pytest.mark.parametrize("N,z", [(65, 49), (129, 64)])
def test_a_general_fit_arms_meet_the_same_bars(monkeypatch, N, z, env):
    """The same heads through the nine-launch general fit, 64-padded (B7_BLR_SMALL=0) and 128-padded (B7_NPAD_SMALL=0)."""
    c = _diag(monkeypatch, **env)
    try:
        ratios = _nominate_and_check(c, R.problem(N, z, M_SMALL), R.SMALL_HYP, small_route=False)
    finally:
        c.close()
    _report("a %s N %d z %d" % (sorted(env)[0], N, z), ratios)


# ---- b. the separate entry points -----------------------------------------------------------------------------------------------
def _nll_ratio(nll, t, o):
    bar = E.gp_bar(R.err_pairs([o["nll"]], t.nll), abs(float(t.nll[0][0])))
    return _ratio(R.err_pairs([nll], t.nll), bar)


@pytest.mark.parametrize("N,z", [(65, 49), (129, 64)])
def test_b_separate_entry_points(ctx, N, z):
    """b7_blr_fit (host features) + b7_blr_features + b7_blr_predict, and b7_blr_fit_x + b7_blr_basis + b7_blr_predict, to the truths
    of test a; the evidence (want_nll) to the truth's within gp_bar of LAPACK's own error."""
    p = R.problem(N, z, M_SMALL)
    alpha, beta, mean = R.SMALL_HYP
    worst = {}
    nll = ctx.blr_fit(p.Z0, p.Y, alpha, beta, mean, want_nll=True)
    ctx.blr_features(p.Z1)
    ratios, _, (t, o) = _check_small_head(ctx, (N, z), p.Z0, p.Y, p.Z1, R.SMALL_HYP)
    ratios["nll / truth"] = _nll_ratio(nll, t, o)
    _merge(worst, ratios)
    ctx.grid_upload(p.Xg)
    nll = ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean, want_nll=True)
    ctx.blr_basis(p.W, p.b, ACT)
    ratios, _, _ = _check_small_head(ctx, (N, z), p.Z0, p.Y, p.Z1, R.SMALL_HYP)
    ratios["nll / truth"] = _nll_ratio(nll, t, o)
    _merge(worst, ratios)
    assert worst["nll / truth"] <= 1.0
    _report("b N %d z %d" % (N, z), worst)


def test_b_tanh_head_at_the_workloads_conditioning(ctx, orc):
    """The workload's 3 x 50 tanh basis, N = 80: the features are downloaded from b7_blr_basis and taken as given, so the head is
    judged on them alone, at the condition number of a real DNGO head (printed)."""
    d, N = 6, 80
    W, b = make_network(d, (50, 50, 50), seed=d)
    X, Y, Xg, _ = make_problem(ctx, orc, d, N, M_SMALL, lambda X: np.sin(3 * X.sum(axis=1, keepdims=True)))
    hyp = (2.0, 1.0 / (1e-2 * float(np.var(Y))), float(np.mean(Y)))
    ctx.grid_upload(Xg)
    Z1 = ctx.blr_basis(W, b, "Tanh", download=True)
    Z0 = ctx.blr_basis(W, b, "Tanh", X=X)
    worst = {}
    nll = ctx.blr_fit(Z0, Y, *hyp, want_nll=True)
    ctx.blr_features(Z1)
    ratios, cond, (t, o) = _check_small_head(ctx, "tanh", Z0, Y, Z1, hyp)
    ratios["nll / truth"] = _nll_ratio(nll, t, o)
    _merge(worst, ratios)
    ctx.grid_upload(Xg)
    nll = ctx.blr_fit_x(W, b, "Tanh", X, Y, *hyp, want_nll=True)
    ctx.blr_basis(W, b, "Tanh")
    ratios, _, _ = _check_small_head(ctx, "tanh", Z0, Y, Z1, hyp)
    ratios["nll / truth"] = _nll_ratio(nll, t, o)
    _merge(worst, ratios)
    assert worst["nll / truth"] <= 1.0
    print("b tanh: cond(A) = %.3e" % cond)
    _report("b tanh 3x50 N 80", worst)
    assert 1e4 <= cond <= 1e10


# ---- c. wide heads ---------------------------------------------------------------------------------------------------------------
def _check_wide_head(c, p, hyp, rows):
    """Backward errors of the fit c holds against the EXACT A and q (R.exact_head), LAPACK doing the same algebra the yardstick,
    and mean / variance of the given rows against the exact evaluation."""
    A, q = R.exact_head(p.Z0, p.Y, *hyp)
    L, m, Li = c.gp_download(p.z)
    m = m[:, 0]
    assert not np.triu(L, 1).any() and not np.triu(Li, 1).any()
    Ll, Lli, ml = R.lapack_head(A, q)
    g, o = E.backward_errors(A, L, Li), E.backward_errors(A, Ll, Lli)
    cond = np.linalg.cond(A)
    near = NEAR_SINGULAR_FACTOR if cond >= 1e10 else 0.0
    res, res_l = R.solve_residual(A, m, q), R.solve_residual(A, ml, q)
    print("N %d z %d: cond %.2e: factor %.3g (LAPACK %.3g), inverse %.3g (LAPACK %.3g), residual %.3g (LAPACK %.3g)"
          % (p.N, p.z, cond, g[0], o[0], g[1], o[1], res, res_l))
    ratios = {"factor": g[0] / max(4 * o[0], near), "inverse": g[1] / (4 * o[1]), "residual": res / max(4 * res_l, near)}
    mu, var = c.blr_predict()
    ratios["var / exact"], ratios["mean / exact"] = _exact_checks(p.z, m, Li, p.Z1, hyp, mu, var, rows)
    assert all(v <= 1.0 for v in ratios.values()), (p.N, p.z, cond, ratios)
    return ratios, (mu, var)


@pytest.mark.parametrize("N,z", R.WIDE_CASES)
def test_c_wide_heads(ctx, N, z):
    """z = 65 .. 256 (padded to 128 and 256; z > 128 takes the widest basis kernel), N around a 16-multiple, 300, and N = 10 < z:
    ||L L' - A|| / ||A||, ||L^-1 L - I|| and ||A m - q|| / (||A|| ||m|| + ||q||) in long double against an A and a q that are exact
    in float64, each within 4 x LAPACK's; mean and variance of 64 rows against the exact evaluation."""
    p = R.problem(N, z, M_SMALL)
    alpha, beta, mean = R.WIDE_HYP
    ctx.grid_upload(p.Xg)
    assert np.array_equal(ctx.blr_basis(p.W, p.b, ACT, X=p.X), p.Z0)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean)
        assert _launches(ctx, "mean") >= 1 and _launches(ctx, "potrf") >= 1            # the general fit: q by launch_gemv_rows
    finally:
        ctx.profile_enable(False)
    assert np.array_equal(ctx.blr_basis(p.W, p.b, ACT, download=True), p.Z1)
    rows = np.linspace(0, M_SMALL - 1, 64).astype(int)
    ratios, _ = _check_wide_head(ctx, p, R.WIDE_HYP, rows)
    _report("c N %d z %d" % (N, z), ratios)


def test_c_257_features_are_refused(ctx):
    from bot7_amd import Bot7HipError
    p = R.problem(16, 257, 4)
    ctx.grid_upload(p.Xg)
    for call in (lambda: ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, *R.WIDE_HYP),
                 lambda: ctx.blr_eval_nominate(p.W, p.b, ACT, p.X, p.Y, *R.WIDE_HYP, score="cb")):
        with pytest.raises(Bot7HipError) as e:
            call()
        assert e.value.code == -5           # B7_ERR_UNSUPPORTED


# ---- d. the tall ring kernel on heads ------------------------------------------------------------------------------------------------
M_TALL = 65536 + 77


def _tall_predict(c, p):
    c.grid_upload(p.Xg)
    c.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, *R.WIDE_HYP)
    c.blr_basis(p.W, p.b, ACT)
    return c.blr_predict()


@pytest.mark.parametrize("z", [200, 256])
def test_d_tall_ring_kernel_on_a_head(ctx, z):
    """A head padded to 256 over 65 613 feature rows is served by post_kernel_w4t<2,16> (one 256-row workgroup per CU at least:
    asserted from the device's CU count), with feature rows for K*, sign +1 and + 1/beta; the first 4096 rows alone go through the
    128-candidate kernel and must give the same bits; 64 sampled rows and the last 77 against the exact evaluation."""
    p = R.problem(300, z, M_TALL)
    cus = ctx.device_info()["compute_units"]
    assert (M_TALL + 255) // 256 >= cus and 4096 // 256 < cus
    mu, var = _tall_predict(ctx, p)
    ratios, _ = _check_wide_head(ctx, p, R.WIDE_HYP, np.concatenate([np.linspace(0, M_TALL - 78, 64).astype(int),
                                                                     np.arange(M_TALL - 77, M_TALL)]))
    ctx.grid_upload(p.Xg[:4096])
    ctx.blr_basis(p.W, p.b, ACT)
    mu_s, var_s = ctx.blr_predict()
    assert np.array_equal(var[:4096], var_s) and np.array_equal(mu[:4096], mu_s)
    _report("d z %d" % z, ratios)


def test_d_a_repeated_head_prediction_sees_nothing_of_the_one_before(ctx):
    """tests/test_gpu_post_ring.py's pattern with a z = 200 and a z = 256 head alternating on the tall kernel."""
    A, B = R.problem(300, 200, M_TALL), R.problem(40, 256, M_TALL)
    mu0, var0 = _tall_predict(ctx, A)
    mub, varb = _tall_predict(ctx, B)
    mu1, var1 = _tall_predict(ctx, A)
    mub2, varb2 = _tall_predict(ctx, B)
    mu2, var2 = _tall_predict(ctx, A)
    assert np.array_equal(var0, var1) and np.array_equal(var0, var2) and np.array_equal(varb, varb2)
    assert np.array_equal(mu0, mu1) and np.array_equal(mu0, mu2) and np.array_equal(mub, mub2)


# ---- e. marginalised heads --------------------------------------------------------------------------------------------------------
MARG_AL, MARG_BE, MARG_MN = [0.37, 0.61, 1.3], [83.0, 40.5, 120.25], [0.11, -0.07, 0.2]


def _score(c, kind, fmin):
    if kind == "ei":
        c.score_ei(fmin, 0.0)
    else:
        c.score_cb()


@pytest.mark.parametrize("kind", ["cb", "ei"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("z", [49, 70])
def test_e_marginalised_heads(ctx, z, S, kind):
    """S heads with distinct alpha, beta and mean over N = 65, M = 1000.  The evidence of every head against the truth.  z = 49 (S
    workgroups of blr_head_small_kernel, one batched mean launch, launch_post_heads with per-sample 1/beta): blr_small.hip promises
    the single head's rounded operations, so the accumulator must equal ((g_0 + g_1) + g_2) / S BIT FOR BIT, g_s the scores of
    the head b7_blr_eval_nominate fits under sample s's hypers.  z = 70 (head by head): the same against b7_blr_fit_x +
    b7_blr_predict + b7_score_* per sample.

    Which g_s: b7_blr_eval_nominate's OWN accumulator takes its mean from the basis kernel (four fma chains per row, folded:
    extras.hip, mlp_resident_kernel), the marginalised route from gemv_rows64_multi_kernel (the wave-butterfly tree of
    gemv_rows_kernel, products unfused).  Same operands, another order of summation: that accumulator differs in the last bits of
    the mean and nowhere else.  So g_s is taken from the head b7_blr_eval_nominate LEFT in the context, predicted by
    b7_blr_predict (gemv_rows_kernel) and scored by b7_score_*: bit for bit.  (This caught gemv_rows64_multi_kernel with the first
    level of its tree contracted into fma: 38 .. 62 % of the entries differed by up to 2.2e-15 until contraction went off there.)
    The fused-mean accumulator is compared as well: its
    distance must be explained by the two mean bars alone (CB: twice the exact-evaluation bar of the mean plus the rounding of
    the score's own two operations); the count of differing entries is printed."""
    N, M = 65, 1000
    p = R.problem(N, z, M)
    al, be, mn = MARG_AL[:S], MARG_BE[:S], MARG_MN[:S]
    fmin = [float(p.Y.min())]
    ctx.grid_upload(p.Xg)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        v, i, jit, nll = ctx.blr_eval_nominate_marg(p.W, p.b, ACT, p.X, p.Y, al, be, mn, score=kind, fmin=fmin, want_nll=True)
        mean_launches, potrf_launches = _launches(ctx, "mean"), _launches(ctx, "potrf")
    finally:
        ctx.profile_enable(False)
    _, _, acc = ctx.score_finish(1.0, download=True)
    assert jit == 0.0
    # the fast route: S heads in ONE "potrf" launch, S means in ONE "mean" launch; head by head: q and the mean of every head
    assert (mean_launches, potrf_launches) == (1, 1) if z <= 64 else (mean_launches >= 2 * S and potrf_launches >= S)
    ratios = {}
    for s in range(S):
        t, o = _truth(("marg", z, s), p.Z0, p.Y, (al[s], be[s], mn[s]), p.Z1[:1])
        ratios["nll / truth"] = max(ratios.get("nll / truth", 0.0), _nll_ratio(nll[s], t, o))
    assert ratios["nll / truth"] <= 1.0
    want = np.zeros(M)
    if z <= 64:
        fused, slack, mag = np.zeros(M), np.zeros(M), np.zeros(M)
        for s in range(S):
            ctx.blr_eval_nominate(p.W, p.b, ACT, p.X, p.Y, al[s], be[s], mn[s], score=kind, fmin=fmin)
            _, _, g_fused = ctx.score_finish(1.0, download=True)
            fused = fused + g_fused
            _, m, _ = ctx.gp_download(z)
            slack = slack + 2 * R.mean_bar(z, mn[s], np.abs(p.Z1 * m[:, 0]).sum(1)) + 4 * R.U * np.abs(g_fused)
            mag = mag + np.abs(g_fused)
            ctx.blr_predict(download=False)
            ctx.score_reset()
            _score(ctx, kind, fmin)
            _, _, g = ctx.score_finish(1.0, download=True)
            want = want + g
        want, fused = want / S, fused / S
        differing = int((fused != acc).sum())
        print("e z %d S %d %s: %d of %d entries differ from the fused-mean accumulators (max %.3g)" % (
            z, S, kind, differing, M, float(np.abs(fused - acc).max())))
        if kind == "cb":
            # + the S additions and the division of either accumulation: (S + 1) 2^-53 sum |g_s| / S on each side
            ratios["fused-mean accumulator"] = float((np.abs(fused - acc) / ((slack + 2 * (S + 1) * R.U * mag) / S)).max())
            assert ratios["fused-mean accumulator"] <= 1.0
        v0, i0 = float(want.max()), int(np.argmax(want)) + 1
    else:
        for s in range(S):
            ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, al[s], be[s], mn[s])
            ctx.blr_basis(p.W, p.b, ACT)
            ctx.blr_predict(download=False)
            if s == 0:
                ctx.score_reset()
            _score(ctx, kind, fmin)
        v0, i0, want = ctx.score_finish(float(S), download=True)
    assert np.array_equal(acc, want), "%d of %d entries differ, max %.3g" % ((acc != want).sum(), M, np.abs(acc - want).max())
    assert (v, i) == (v0, i0)
    _report("e z %d S %d %s" % (z, S, kind), ratios)


# ---- f. the feature buffer as state -----------------------------------------------------------------------------------------------
def test_f_feature_buffer_padding_survives_changes_of_width_and_rows():
    """feat_alloc zeroes the buffer only when it grows or the width changes; the variance kernel reads whole padded rows.  One
    context through z = 64 / M = 3000, z = 50 / M = 3000, z = 64 / M = 257, z = 64 / M = 3000, host features z = 50 / M = 300,
    z = 130 / M = 300: after every step b7_blr_predict must equal, bit for bit, a fresh context doing that step alone."""
    import bot7_amd
    alpha, beta, mean = R.SMALL_HYP
    N = 40
    P = {z: R.problem(N, z, 3000) for z in (64, 50, 130)}

    def by_basis(z, M):
        def step(c):
            p = P[z]
            c.grid_upload(p.Xg[:M])
            c.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean)
            c.blr_basis(p.W, p.b, ACT)
            return c.blr_predict()
        return step

    def by_features(z, M):
        def step(c):
            p = P[z]
            c.blr_fit(p.Z0, p.Y, alpha, beta, mean)
            c.blr_features(p.Z1[:M])
            return c.blr_predict()
        return step

    steps = [by_basis(64, 3000), by_basis(50, 3000), by_basis(64, 257), by_basis(64, 3000), by_features(50, 300), by_basis(130, 300)]
    one = bot7_amd.Context(0)
    try:
        for k, step in enumerate(steps):
            mu, var = step(one)
            fresh = bot7_amd.Context(0)
            try:
                mu_f, var_f = step(fresh)
            finally:
                fresh.close()
            assert np.array_equal(var, var_f) and np.array_equal(mu, mu_f), "step %d" % k
    finally:
        one.close()


# ---- g. the failed pivot --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cb", "ei"])
def test_g_failed_pivot_is_redone_through_the_jitter_schedule(ctx, kind):
    """R.pivot_case: A_11 = A_21 = A_22 = 16 in float64, so the second pivot of the plain attempt is exactly 0 (checked on the host
    in tests/test_blr_host.py).  Both nominate entry points must report -2 and give the value, the index and the accumulator of
    b7_blr_fit_x (the jitter schedule) + b7_blr_basis + b7_blr_predict + b7_score_*, bit for bit: the redo is that route."""
    W, b, X, Y, alpha, beta = R.pivot_case()
    Z0 = R.dyadic_features(X, W, b)
    assert E.min_pivot(beta * (Z0.T @ Z0) + alpha * np.eye(Z0.shape[1])) == 0.0
    Xg = R.dyadic_points(500, R.D, 99)
    fmin = [float(Y.min())]
    ctx.grid_upload(Xg)
    v, i, jit = ctx.blr_eval_nominate(W, b, ACT, X, Y, alpha, beta, 0.25, score=kind, fmin=fmin, want_jitter=True)
    _, _, acc = ctx.score_finish(1.0, download=True)
    assert jit == -2.0
    ctx.blr_fit_x(W, b, ACT, X, Y, alpha, beta, 0.25)
    ctx.blr_basis(W, b, ACT)
    ctx.blr_predict(download=False)
    ctx.score_reset()
    _score(ctx, kind, fmin)
    v0, i0, acc0 = ctx.score_finish(1.0, download=True)
    assert np.isfinite(acc0).all()
    assert np.array_equal(acc, acc0) and (v, i) == (v0, i0)
    # S = 2 heads, both with a zero second pivot (beta = 1: 16 - 4 * 4; beta = 4: 64 - 8 * 8)
    al, be, mn = [alpha, alpha], [1.0, 4.0], [0.25, 0.125]
    v, i, jit = ctx.blr_eval_nominate_marg(W, b, ACT, X, Y, al, be, mn, score=kind, fmin=fmin)
    _, _, acc = ctx.score_finish(1.0, download=True)
    assert jit == -2.0
    for s in range(2):
        ctx.blr_fit_x(W, b, ACT, X, Y, al[s], be[s], mn[s])
        ctx.blr_basis(W, b, ACT)
        ctx.blr_predict(download=False)
        if s == 0:
            ctx.score_reset()
        _score(ctx, kind, fmin)
    v0, i0, acc0 = ctx.score_finish(2.0, download=True)
    assert np.isfinite(acc0).all()
    assert np.array_equal(acc, acc0) and (v, i) == (v0, i0)
