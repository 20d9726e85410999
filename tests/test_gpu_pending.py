"""Multi-column fits, pending-point fantasies and append chains against exact arithmetic.  Host references: tests/_pending_ref.py
(R; checked on the CPU by tests/test_pending_host.py) and tests/_exact.py (E).  u = 2^-53, eps = 2^-52.

Every bar is one of: derived (the comment or the reference's docstring says how); a named constant of the suite (K_GAP,
NEAR_SINGULAR_FACTOR, the 4-ulp draw figure DRAW_ULP, gp_bar's 8 x / 16 eps, the 4 x of the corner test); or a multiple of a
yardstick computed in the same test from a host reference (LAPACK, the float64 restatement of the chain), never from the device.

  A. c > 1 response columns (trmv_lower*_kernel over columns, mean_multi_kernel's 128 x 64 tile, nll_terms_kernel's column
     branch): alpha against the device's own L^-1 and the mean against the device's own alpha with derived componentwise bars,
     NLL / mean / variance per column against 50 digits, bit-exact column invariances, the c = 257 refusal, eval_nominate.
     Check 4 as the issue states it: no summation order in these kernels depends on a column's position (each column of
     trmv_lower_kernel, trmv_lower_t_part / _sum_kernel and of a GemmF64 tile runs the same products in the same order), so every
     item of it is held bit for bit.
  B. b7_gp_fantasize's moments: against 50 digits, against the device's own factor (derived), symmetry, var_with_noise.
  C. its draws: Y = mu + Lp Z with Z restated from the counter layout z(k, s) = counter_normal(seed, k n + s); the factor
     recovered from the draws is lower triangular and squares to cov_out + j I; the jitter loop; the layout's dependence on n.
  D. b7_gp_append chains from 3, 65, 129 and 257 observations at the covariance corners: backward errors against LAPACK's and
     the restated chain's, every intermediate state of one chain, refusals, near-duplicates, c = 3, Matern.

Each test prints its worst ratio to the bar.  Measured on an MI355X (also in DESIGN.md, section 8):
  A. alpha 0.017 of its bar; mean 0.76 at N = 1 (the bar is K_GAP alone there), 0.27 at N = 2, <= 0.024 from N = 63; Matern 0.006 /
     0.009; against 50 digits the error is 1.04 (NLL), 2.10 (mean), 1.03 (variance) x LAPACK's, bar 8 x.
  B. against 50 digits 3.23 (mean) and 1.00 (covariance) x LAPACK's; covariance against the device's factor 0.14 of its bar at N = 3,
     <= 3e-4 otherwise; mean 0.02; cov_out is symmetric bit for bit.
  C. one pending point 3.00 ulp (bar 8; 110 of 257 draws cancel and take the ulp of the larger term, the others are within 1.00
     ulp of the value itself); recovered factor: upper triangle 0.038 of Delta, residual 0.052 of its bar; both singular
     constructions jitter at the schedule's first step, 1.1e-8, where dpotrf fails too.
  D. chains: factor 0.45, inverse 0.79 of the bars (35 chains; (257 -> 300, 1) corner 2 needs jitter at n0 and is left out); every state of
     65 -> 128: alpha 0.003, mean 1.51 and variance 1.08 x LAPACK's error; the device refuses at n = 105 / 87 on (128, 1) corners
     2 / 3, where the restatement does; Matern 65 -> 80: 0.07, 0.25."""
import math
import os

import numpy as np
import pytest
from scipy.linalg import lapack

import _exact as E
import _pending_ref as R
from oracle import gp

pytestmark = pytest.mark.gpu
GENERAL = {"B7_FIT_SMALL": "0", "B7_KPOST_SMALL": "0", "B7_NLL_SMALL": "0"}
LD = np.longdouble


@pytest.fixture(scope="module")
def gen():
    """A context of the diagnostic build with every small-problem kernel switched off (switches are read at b7_create)."""
    import bot7_amd
    old = {k: os.environ.get(k) for k in GENERAL}
    os.environ.update(GENERAL)
    try:
        c = bot7_amd.Context(0, lib="diag")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _fit(c, X, Y, h, **kw):
    return c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], **kw)


def _ratio(got, ref, bar):
    """max |got - ref| / bar (long double difference); a zero bar passes only a zero error."""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(np.max(q))


def _check_alpha(c, N, cols, Y, h, tag):
    """A.1: the device's alpha against Linv' (Linv r) of its own downloaded Linv; R.alpha_ref_bar derives the bar."""
    L, alpha, Linv = c.gp_download(N, cols)
    ref, bar = R.alpha_ref_bar(Linv, np.asarray(Y, dtype=np.float64).reshape(N, cols) - h["mean"], R.npad(N))
    q = _ratio(alpha, ref, bar)
    assert q <= 1.0, "%s: alpha at %.3f of its derived bar" % (tag, q)
    return L, alpha, Linv, q


def _check_mean(mu, Ks, alpha, h, N, tag, k_gap=R.K_GAP):
    """A.2: the device's mean against mean + K* alpha of its own alpha on the host's K*; R.mean_ref_bar derives the bar."""
    ref, bar = R.mean_ref_bar(Ks, alpha, h["mean"], R.npad(N), k_gap)
    q = _ratio(mu, ref, bar)
    assert q <= 1.0, "%s: mean at %.3f of its derived bar" % (tag, q)
    return q


# ---- A. multi-column fits ---------------------------------------------------------------------------------------------------------
# a cross, not a product: every N at c = 65, every c at N = 65, every M at (65, 65); d = 1 at two shapes; (N, c, M, d, workspace)
A_CASES = ([(N, 65, 129, 6, None) for N in (1, 2, 63, 64, 65, 128, 129, 256, 257)]
           + [(65, c, 129, 6, None) for c in (2, 63, 64, 128, 129, 256)]
           + [(65, 65, M, 6, None) for M in (1, 127, 128, 300)]
           + [(65, 65, 129, 1, None), (257, 2, 300, 1, None), (129, 256, 300, 6, None)]
           + [(65, 65, 300, 6, 8 * 256 * 128)])        # one 256-row chunk per launch: the second chunk has row0 = 256


@pytest.mark.parametrize("N,cols,M,d,workspace", A_CASES)
def test_multi_column_alpha_and_mean_against_the_devices_own_factor(ctx, N, cols, M, d, workspace):
    X, Y = R.multi_data(N, d, cols, seed=1000 * N + cols)
    Xs = R.grid_points(M, d, seed=M)
    h = R.grid_hyp(d, mean=0.25)
    tag = "N %d c %d M %d d %d" % (N, cols, M, d)
    try:
        if workspace:
            ctx.set_workspace(workspace)
        assert _fit(ctx, X, Y, h)["jitter"] == 0
        _, alpha, _, qa = _check_alpha(ctx, N, cols, Y, h, tag)
        ctx.grid_upload(Xs)
        mu, var = ctx.gp_predict()
        assert mu.shape == (M, cols)
        qm = _check_mean(mu, gp.ardse(Xs, X, h["lenscale_sq"], h["amp"]), alpha, h, N, tag)
    finally:
        if workspace:
            ctx.set_workspace(4 << 30)
    print("%s: alpha %.4f, mean %.4f of the derived bars" % (tag, qa, qm))


def test_multi_column_alpha_and_mean_under_the_matern_kernel(ctx):
    import _matern_ref as MR
    N, cols, M, d = 65, 65, 129, 6
    X, Y = R.multi_data(N, d, cols, seed=3)
    Xs = R.grid_points(M, d, seed=4)
    h = R.grid_hyp(d, j=0, mean=0.25)
    ctx.gp_set_kernel("ardmatern52")
    try:
        assert _fit(ctx, X, Y, h)["jitter"] == 0
        _, alpha, _, qa = _check_alpha(ctx, N, cols, Y, h, "matern")
        ctx.grid_upload(Xs)
        mu, _ = ctx.gp_predict()
        qm = _check_mean(mu, MR.matern52(Xs, X, h["lenscale_sq"], h["amp"]), alpha, h, N, "matern",
                         k_gap=R.matern_gap(Xs, X, h["lenscale_sq"]))
    finally:
        ctx.gp_set_kernel("ardse")
    print("matern N 65 c 65: alpha %.4f, mean %.4f of the derived bars" % (qa, qm))


def _judge(what, got, truth, orcs, scale, worst):
    e_g, e_o = E.err_vs(got, truth), max(E.err_vs(o, truth) for o in orcs)
    worst[what] = max(worst.get(what, 0.0), e_g / max(e_o, 16 * E.EPS * scale))
    assert e_g <= E.gp_bar(e_o, scale), "%s: GPU error %.3g, LAPACK %.3g, scale %.3g" % (what, e_g, e_o, scale)


def _small_data(N, cols, seed):
    rng = np.random.default_rng(seed)
    d = 1 if N == 2 else 2
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0])
    Y = y[:, None] + 0.1 * rng.normal(size=(N, cols))
    return X, (Y - Y.mean()) / Y.std(), rng.random((8, d))


@pytest.mark.parametrize("N", [2, 16])
def test_multi_column_nll_mean_and_variance_against_50_digits(ctx, N):
    """A.3: c = 3 at two corners of the hyper box and an interior point; per column the NLL, mean and variance against
    E.gp_truth of that column, bar E.gp_bar of LAPACK's error (on K and on K with its off-diagonals 1 -+ eps, as _judge does)."""
    X, Y, Xs = _small_data(N, 3, seed=N)
    worst, judged = {}, 0
    for hi_, h in enumerate(R.box_hyps(X, Y, seed=N)):
        ctx.grid_upload(Xs)
        rep = _fit(ctx, X, Y, h, want_nll=True)
        jit = rep["jitter"]
        if jit < 0:
            continue
        mu, var = ctx.gp_predict()
        for k in range(3):
            args = (X, Y[:, k], h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xs)
            orcs = [E.lapack_fit(*args, jitter=jit, kscale=ks) for ks in (1.0, 1.0 - E.EPS, 1.0 + E.EPS)]
            orcs = [o for o in orcs if o is not None]
            if not orcs:
                continue
            t = E.gp_truth(*args, jitter=jit)
            _judge("nll", [rep["nll"][k]], [t.nll], [[o[0]] for o in orcs], abs(float(t.nll)), worst)
            _judge("mean", mu[:, k], t.mu, [o[1] for o in orcs], math.sqrt(h["amp"]) + abs(h["mean"]), worst)
            if k == 0:
                _judge("var", var, t.var, [o[2] for o in orcs], h["amp"], worst)
            judged += 1
    assert judged >= 6
    print("N %d c 3: worst GPU / LAPACK error ratios %s" % (N, {k: round(v, 3) for k, v in worst.items()}))


def test_multi_column_invariances_are_exact(ctx, gen):
    """A.4, all bit for bit: a column repeated at positions 0, 63, 64 and c - 1 (c = 129); a column permutation; and on the
    diagnostic context L, Linv and var of the c-column fit against the one-column fit (they do not read Y)."""
    N, cols, M, d = 65, 129, 129, 6
    X, Y = R.multi_data(N, d, cols, seed=11)
    Xs = R.grid_points(M, d, seed=12)
    h = R.grid_hyp(d, mean=0.25)
    rep_at = [0, 63, 64, cols - 1]
    Y[:, rep_at] = Y[:, [5]]
    perm = np.random.default_rng(13).permutation(cols)
    out = {}
    for c, name in ((ctx, "default"), (gen, "general")):
        c.grid_upload(Xs)
        _fit(c, X, Y, h)
        L, alpha, Linv = c.gp_download(N, cols)
        mu, var = c.gp_predict()
        for p in rep_at[1:]:
            assert _bits(alpha[:, p]) == _bits(alpha[:, 0]) and _bits(mu[:, p]) == _bits(mu[:, 0]), (name, p)
        _fit(c, X, Y[:, perm], h)
        _, alpha_p, _ = c.gp_download(N, cols)
        mu_p, var_p = c.gp_predict()
        assert _bits(alpha_p) == _bits(alpha[:, perm]) and _bits(mu_p) == _bits(mu[:, perm]) and _bits(var_p) == _bits(var), name
        out[name] = (L, Linv, var)
    _fit(gen, X, Y[:, :1], h)
    L1, a1, Linv1 = gen.gp_download(N, 1)
    _, var1 = gen.gp_predict()
    L, Linv, var = out["general"]
    assert _bits(L) == _bits(L1) and _bits(Linv) == _bits(Linv1) and _bits(var) == _bits(var1)


def test_257_columns_are_refused_and_the_previous_fit_stays_usable(ctx):
    import bot7_amd
    X, Y = R.multi_data(20, 2, 257, seed=2)
    h = R.grid_hyp(2)
    ctx.grid_upload(R.grid_points(40, 2, seed=3))
    _fit(ctx, X, Y[:, :256], h)
    before = ctx.gp_predict()
    state = [_bits(a) for a in ctx.gp_download(20, 256)]
    for call in (lambda: ctx.gp_set_data(X, Y), lambda: _fit(ctx, X, Y, h)):
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            call()
        assert e.value.code == -5                 # B7_ERR_UNSUPPORTED: "gp_set_data: ycols 257 > 256"
        after = ctx.gp_predict()
        assert _bits(after[0]) == _bits(before[0]) and _bits(after[1]) == _bits(before[1])
        assert [_bits(a) for a in ctx.gp_download(20, 256)] == state       # L, alpha (256 columns) and Linv as before the call


@pytest.mark.parametrize("cols", [2, 65])
@pytest.mark.parametrize("score", ["ei", "logei"])
def test_eval_nominate_with_c_columns_is_the_per_sample_loop(ctx, cols, score):
    """A.6: N = 65, S = 3: accumulator and nominee of b7_eval_nominate bit for bit those of fit, predict, score_*, score_finish."""
    N, d, M, S = 65, 6, 300, 3
    X, Y = R.multi_data(N, d, cols, seed=cols)
    h = R.grid_hyp(d, mean=0.1)
    hyps = [dict(h, lenscale_sq=h["lenscale_sq"] * (1 + 0.05 * s), amp=h["amp"] * (1 + 0.03 * s)) for s in range(S)]
    fmin = Y.min(axis=0)
    ctx.grid_upload(R.grid_points(M, d, seed=7))
    for s, hs in enumerate(hyps):
        _fit(ctx, X, Y, hs)
        ctx.gp_predict(download=False)
        if s == 0:
            ctx.score_reset()
        (ctx.score_ei if score == "ei" else ctx.score_logei)(fmin, 0.0)
    val0, idx0, sc0 = ctx.score_finish(float(S), download=True)
    ctx.gp_set_data(X, Y)
    val1, idx1, rep = ctx.eval_nominate(hyps, score=score, fmin=fmin, want_report=True)
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    assert not rep["jitter"].any()
    assert idx1 == idx0 and _bits([val1]) == _bits([val0]) and _bits(sc1) == _bits(sc0)


# ---- B. fantasies: moments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(2, 1), (2, 3), (16, 1), (16, 3)])
def test_fantasy_moments_against_50_digits(ctx, N, P):
    """B.1: mean_out and cov_out against R.gp_cov_truth; yardstick LAPACK on the host's K and on K with its off-diagonals 1 -+ eps."""
    X, Y, Xs = _small_data(N, 1, seed=10 + N)
    Xp = Xs[:P]
    worst, judged = {}, 0
    for h in R.box_hyps(X, Y, seed=N):
        jit = _fit(ctx, X, Y, h)["jitter"]
        if jit < 0:
            continue
        _, mu, cov = ctx.gp_fantasize(Xp, 4, seed=1, want_moments=True)
        orcs = [R.lapack_cov(X, Y, h, Xp, jitter=jit, kscale=ks) for ks in (1.0, 1.0 - E.EPS, 1.0 + E.EPS)]
        orcs = [o for o in orcs if o is not None]
        if not orcs:
            continue
        mu_t, cov_t = R.gp_cov_truth(X, Y, h, Xp, jitter=jit)
        _judge("mean", mu, mu_t, [o[0] for o in orcs], math.sqrt(h["amp"]) + abs(h["mean"]), worst)
        _judge("cov", cov.ravel(), R.mp_flat(cov_t), [o[1].ravel() for o in orcs], h["amp"], worst)
        judged += 1
    assert judged >= 2
    print("N %d P %d: worst GPU / LAPACK error ratios %s" % (N, P, {k: round(v, 3) for k, v in worst.items()}))


B_CASES = ([(65, P, 6) for P in (1, 2, 63, 64)] + [(N, 64, 6) for N in (3, 64, 129, 257)] + [(65, 2, 1), (257, 64, 1), (3, 1, 1)])


@pytest.mark.parametrize("N,P,d", B_CASES)
def test_fantasy_moments_against_the_devices_own_factor(ctx, N, P, d):
    """B.2 - B.4 at noise = 1e-2 amp on grid inputs: cov_out against K(Xp, Xp) - V V', V = K_p Linv' of the downloaded Linv
    (R.cov_ref_bar derives the bar), mean_out with A.2's bar, symmetry within the same bar, and var_with_noise: off-diagonals
    the same bits, each diagonal entry fl(v + noise)."""
    X, Y = E.grid_data(max(N, 2), d, seed=N)
    X, Y = X[:N], Y[:N]
    Xp = R.grid_points(P, d, seed=100 + P)
    h = R.grid_hyp(d, mean=0.25)
    tag = "N %d P %d d %d" % (N, P, d)
    assert _fit(ctx, X, Y, h)["jitter"] == 0
    _, alpha, Linv, _ = _check_alpha(ctx, N, 1, Y, h, tag)
    _, mu, cov = ctx.gp_fantasize(Xp, 2, seed=3, want_moments=True)
    Kp, Kpp = gp.ardse(Xp, X, h["lenscale_sq"], h["amp"]), gp.ardse(Xp, None, h["lenscale_sq"], h["amp"])
    ref, bar = R.cov_ref_bar(Kp, Kpp, Linv, R.npad(N))
    qc = _ratio(cov, ref, bar)
    assert qc <= 1.0, "%s: cov_out at %.3f of its derived bar" % (tag, qc)
    qm = _check_mean(mu[:, None], Kp, alpha, h, N, tag)
    sym = np.minimum(bar, bar.T)                  # B.3: the bar of check 2 itself (the smaller of its two entries), not their sum
    with np.errstate(divide="ignore", invalid="ignore"):
        qs = float(np.max(np.where(sym > 0, np.abs(cov - cov.T) / sym, np.where(cov == cov.T, 0.0, np.inf))))
    assert qs <= 1.0, "%s: |cov - cov'| at %.3f of the bar" % (tag, qs)
    try:
        ctx.gp_set_opts(var_with_noise=1)
        _, mu_n, cov_n = ctx.gp_fantasize(Xp, 2, seed=3, want_moments=True)
    finally:
        ctx.gp_set_opts()
    off = ~np.eye(P, dtype=bool)
    assert _bits(cov_n[off]) == _bits(cov[off]) and _bits(mu_n) == _bits(mu)
    assert _bits(np.diag(cov_n)) == _bits(np.diag(cov) + h["noise"])
    print("%s: cov %.4f, mean %.4f, asymmetry %.4f of the derived bars" % (tag, qc, qm, qs))


def test_fantasize_refusals_and_one_dimensional_pending_input(ctx):
    import bot7_amd
    X, Y = E.grid_data(20, 3, seed=20)
    h = R.grid_hyp(3)
    _fit(ctx, X, Y, h)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        ctx.gp_fantasize(R.grid_points(65, 3, seed=1), 4)
    assert e.value.code == -5                     # B7_ERR_UNSUPPORTED: more than 64 pending points
    one = R.grid_points(1, 3, seed=2)
    a = ctx.gp_fantasize(one[0], 9, seed=5, want_moments=True)
    b = ctx.gp_fantasize(one, 9, seed=5, want_moments=True)
    assert a[0].shape == (1, 9) and all(_bits(u) == _bits(v) for u, v in zip(a, b))
    _fit(ctx, X, np.hstack([Y, Y]), h)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        ctx.gp_fantasize(one, 4)
    assert e.value.code == -5                     # B7_ERR_UNSUPPORTED: the fit must have one response column
    ctx.gp_set_data(X, Y)                         # new data, no fit yet
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        ctx.gp_fantasize(one, 4)
    assert e.value.code == -4                     # B7_ERR_STATE: no GP fit on this context


# ---- C. fantasies: draws ----------------------------------------------------------------------------------------------------------
BIG_SEED = 2 ** 63 + 977


def _draw_problem(ctx, P, d=6, N=65):
    X, Y = E.grid_data(N, d, seed=N + P)
    h = R.grid_hyp(d, mean=0.25)
    assert _fit(ctx, X, Y, h)["jitter"] == 0
    return R.grid_points(P, d, seed=300 + P)


@pytest.mark.parametrize("seed", [7, BIG_SEED])
def test_one_pending_point_draws_are_mu_plus_sd_times_the_restated_normals(ctx, seed):
    """C.1: Y[0, s] within 8 ulp of mu + sqrt(cov00) Z[0, s]: 4 for z (DRAW_ULP), one each for sqrt, product and sum, rounded up;
    the ulp is that of the larger of the two terms and the result, since the sum may cancel."""
    Xp = _draw_problem(ctx, 1)
    n = 257
    Yd, mu, cov = ctx.gp_fantasize(Xp, n, seed=seed, want_moments=True)
    Z = R.fantasy_normals(seed, 1, n)
    term = math.sqrt(cov[0, 0]) * Z[0]
    want = mu[0] + term
    ulp = np.spacing(np.maximum(np.maximum(np.abs(want), np.abs(term)), abs(mu[0])))
    q = float(np.max(np.abs(Yd[0] - want) / ulp))
    cancel = ulp > np.spacing(np.abs(want))       # draws whose allowance is larger than 8 ulp of the restated value itself
    q_plain = float(np.max((np.abs(Yd[0] - want) / np.spacing(np.abs(want)))[~cancel])) if (~cancel).any() else 0.0
    print("P 1 seed %d: worst %.2f ulp; %d of %d draws cancel (ulp of the larger term), the other %d: worst %.2f ulp of the value"
          % (seed, q, int(cancel.sum()), n, int((~cancel).sum()), q_plain))
    assert q <= R.DRAW_ULP + 4


def _recovered(Yd, mu, cov, Z):
    """C.2's assertions; returns (L_est, Delta, j, schedule index or None)."""
    P = len(mu)
    L_est, delta, cond = R.recover_factor(Yd, mu, Z)
    assert cond < 4.0
    up = float(np.linalg.norm(np.triu(L_est, 1)))
    assert up <= delta, "strict upper triangle of the recovered factor %.3g > Delta %.3g" % (up, delta)
    G = L_est @ L_est.T
    j = float(np.mean(np.diag(G - cov)))
    step = R.match_schedule(j)
    jv = R.fantasy_schedule()[step] if step is not None else 0.0
    res = float(np.linalg.norm(G - (cov + jv * np.eye(P))))
    bar = R.NEAR_SINGULAR_FACTOR * float(np.linalg.norm(cov)) + 2 * float(np.linalg.norm(L_est)) * delta
    assert res <= bar, "||L L' - (cov + j I)|| %.3g > %.3g (j %.3g, step %s)" % (res, bar, j, step)
    return L_est, delta, j, step, up / delta, res / bar


@pytest.mark.parametrize("P", [2, 8, 64])
def test_the_factor_recovered_from_the_draws_is_lower_triangular_and_squares_to_the_covariance(ctx, P):
    """C.2: n = 4 P, a seed >= 2^63 (the binding masks it to 64 bits)."""
    Xp = _draw_problem(ctx, P)
    n = 4 * P
    Yd, mu, cov = ctx.gp_fantasize(Xp, n, seed=BIG_SEED, want_moments=True)
    _, delta, j, step, qu, qr = _recovered(Yd, mu, cov, R.fantasy_normals(BIG_SEED, P, n))
    assert step is None, "a well-conditioned covariance needs no jitter (j = %.3g)" % j
    print("P %d: upper triangle %.4f of Delta, residual %.4f of its bar" % (P, qu, qr))


def test_the_fantasy_jitter_loop_follows_the_schedule(ctx):
    """C.3: covariances that are singular in exact arithmetic (R.jitter_cases; the CPU test shows that LAPACK needs one schedule
    step on each).  The jitter recovered from the draws is a value of the schedule, and the verdict agrees with dpotrf's on
    cov_out unless its smallest pivot is within P eps ||cov_out|| of zero."""
    entered = 0
    for name, X, Y, h, Xp in R.jitter_cases():
        assert _fit(ctx, X, Y, h)["jitter"] == 0
        P = len(Xp)
        n = 4 * P
        Yd, mu, cov = ctx.gp_fantasize(Xp, n, seed=11, want_moments=True)
        _, delta, j, step, qu, qr = _recovered(Yd, mu, cov, R.fantasy_normals(11, P, n))
        S = np.tril(cov) + np.tril(cov, -1).T     # the factor reads the lower triangle
        info = lapack.dpotrf(S, lower=1, clean=1)[1]
        print("%s: jitter %.6g (schedule step %s), dpotrf info %d, min pivot %.3g" % (name, j, step, info, E.min_pivot(S)))
        if (info != 0) != (step is not None):
            assert abs(E.min_pivot(S)) <= P * E.EPS * float(np.linalg.norm(S)), (name, j, info)
        assert step is None or step < 20
        entered += step is not None
    assert entered, "neither case entered b7_gp_fantasize's jitter loop"


def test_the_draws_depend_on_n_through_the_counter_layout(ctx):
    """C.4: the same seed with n = 8 and n = 16 (P = 2): each call obeys its own k n + s restatement and gives the same factor;
    row 0 (counters s) is shared bit for bit, row 1 is not; the n = 8 draws do not fit the n = 16 layout."""
    Xp = _draw_problem(ctx, 2)
    got = {}
    for n in (8, 16):
        Yd, mu, cov = ctx.gp_fantasize(Xp, n, seed=21, want_moments=True)
        got[n] = (Yd, _recovered(Yd, mu, cov, R.fantasy_normals(21, 2, n)))
    (Y8, r8), (Y16, r16) = got[8], got[16]
    assert np.linalg.norm(r8[0] - r16[0]) <= r8[1] + r16[1]
    assert _bits(Y8[0]) == _bits(Y16[0, :8]) and not np.array_equal(Y8[1], Y16[1, :8])
    Lw, dw, _ = R.recover_factor(Y8, mu, R.fantasy_normals(21, 2, 16)[:, :8])      # row 1 solved against the wrong normals
    assert np.linalg.norm(Lw - r16[0]) > dw + r16[1]


def test_expected_improvement_with_pending_points_end_to_end(ctx, orc):
    """C.5: P = 2, nFantasies = 65, N = 63 (N + P = 65 crosses the 64 block): against the oracle scoring the same fantasies
    (rtol 1e-5: plumbing), and bit for bit the accumulator of the entry points called by hand."""
    import bot7_amd
    d, N, M, nF = 3, 63, 500, 65
    X, Y = E.grid_data(N, d, seed=63)
    Xh, Xp = R.grid_points(M, d, seed=64), R.grid_points(2, d, seed=65)
    h = R.grid_hyp(d, mean=0.1)
    model = bot7_amd.models.gp_regressor({"seed": 4}, context=ctx)
    model.hyp = h
    score = bot7_amd.scores.expected_improvement({"nFantasies": nF})
    got = score(model, h, X, Y, Xh, Xp)
    _fit(ctx, X, Y, h)
    Yp = ctx.gp_fantasize(Xp, nF, seed=4 * 1000003 + 1)
    X2, Y2 = np.concatenate([X, Xp]), np.concatenate([np.tile(Y, (1, nF)), Yp])
    ctx.grid_upload(Xh)
    _fit(ctx, X2, Y2, h)
    ctx.gp_predict(download=False)
    ctx.score_reset()
    ctx.score_ei(Y2.min(axis=0), 0.0)
    _, _, by_hand = ctx.score_finish(1.0, download=True)
    assert got.shape == (M,) and _bits(got) == _bits(by_hand)
    mu2, var2 = orc.gp.predict(orc.gp.fit(X2, Y2, **h), Xh)
    want = orc.c.ei(mu2, var2, Y2.min(axis=0))
    assert np.allclose(got, want, rtol=1e-5, atol=1e-9) and int(np.argmax(got)) == int(np.argmax(want))


# ---- D. append chains -------------------------------------------------------------------------------------------------------------
def _append_all(c, X, Y, n0, n1):
    """Appends rows n0 .. n1 - 1; returns the size reached (the first refusal, code -4, ends the chain)."""
    import bot7_amd
    assert n1 <= R.npad(n0), "the padding of a fit of %d rows ends at %d" % (n0, R.npad(n0))
    for n in range(n0, n1):
        try:
            c.gp_append(X[n], Y[n])
        except bot7_amd.Bot7HipError as e:
            assert e.code == -4, e
            return n
    return n1


def _check_chain_state(c, K, n0, n_dev, tag, k_gap=R.K_GAP):
    """D.1 at the size the device reached: its backward errors against 4 x the larger of LAPACK's and the restated chain's on the
    host's K (+ K_GAP for the factor: the 4 x and K_GAP of test_factors_at_the_corners...)."""
    L, _, Linv = c.gp_download(n_dev)
    assert np.isfinite(L).all() and np.isfinite(Linv).all(), tag
    Kn = K[:n_dev, :n_dev]
    yard, rs, la = R.chain_yardstick(K, n0, n_dev)
    g = E.backward_errors(Kn, L, Linv)
    print("%s n %d: device factor %.3g inverse %.3g | restated %s | LAPACK %s" % (tag, n_dev, g[0], g[1], rs, la))
    if yard is None:    # dpotrf fails and the restated chain stops short: no yardstick; the factor is held to NEAR_SINGULAR_FACTOR
        assert g[0] <= R.NEAR_SINGULAR_FACTOR + k_gap, (tag, g)
        return g[0] / (R.NEAR_SINGULAR_FACTOR + k_gap), float("nan")
    assert g[0] <= 4 * yard[0] + k_gap and g[1] <= 4 * yard[1], (tag, g, yard)
    return g[0] / (4 * yard[0] + k_gap), g[1] / (4 * yard[1])


def _check_verdicts(K, n0, n_dev, n1, tag):
    """D.3: where device and restatement disagree on refusing a step, the restated l2 lies within 2 x its own tol."""
    ch = R.append_chain(K, n0, n1)
    if ch is None:
        return
    n_ref = ch[2]
    if n_ref != n_dev:
        ch = R.append_chain(K, n0, min(n_ref, n_dev) + 1)      # the restated step at the first disagreement
        n, ok, l2, tol = ch[3][-1]
        assert n == min(n_ref, n_dev)
        print("%s: device stops at %d, restatement at %d; restated l2 %.3g tol %.3g" % (tag, n_dev, n_ref, l2, tol))
        assert abs(l2) <= 2 * tol, (tag, n_dev, n_ref, l2, tol)


# (257 -> 300, 1) at corner 2 is left out: K of the first 257 rows needs jitter there (the restatement, started from LAPACK's factor,
# refuses the very first append, n = 257: tests/test_pending_host.py), and a jittered factor is never extended.
CHAIN_CASES = [(n0, N, d, hyper) for n0, N, d in R.CHAINS for hyper in range(9) if (N, d, hyper) != (300, 1, 2)]


@pytest.mark.parametrize("n0,N,d,hyper", CHAIN_CASES)
def test_append_chains_have_lapack_sized_backward_errors(ctx, n0, N, d, hyper):
    """D.1 (+ D.3's verdict rule, + the refusal of the 65th row): hypers 0 .. 7 the covariance corners, 8 the interior point."""
    import bot7_amd
    X, Y = E.grid_data(N, d, seed=N)
    h = R.chain_hypers(X, Y)[hyper]
    tag = "(%d -> %d, %d) hyper %d" % (n0, N, d, hyper)
    rep = _fit(ctx, X[:n0], Y[:n0], h)
    assert rep["jitter"] == 0, "%s: the fit at n0 needs jitter %g" % (tag, rep["jitter"])
    K = R.host_K(X, h)
    n_dev = _append_all(ctx, X, Y, n0, N)
    _check_verdicts(K, n0, n_dev, N, tag)
    q = _check_chain_state(ctx, K, n0, n_dev, tag)
    if hyper in (0, 4, 5, 6, 7, 8) or (hyper == 2 and d > 1):     # every hyper but the near-singular corners 1, 3 and (d = 1) 2
        assert n_dev == N, "%s: a well-conditioned chain must run to the end" % tag
    print("%s: factor %.3f, inverse %.3f of the bars" % (tag, q[0], q[1]))
    if N == 64 and n_dev == N:      # the 64 padding is full
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            ctx.gp_append(X[0] + 0.5, Y[0])
        assert e.value.code == -4


def test_every_intermediate_state_of_a_chain(ctx):
    """D.2: 65 -> 128 at the interior hyper; after every append alpha against the device's own Linv (A.1) and mean / variance at
    129 grid candidates within E.gp_bar of LAPACK's error against a long-double refit (LAPACK on K and on K 1 -+ eps off the
    diagonal: the interior lenscale_sq is no power of 4)."""
    n0, N, d = 65, 128, 6
    X, Y = E.grid_data(N, d, seed=N)
    h = R.interior_hyp(d)
    Xs = R.grid_points(129, d, seed=9)
    K, Ks = R.host_K(X, h), gp.ardse(Xs, X, h["lenscale_sq"], h["amp"])
    ctx.grid_upload(Xs)
    assert _fit(ctx, X[:n0], Y[:n0], h)["jitter"] == 0
    worst = {}
    for n in range(n0, N):
        ctx.gp_append(X[n], Y[n])
        m = n + 1
        _, _, _, qa = _check_alpha(ctx, m, 1, Y[:m], h, "n %d" % m)
        worst["alpha"] = max(worst.get("alpha", 0.0), qa)
        mu, var = ctx.gp_predict()
        mu_t, var_t = R.ld_posterior(K[:m, :m], Ks[:, :m], Y[:m] - h["mean"], h["mean"], h["amp"])
        orcs = [E.lapack_fit(X[:m], Y[:m], h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xs, kscale=ks)
                for ks in (1.0, 1.0 - E.EPS, 1.0 + E.EPS)]
        for what, got, t, k, scale in (("mean", mu[:, 0], mu_t[:, 0], 1, math.sqrt(h["amp"])), ("var", var, var_t, 2, h["amp"])):
            e_g = float(np.max(np.abs(got.astype(LD) - t)))
            e_o = max(float(np.max(np.abs(o[k].astype(LD) - t))) for o in orcs)
            worst[what] = max(worst.get(what, 0.0), e_g / max(e_o, 16 * E.EPS * scale))
            assert e_g <= E.gp_bar(e_o, scale), (what, m, e_g, e_o)
    print("65 -> 128 every state: alpha %.4f of its bar; worst GPU / LAPACK error ratios mean %.3f var %.3f"
          % (worst["alpha"], worst["mean"], worst["var"]))


def _state(c, n, cols=1):
    return [_bits(a) for a in c.gp_download(n, cols)] + [_bits(a) for a in c.gp_predict()]


def _check_refused(c, X, Y, h, n, x_new, y_new):
    """D.3 after a refusal: -4, L / alpha / Linv and the posterior bit for bit as before, and the resident data still n rows."""
    import bot7_amd
    before = _state(c, n)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        c.gp_append(x_new, y_new)
    assert e.value.code == -4
    assert _state(c, n) == before
    again = c.gp_fit_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
    fresh = _fit(c, X[:n], Y[:n], h, want_nll=True)
    assert again["jitter"] == fresh["jitter"] and _bits(again["nll"]) == _bits(fresh["nll"])   # the NLL counts N: n rows, not n + 1


@pytest.mark.parametrize("corner", [2, 3])
def test_refusals_at_the_near_singular_corners(ctx, corner):
    """D.3 on (128, 1): the restatement refuses at n = 105 (corner 2) and 87 (corner 3), from n0 = 8 (the CPU test) and from
    n0 = 65 alike.  The device starts at 65: a fit of 8 rows has the 64 padding and cannot be extended past it."""
    n0 = 65
    X, Y = E.grid_data(128, 1, seed=128)
    h = R.chain_hypers(X, Y)[corner]
    ctx.grid_upload(R.grid_points(50, 1, seed=1))
    rep = _fit(ctx, X[:n0], Y[:n0], h)
    assert rep["jitter"] == 0
    K = R.host_K(X, h)
    n_dev = _append_all(ctx, X, Y, n0, 128)
    _check_verdicts(K, n0, n_dev, 128, "corner %d" % corner)
    _check_chain_state(ctx, K, n0, n_dev, "corner %d" % corner)
    assert n_dev < 128 or R.append_chain(K, n0)[2] < 128       # (the verdict rule above has judged a disagreement)
    if n_dev < 128:
        _check_refused(ctx, X, Y, h, n_dev, X[n_dev], Y[n_dev])


@pytest.mark.parametrize("noise", [0.0, 1e-8])
def test_near_duplicate_appends_are_accepted_cleanly_or_refused(ctx, noise):
    """D.3: a row at distance 2^-k (k in 10, 20, 26, 30) from observation 5 of 40."""
    X0, Y = E.grid_data(41, 2, seed=41)
    h = dict(R.grid_hyp(2, j=-2), noise=noise)
    ctx.grid_upload(R.grid_points(50, 2, seed=1))
    for k in (10, 20, 26, 30):
        X = X0.copy()
        X[40] = X[5]
        X[40, 0] += 2.0 ** -k
        tag = "noise %g k %d" % (noise, k)
        assert _fit(ctx, X[:40], Y[:40], h)["jitter"] == 0
        K = R.host_K(X, h)
        n_dev = _append_all(ctx, X, Y, 40, 41)
        _check_verdicts(K, 40, n_dev, 41, tag)
        if n_dev == 41:
            _check_chain_state(ctx, K, 40, 41, tag)
        else:
            _check_refused(ctx, X, Y, h, 40, X[40], Y[40])


def test_the_model_rebuilds_after_a_refused_append(ctx):
    """D.3: gp_regressor.fit takes the append by default; a refused one falls back to a full fit with the jitter schedule."""
    import bot7_amd
    X, Y = E.grid_data(41, 2, seed=41)
    X[40] = X[5]
    h = dict(R.grid_hyp(2, j=-2), noise=0.0)
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    model.hyp = h
    model.fit(X[:39], Y[:39])
    assert not model.last_fit.get("incremental") and model.last_fit["jitter"] == 0
    model.fit(X[:40], Y[:40])
    assert model.last_fit.get("incremental")
    model.fit(X, Y)                               # an exact duplicate under noise 0: refused, rebuilt (with jitter where K needs it)
    print("rebuilt after the refusal: %s" % model.last_fit)
    assert not model.last_fit.get("incremental") and model.last_fit["jitter"] >= 0
    if model.last_fit["jitter"] == 0:             # K is singular in exact arithmetic: a clean factor needs its smallest pivot at zero
        K = R.host_K(X, h)
        assert abs(E.min_pivot(K)) <= len(X) * E.EPS * float(np.linalg.norm(K)), E.min_pivot(K)
    else:
        assert model.last_fit["jitter"] in E.jitter_schedule(float(np.linalg.norm(R.host_K(X, h))))


def test_multi_column_append_and_the_resident_data(ctx):
    """D.4: c = 3, 100 -> 104: alpha (A.1) and mean (A.2) after the chain; then b7_gp_fit_hyp under the same hypers gives the
    factor of a fresh fit on all 104 rows bit for bit (ybuf and xobs have grown)."""
    X, Y = R.multi_data(104, 6, 3, seed=104)
    h = R.grid_hyp(6, mean=0.25)
    Xs = R.grid_points(129, 6, seed=5)
    ctx.grid_upload(Xs)
    assert _fit(ctx, X[:100], Y[:100], h)["jitter"] == 0
    assert _append_all(ctx, X, Y, 100, 104) == 104
    _, alpha, _, qa = _check_alpha(ctx, 104, 3, Y, h, "c 3 append")
    mu, _ = ctx.gp_predict()
    qm = _check_mean(mu, gp.ardse(Xs, X, h["lenscale_sq"], h["amp"]), alpha, h, 104, "c 3 append")
    again = ctx.gp_fit_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
    refit = [_bits(a) for a in ctx.gp_download(104, 3)]
    fresh = _fit(ctx, X, Y, h, want_nll=True)
    assert refit == [_bits(a) for a in ctx.gp_download(104, 3)] and _bits(again["nll"]) == _bits(fresh["nll"])
    print("c 3, 100 -> 104: alpha %.4f, mean %.4f of the derived bars" % (qa, qm))


def test_append_chain_under_the_matern_kernel(ctx):
    """D.5: 65 -> 80, d = 6, lenscale_sq 1; K_GAP is replaced by the Matern kernel's own distance to the host's K."""
    X, Y = E.grid_data(80, 6, seed=80)
    h = R.grid_hyp(6, j=0)
    ctx.gp_set_kernel("ardmatern52")
    try:
        assert _fit(ctx, X[:65], Y[:65], h)["jitter"] == 0
        K = R.host_K(X, h, "ardmatern52")
        gap = float(np.linalg.norm(K * R.matern_gap(X, None, h["lenscale_sq"])) / np.linalg.norm(K))
        assert _append_all(ctx, X, Y, 65, 80) == 80
        q = _check_chain_state(ctx, K, 65, 80, "matern 65 -> 80", k_gap=gap)
    finally:
        ctx.gp_set_kernel("ardse")
    print("matern 65 -> 80: factor %.3f, inverse %.3f of the bars" % q)
