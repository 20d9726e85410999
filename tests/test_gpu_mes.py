"""Max-value entropy search (B7_SCORE_MES) on the device: the score against 50-digit arithmetic, the y* search against bisection
to adjacent doubles, every route of b7_eval_nominate against the per-sample loop bit for bit and against the reference end to
end, the refusals, and the trial loop (references: tests/_mes_ref.py).

Bars.  Score values: |err| <= 1e-13 max(1, |ref|), the project's bar for a score through ocml.  y*: |y* - ref| <= (RESOLUTION +
ALLOWANCE) (hi0 - lo0), RESOLUTION = (1/2) 16^-10 = 4.5e-13 the half width of the last bracket (derived), ALLOWANCE the rounding
allowance below.  Accumulator end to end: 1e-12 max(1, |ref|) = |d score / d y*| (<= 0.6 on the checked distributions) times the
y* bar, plus the score bar.  Each test prints its achieved figure."""
import functools

import mpmath
import numpy as np
import pytest

import bot7_amd
from conftest import make_network, make_problem
from harness import benchmarks as B
from harness import bots

import _mes_ref as R

pytestmark = pytest.mark.gpu

# The y* bar's rounding allowance: 8 x the worst deviation beyond RESOLUTION seen against ystar_ref on the first MI355X run, over
# the 84 bisection-checked cases of test_ystar_against_bisection.  That run: worst |y* - ref| = 4.54903e-13 (hi0 - lo0) (u1, M = 5,
# K = 1: a root at the very edge of its last bracket), RESOLUTION = 4.54747e-13, so the worst excess is 1.56e-16 (hi0 - lo0) -- one
# rounding of the bracket's end points -- and 82 of the 84 cases show none.  8 x 1.56e-16 = 1.25e-15, far below the 1e-9 at which
# it would be a defect of the reduction rather than a tolerance.
MEASURED_WORST_EXCESS = 1.56e-16
ALLOWANCE = 8 * MEASURED_WORST_EXCESS


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


@pytest.fixture(autouse=True)
def _default_levels(ctx):
    ctx.mes_set_levels(8)
    yield
    ctx.mes_set_levels(8)


# ---- 1. h values -------------------------------------------------------------------------------------------------------------
def _swept(rng, n, ystar, glo=-8.0, ghi=40.0, slo=1e-3):
    """n rows whose g = (mu - ystar)/sigma covers [glo, ghi] (a sixth packed around the branch points 0 and -1), sigma log-uniform
    in [slo, 10]; rows whose ROUNDED g leaves the interval are pulled back in."""
    g = np.concatenate([rng.uniform(glo, ghi, n - 2 * (n // 12)), rng.normal(scale=0.02, size=n // 12),
                        -1.0 + rng.normal(scale=0.02, size=n // 12)])
    g[:4] = [glo, ghi, 0.0, -1.0]
    sigma = np.exp(rng.uniform(np.log(slo), np.log(10.0), n))
    mu = ystar + g * sigma
    var = sigma * sigma
    got_g = (mu - ystar) / np.sqrt(var)
    fix = (got_g < glo) | (got_g > ghi)
    mu[fix] = ystar + 0.5 * np.sqrt(var[fix])
    return mu, var


def test_h_values_against_50_digits(ctx):
    """b7_mes_compute, M = 4096, K = 1, g = (mu - y*)/sigma over [-8, 40] through mu, sigma (log-uniform in [1e-3, 10]) and y* (-1.7,
    then 250): against h in 50 digits on the exact inputs, bar 1e-13 max(1, |ref|).  Finite on g in [-1e6, -8).  Then K = 3 against
    the mean of the three.  Measured on an MI355X: K = 1 worst 4.3e-15 (at g = -7.2), K = 3 worst 1.9e-15."""
    rng = np.random.default_rng(4096)
    for ystar in (-1.7, 250.0):
        mu, var = _swept(rng, 4096, ystar)
        g = (mu - ystar) / np.sqrt(var)
        assert g.min() >= -8.0 and g.max() <= 40.0 and g.min() < -7.9 and g.max() > 39.9
        got = ctx.mes_compute(mu, var, [ystar])
        err = R.scaled_errors(got, R.mes_ref(mu, var, [ystar]))
        print("MES h, y* = %g: worst scaled error %.3g at g = %.6g" % (ystar, err.max(), g[err.argmax()]))
        assert np.isfinite(got).all() and (got >= 0).all()
        assert err.max() <= R.BAR, "%.3g at g = %g" % (err.max(), g[err.argmax()])
    t = np.exp(rng.uniform(np.log(8.0), np.log(1e6), 1024))
    far = ctx.mes_compute(-t, np.ones(t.size), [0.0])
    assert np.isfinite(far).all()
    ys = [-2.0, -1.7, -1.1]        # sigma >= 0.5 keeps all three g of a row within 1.2 of each other, inside [-8, 40]
    mu, var = _swept(rng, 1024, -1.7, -6.0, 38.0, slo=0.5)
    g3 = (mu[:, None] - np.array(ys)[None, :]) / np.sqrt(var)[:, None]
    assert g3.min() >= -8.0 and g3.max() <= 40.0
    got = ctx.mes_compute(mu, var, ys)
    err = R.scaled_errors(got, R.mes_ref(mu, var, ys))
    print("MES h, K = 3: worst scaled error %.3g" % err.max())
    assert err.max() <= R.BAR


# ---- 2. row classes ------------------------------------------------------------------------------------------------------------
def test_row_classes(ctx):
    """var in {0, -1, NaN} and mu NaN: bad rows score NaN, exact rows score exactly 0.0, live rows score what they score without
    them.  The search skips both classes: lo0 / hi0 are the clean vector's bits.  y* is NOT expected to be the clean vector's bits:
    a row's block and thread follow its POSITION (row j belongs to block j / 256 mod nb), so interleaved rows move the live ones
    between partial sums and the roundings differ; it is held to the bisection reference on the clean vector within the y* bar."""
    nan = np.nan
    mu0, var0 = R.distribution("u1", 1000)
    at = [0, 3, 3, 257, 500, 999, 1000]
    mu = np.insert(mu0, at, [0.5, nan, nan, -9.0, 0.0, nan, -50.0])
    var = np.insert(var0, at, [0.0, 1.0, 0.0, -1.0, nan, nan, 0.0])
    ys = R.ystar_ref(mu0, var0, 8)
    got, clean = ctx.mes_compute(mu, var, ys), ctx.mes_compute(mu0, var0, ys)
    bad, exact, live = R.classes(mu, var)
    assert bad.sum() == 5 and exact.sum() == 2 and live.sum() == 1000
    assert np.isnan(got[bad]).all() and (got[exact] == 0.0).all() and not np.signbit(got[exact]).any()
    assert _bits(got[live]) == _bits(clean)
    lo0, hi0 = R.bracket(mu0, var0)
    y1, b1 = ctx.mes_ystar(mu, var, 8)
    y0, b0 = ctx.mes_ystar(mu0, var0, 8)
    assert _bits(b1) == _bits([lo0, hi0]) == _bits(b0)
    bar = R.ystar_bar(lo0, hi0, ALLOWANCE)
    print("MES row classes: |y* - ref| worst %.3g (interleaved), %.3g (clean), bar %.3g" % (np.abs(y1 - ys).max(), np.abs(y0 - ys).max(), bar))
    assert np.abs(y1 - ys).max() <= bar and np.abs(y0 - ys).max() <= bar
    # b7_mes_compute keeps the caller's y* apart: the last search's values are still there afterwards
    ctx.mes_compute(mu0, var0, [0.25, 0.5])
    yl, bl = ctx.mes_last_ystar()
    assert yl.shape == (1, 8) and _bits(yl[0]) == _bits(y0) and _bits(bl[0]) == _bits(b0)
    # no live row at all: nothing to search, every y* and the bracket are NaN
    yn, bn = ctx.mes_ystar([0.0, nan, 1.0], [0.0, 1.0, -2.0], 3)
    assert np.isnan(yn).all() and np.isnan(bn).all()


# ---- 3. y* against bisection ---------------------------------------------------------------------------------------------------
DISTS = ("u1", "u2", "u3", "one", "same", "wide")


@functools.lru_cache(maxsize=None)
def _ref(name, M, K):
    mu, var = R.distribution(name, M)
    return R.ystar_ref(mu, var, K)


def _straddles(y, mu, var, K, levels, bar):
    """|y*_k - root_k| <= bar without finding the root: L is non-increasing, so the root of L = t_k lies within bar of y*_k exactly
    when L(y*_k - bar) > t_k >= L(y*_k + bar) -- two sums per level where bisection to adjacent doubles takes fifty-six."""
    t = R.targets(K)
    return all(R.log_survival(y[k] - bar, mu, var) > t[k] >= R.log_survival(y[k] + bar, mu, var) for k in levels)


@pytest.mark.parametrize("name", DISTS)
def test_ystar_against_bisection(ctx, name):
    """b7_mes_ystar on three draws of the distribution the search was prototyped on (mu ~ U(-2, 2), sigma log-uniform in [1e-3, 1],
    default_rng(1..3)) and three boundary shapes (one sharp row far below the rest; every row alike; a bracket 2e3 wide with sigma
    over eight decades): M in {5, 257, 1000, 4096, 20000} (one thread's worth, an odd block and a bit, several blocks, a multiple of
    the block, many blocks), K in {1, 8} everywhere and K = 64 up to M = 4096, against bisection to adjacent doubles.  lo0 / hi0
    equal the reference's bit for bit.  Bar (RESOLUTION + ALLOWANCE) (hi0 - lo0).  K = 64 at M = 20000: the same bar through the
    straddle form (bisection of 64 levels over 2e4 rows takes 8 s on the host).
    Measured on an MI355X: worst 4.549e-13 (hi0 - lo0), 1.56e-16 beyond the resolution term (top of the file)."""
    worst = 0.0
    for M in (5, 257, 1000, 4096, 20000):
        mu, var = R.distribution(name, M)
        lo0, hi0 = R.bracket(mu, var)
        for K in (1, 8, 64):
            y, b = ctx.mes_ystar(mu, var, K)
            assert _bits(b) == _bits([lo0, hi0]), (name, M, K)
            assert (np.diff(y) >= 0).all() and lo0 < y[0] and y[-1] < hi0
            bar = R.ystar_bar(lo0, hi0, ALLOWANCE)
            if K == 64 and M > 4096:
                assert _straddles(y, mu, var, K, range(K), bar), (name, M, K)
                continue
            dev = np.abs(y - _ref(name, M, K)).max() / (hi0 - lo0)
            worst = max(worst, dev)
            assert dev * (hi0 - lo0) <= bar, "%s M %d K %d: %.3g (hi0 - lo0), bar %.3g" % (name, M, K, dev, bar / (hi0 - lo0))
    print("MES y* %s: worst |y* - ref| = %.4g (hi0 - lo0); resolution term %.4g, excess %.3g"
          % (name, worst, R.RESOLUTION, max(0.0, worst - R.RESOLUTION)))


@pytest.mark.parametrize("K", (1, 8, 64))
@pytest.mark.parametrize("name", DISTS)
def test_ystar_past_one_pass_of_the_grid(ctx, name, K):
    """M = 600 001 rows: more than cus x 8 x 256, so the blocks go round the grid-stride loop and a thread's sum has several
    passes -- all six distributions ('same' makes every one of the 6e5 terms alike, 'wide' spreads them over eight decades: the two
    ends of what a long sum's rounding can meet), K in {1, 8, 64}, EVERY level within the bar of the root.  The bar is test 3's,
    in the straddle form L(y* - bar) > t_k >= L(y* + bar) with the reference's own L (math.fsum of log_ndtr): two sums per level,
    where bisection to adjacent doubles over 6e5 rows is 3 s a level on the host.  lo0 / hi0 bit for bit; the same call twice
    gives the same bits."""
    import math
    from scipy import special
    M = 600001
    mu, var = R.distribution(name, M)
    lo0, hi0 = R.bracket(mu, var)
    bar = R.ystar_bar(lo0, hi0, ALLOWANCE)
    y, b = ctx.mes_ystar(mu, var, K)
    assert _bits(b) == _bits([lo0, hi0])
    assert (np.diff(y) >= 0).all() and lo0 < y[0] and y[-1] < hi0
    # R.log_survival's sum over fewer rows: every row of these distributions is live, and a row whose term is exactly 0.0 at the
    # highest point evaluated is exactly 0.0 at every point below it (log Phi is monotone and <= 0): the same sums
    sigma = np.sqrt(var)
    keep = special.log_ndtr((mu - (y[-1] + bar)) / sigma) != 0.0
    mk, sk = mu[keep], sigma[keep]

    def L(at):
        return math.fsum(special.log_ndtr((mk - at) / sk))
    assert L(y[0]) == R.log_survival(y[0], mu, var)
    t = R.targets(K)
    for k in range(K):
        assert L(y[k] - bar) > t[k] >= L(y[k] + bar), (name, K, k)
    if K == 8:
        y2, _ = ctx.mes_ystar(mu, var, K)
        assert _bits(y2) == _bits(y)


# ---- 4. determinism and routes ---------------------------------------------------------------------------------------------------
def _objective(X):
    return np.sin(3.0 * X).sum(axis=1, keepdims=True)


def _hyps(hyp, S):
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.25 * s), amp=hyp["amp"] * (1.0 + 0.1 * s)) for s in range(S)]


def _loop(c, X_obs, Y, hyps):
    """{b7_gp_predict_hyp; b7_score_mes} x S + b7_score_finish(S) -> value, index, scores, y* [S][K], [(mean, var)] per sample"""
    c.gp_set_data(X_obs, Y)
    mv, ys = [], []
    for s, h in enumerate(hyps):
        out = c.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], download=True)
        mv.append((out["mean"][:, 0].copy(), out["var"].copy()))
        if s == 0:
            c.score_reset()
        c.score_mes()
        y, _ = c.mes_last_ystar()
        assert y.shape == (1, 8)
        ys.append(y[0])
    val, idx, scores = c.score_finish(float(len(hyps)), download=True)
    return val, idx, scores, np.array(ys), mv


# (N, d, M, S), workspace bytes (None: the default), launches expected in the phases (mes, score, argmax)
ROUTES = {
    "small": ((20, 3, 1000, 3), None, (11, 1, 0)),        # one-launch fit + kpost_small; the fused score / arg-max kernel
    "batched": ((200, 6, 2049, 3), None, (11, 1, 1)),     # ksx / post of all samples at once; score_batch_kernel
    "per_sample": ((200, 6, 2049, 3), 8 << 20, (33, 3, 1)),  # K* of three samples does not fit 8 MiB: predict_into per sample
    "one_sample": ((200, 6, 2049, 1), None, (11, 1, 1)),  # S = 1: the non-batch fit loop
}


_RUNS = {}


def _nominate(ctx, orc, route):
    """The route's nomination twice, then the per-sample loop: everything the route tests compare, computed once per route."""
    if route not in _RUNS:
        _RUNS[route] = _nominate_once(ctx, orc, route)
    return _RUNS[route]


def _nominate_once(ctx, orc, route):
    (N, d, M, S), workspace, launches = ROUTES[route]
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, d, N, M, _objective)
    hyps = _hyps(hyp, S)
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    if workspace:
        ctx.set_workspace(workspace)
    try:
        runs = []
        for rep in range(2):
            ctx.profile_enable(True)
            try:
                ctx.profile_reset()
                val, idx, report = ctx.eval_nominate(hyps, score="mes", want_report=True)
                counts = tuple(ctx.profile_get(ph)[1] for ph in ("mes", "score", "argmax"))
            finally:
                ctx.profile_enable(False)
            _, _, acc = ctx.score_finish(1.0, download=True)
            ystar, brackets = ctx.mes_last_ystar()
            runs.append((val, idx, acc, ystar, brackets, counts, report))
    finally:
        if workspace:
            ctx.set_workspace(4 << 30)
    return runs, _loop(ctx, X_obs, Y, hyps), launches


@pytest.mark.parametrize("route", list(ROUTES))
def test_eval_nominate_is_deterministic_and_is_the_per_sample_loop_bit_for_bit(ctx, orc, route):
    """b7_eval_nominate(B7_SCORE_MES) twice: the same best_val, index, accumulator and y* bits.  And against {b7_gp_predict_hyp;
    b7_score_mes} x S + b7_score_finish(S): equal winner, value, accumulator and y* (b7_mes_last_ystar), bit for bit, on the small
    fused route, the batched route, the per-sample branch (a workspace too small for three K*) and S = 1; the phase counters say
    which route ran (a search is 11 launches: one for the bracket, ten rounds)."""
    (a, b), (val0, idx0, sc0, ys0, mv), launches = _nominate(ctx, orc, route)
    assert a[5] == launches and b[5] == launches, (a[5], launches)
    assert not a[6]["jitter"].any() and not a[6]["info"].any()
    assert (a[1], _bits([a[0]]), _bits(a[2]), _bits(a[3]), _bits(a[4])) == (b[1], _bits([b[0]]), _bits(b[2]), _bits(b[3]), _bits(b[4]))
    assert a[3].shape == ys0.shape == (len(mv), 8)
    assert a[1] == idx0 and _bits([a[0]]) == _bits([val0]) and _bits(a[2]) == _bits(sc0) and _bits(a[3]) == _bits(ys0)
    assert _bits([a[0]]) == _bits([a[2][a[1] - 1]])
    for s, (m, v) in enumerate(mv):
        assert _bits(a[4][s]) == _bits(R.bracket(m, v))


# ---- 5. end to end against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_nomination_against_the_reference(ctx, orc, route):
    """From each sample's downloaded mean and variance: y* by bisection, the scores in 50 digits, the marginal and the nominee by
    the reference's own rule.  The device's y* within the y* bar, its accumulator within 1e-12 max(1, |ref|), its nominee the
    reference's -- on inputs whose reference top-2 gap is at least 1e6 x the measured score error (asserted, not assumed).
    Measured on an MI355X: accumulator worst 3e-15, gaps 1e-3 and up."""
    (a, _), (_, _, _, _, mv), _ = _nominate(ctx, orc, route)
    val, idx, acc, ystar = a[0], a[1], a[2], a[3]
    cols = []
    for s, (m, v) in enumerate(mv):
        ys = R.ystar_ref(m, v, 8)
        lo0, hi0 = R.bracket(m, v)
        assert np.abs(ystar[s] - ys).max() <= R.ystar_bar(lo0, hi0, ALLOWANCE)
        cols.append(R.mes_ref(m, v, ys))
    ref = R.mean_mp(cols)
    err = R.scaled_errors(acc, ref)
    gap = R.top2_gap(ref)
    print("MES end to end, %s: accumulator worst scaled error %.3g, reference top-2 gap %.3g" % (route, err.max(), gap))
    assert err.max() <= 1e-12
    assert gap >= 1e6 * err.max(), "the inputs do not decide the winner: gap %.3g, error %.3g" % (gap, err.max())
    assert idx == R.nominee(ref) + 1
    assert abs(val - float(ref[idx - 1])) <= 1e-12 * max(1.0, abs(float(ref[idx - 1])))


# ---- 6. the jitter redo -----------------------------------------------------------------------------------------------------------
def test_jitter_redo_keeps_the_loops_winner(ctx, orc):
    """Duplicated observations, zero noise: the plain factorisation fails and the nomination is redone through the jitter schedule;
    under MES it returns what the per-sample loop returns, bit for bit, y* included."""
    X = orc.c.sobol(40, 3, 1)
    X[7] = X[3]
    Y = _objective(X)
    X_hid = orc.c.sobol(2048, 3, 100)
    good = dict(lenscale_sq=np.full(3, 0.4), amp=1.0, noise=1e-3, mean=0.1)
    hyps = [good, dict(good, noise=0.0, mean=0.0), dict(good, amp=1.3)]
    ctx.grid_upload(X_hid)
    val0, idx0, sc0, ys0, _ = _loop(ctx, X, Y, hyps)
    ctx.gp_set_data(X, Y)
    val1, idx1, rep = ctx.eval_nominate(hyps, score="mes", want_report=True)
    _, _, sc1 = ctx.score_finish(1.0, download=True)
    ys1, _ = ctx.mes_last_ystar()
    assert rep["info"][1] > 0 and rep["jitter"][1] != 0
    assert idx1 == idx0 and _bits([val1]) == _bits([val0]) and _bits(sc1) == _bits(sc0) and _bits(ys1) == _bits(ys0)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *args, **kw):
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_refusals_leave_the_context_usable(ctx, orc):
    """Every route MES is not built on answers B7_ERR_UNSUPPORTED (-5) with a message naming the case -- the group call, both BLR
    nominations, the batch nomination, more than one response column (nomination and b7_score_mes) -- and K = 0 / K = 65 answer
    B7_ERR_INVALID (-1).  (A communicator of more than one rank: test_world_of_two_is_refused, one process per rank.)  Afterwards
    an EI nomination gives the bits it gave before, and the manual DNGO path
    b7_blr_predict + b7_score_mes works."""
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, 3, 24, 1000, _objective)
    hyps, fmin = _hyps(hyp, 2), [float(Y.min())]
    ctx.grid_upload(X_hid)
    ctx.gp_set_data(X_obs, Y)
    before = ctx.eval_nominate(hyps, score="ei", fmin=fmin) + (ctx.score_finish(1.0, download=True)[2],)
    assert "batch" in _refused(-5, ctx.eval_nominate_batch, hyps, 2, score="mes")
    W, b = make_network(3, (16, 16), seed=11)
    be = 1.0 / (1e-2 * float(np.var(Y)))
    assert "blr_eval_nominate" in _refused(-5, ctx.blr_eval_nominate, W, b, "Tanh", X_obs, Y, 1.0, be, 0.0, score="mes")
    assert "blr_eval_nominate_marg" in _refused(-5, ctx.blr_eval_nominate_marg, W, b, "Tanh", X_obs, Y, [1.0, 2.0], [be, be], [0.0, 0.0], score="mes")
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(X_hid)
        g.gp_set_data(X_obs, Y)
        assert "sharded" in _refused(-5, g.eval_nominate, hyps, score="mes")
    finally:
        g.close()
    Y2 = np.concatenate([Y, Y + 0.5], axis=1)
    ctx.gp_set_data(X_obs, Y2)
    assert "response columns" in _refused(-5, ctx.eval_nominate, hyps, score="mes")
    ctx.gp_predict_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
    ctx.score_reset()
    assert "response columns" in _refused(-5, ctx.score_mes)
    for K in (0, 65):
        _refused(-1, ctx.mes_set_levels, K)
        _refused(-1, ctx.mes_ystar, [0.0, 1.0], [1.0, 1.0], K)
    _refused(-1, ctx.mes_compute, [0.0], [1.0], np.zeros(65))
    _refused(-1, ctx.mes_compute, [0.0], [1.0], np.zeros(0))
    ctx.gp_set_data(X_obs, Y)
    after = ctx.eval_nominate(hyps, score="ei", fmin=fmin) + (ctx.score_finish(1.0, download=True)[2],)
    assert after[1] == before[1] and _bits([after[0]]) == _bits([before[0]]) and _bits(after[2]) == _bits(before[2])
    # the manual DNGO path: the head's posterior scored by MES, against the reference on the downloaded mean / variance
    ctx.blr_fit_x(W, b, "Tanh", X_obs, Y, 1.0, be, float(np.mean(Y)))
    ctx.blr_basis(W, b, "Tanh")
    mu, var = ctx.blr_predict()
    ctx.score_reset()
    ctx.score_mes()
    val, idx, sc = ctx.score_finish(1.0, download=True)
    ys = R.ystar_ref(mu[:, 0], var, 8)
    err = R.scaled_errors(sc[::8], R.mes_ref(mu[::8, 0], var[::8], ys))
    print("MES on the DNGO head: worst scaled error %.3g" % err.max())
    assert err.max() <= 1e-12 and val == sc[idx - 1] == sc.max()


# ---- 8. the trial loop ------------------------------------------------------------------------------------------------------------------
def test_trial_loop_runs_on_max_value_entropy_search(ctx, orc):
    class H(object):
        def __init__(self, name):
            self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1

    cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 3, "nSamples": 2, "seed": 2},
           "grid": {"type": "sobol", "size": 512, "dims": 6}, "score": {"type": "max_value_entropy_search"},
           "model": {"type": "gp_regressor", "sample": True, "nBurnin": 2, "seed": 5}}
    bot = bots.bayesopt(B.hartmann6, [H("x%d" % k) for k in range(6)], cfg)
    assert type(bot.score) is bot7_amd.scores.max_value_entropy_search
    bot.model._ctx = ctx
    bot.candidates = bot7_amd.grids.sobol(bot.config["grid"], context=ctx)()
    grid0 = np.asarray(bot.candidates).copy()
    inner, seen = bot.eval, []

    def recording_eval(candidates=None, want_scores=True):   # every model-based trial's scores, not only the winner
        scores, val, idx = inner(candidates, True)
        seen.append((scores, val, idx))
        return scores, val, idx
    bot.eval = recording_eval
    bot.run_experiment()
    obs = np.asarray(bot.observed)
    assert obs.shape == (12, 6) and np.asarray(bot.candidates).shape == (500, 6)
    rows = {r.tobytes() for r in grid0}
    assert len({r.tobytes() for r in obs}) == 12 and all(r.tobytes() in rows for r in obs)
    assert len(seen) == 12 - 3                                   # the trials after the three random ones
    for t, (scores, val, idx) in enumerate(seen):
        assert scores.shape == (512 - 3 - t,) and np.isfinite(scores).all(), t
        assert val == scores[idx - 1] == scores.max()
    scores, val, idx = bot.eval()
    assert scores.shape == (500,) and np.isfinite(scores).all()
    assert val == scores[idx - 1] == scores.max()


# ---- 9. a communicator of two ranks ------------------------------------------------------------------------------------------------------
def world_problem():
    """(X_obs, Y, candidates, hyps) of the two-rank refusal test and its workers (tests/_mes_worker.py)."""
    rng = np.random.default_rng(17)
    X, Xc = rng.random((24, 3)), rng.random((1000, 3))
    Y = _objective(X)
    amp = float(np.var(Y))
    hyp = {"lenscale_sq": np.full(3, 3 / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(Y))}
    return X, Y, Xc, _hyps(hyp, 2)


def test_world_of_two_is_refused(ctx, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub), each with its shard: b7_eval_nominate(B7_SCORE_MES)
    and b7_score_mes answer B7_ERR_UNSUPPORTED on both with a message naming the communicator -- without a collective: a rank that
    issued one would wait for a peer that has already returned, and the workers would not finish --, and the EI nomination that
    follows gives the single-context nomination of the union."""
    import json
    import os
    import subprocess
    import sys
    from test_sharded_loop import _diag_lib, _stub_lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=root)
    ident = ("b7mes_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(root, "tests", "_mes_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, Y, Xc, hyps = world_problem()
    ctx.grid_upload(Xc)
    ctx.gp_set_data(X, Y)
    want = ctx.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
    for o in outs:
        with open(o) as f:
            res = json.load(f)
        assert res["codes"] == [-5, -5], res
        assert all("communicator of 2 ranks" in m for m in res["messages"]), res["messages"]
        assert (res["value"], res["index"]) == want
