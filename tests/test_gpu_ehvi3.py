"""b7_ehvi3_compute / b7_ehvi3_nominate on the GPU: three-objective nomination by the exact expected hypervolume improvement over a
box decomposition of the non-dominated region.

The two kernels are measured against the marginal at 50 digits (tests/_ehvi3_ref.ehvi3_mp, which cuts the region into slabs and
strips of its own, not into the library's boxes) with the project's bar, tests/_exact.gp_bar: per row 8 x the error of the float64
restatement (ehvi3_numpy) against the same 50 digits + 16 eps x the row's scale, the EHVI against an empty front
T1(r1) T2(r2) T3(r3) at 50 digits, which bounds every EHVI of the row.  The accumulator and the nominee are compared bit for bit with
the calls they restate.  Every test prints its achieved figure.  The build chunks the candidates (the table of a chunk stays within
min(workspace, 256 MiB)), so the chunking test runs."""
import numpy as np
import pytest

import _ehvi3_ref as R
import _ehvi_ref as R2
import _exact as E

pytestmark = pytest.mark.gpu


def bar_ratio(got, mu, var, front, ref):
    """Row classes exactly; the worst |got - 50 digits| / bar over the rows, bar = gp_bar(ehvi3_numpy's error, scale) per row (a bar
    of 0 -- the restatement exact and the scale 0 -- admits an error of 0 alone)."""
    hi, lo, scale = R.ehvi3_mp(mu, var, front, ref)
    assert np.array_equal(np.isnan(got), np.isnan(hi)), "row classes differ"
    ok = ~np.isnan(hi)
    assert np.isfinite(got[ok]).all() and (got[ok] >= 0.0).all()
    err_np = R.err_vs_mp(R.ehvi3_numpy(mu, var, front, ref), hi, lo)[ok]
    bar = E.gp_bar(err_np, scale[ok])
    err = R.err_vs_mp(got, hi, lo)[ok]
    assert (err[bar == 0.0] == 0.0).all()
    live = bar > 0.0
    return float((err[live] / bar[live]).max()) if live.any() else 0.0


def chunks_of(c, fn):
    """(fn's result, how many chunks the call walked: launches of the table kernel)."""
    c.profile_enable(True)
    try:
        c.profile_reset()
        out = fn()
        n = c.profile_get("ehvi3_tab")[1]
    finally:
        c.profile_enable(False)
    return out, n


# ---- 1. the kernels against 50 digits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,S1,S2,S3", R.KERNEL_CASES3)
def test_kernel_against_50_digits(ctx, M, P, S1, S2, S3):
    """b7_ehvi3_compute on synthetic posteriors (_ehvi3_ref.make_rows3: mu from far below the front to far beyond ref, z down to -40
    and past the point where float64 gives 0; sigma 1e-8 .. 1e2 of the front's extent; var == 0 in one sample and in all; the NaN
    and var < 0 classes in each objective) against fronts on a tilted plane with two points one ulp apart in the first objective,
    two sharing a first and two sharing a third coordinate.  M = 1000 ends inside a workgroup of either kernel; P = 33 and 256 end
    inside a block of eight cuts.  Bar: module docstring.  On an MI355X the worst ratio to the bar over the seven cases is 0.27
    (M = 1000)."""
    mu, var = R.make_rows3(M, (S1, S2, S3))
    front = R.make_front3(P)
    got = ctx.ehvi3_compute(mu, var, front, R.REF3)
    assert got.shape == (M,)
    worst = bar_ratio(got, mu, var, front, R.REF3)
    print("ehvi3 kernels M=%d P=%d S=(%d, %d, %d): worst error / bar %.3g" % (M, P, S1, S2, S3, worst))
    assert worst <= 1.0
    assert ctx.ehvi3_compute(mu, var, front, R.REF3).tobytes() == got.tobytes()      # the same call twice: the same bits
    if M >= 128:    # a row's value does not depend on where in the launch it sits
        part = ctx.ehvi3_compute([m[:, 37:101] for m in mu], [v[:, 37:101] for v in var], front, R.REF3)
        assert part.tobytes() == got[37:101].tobytes()


def test_chunking_does_not_change_a_bit(ctx):
    """M = 1000, P = 33 (105 table rows: 852 bytes per candidate): one chunk under the default workspace, eight under the smallest
    one b7_set_workspace takes (128 KiB: 128 candidates per chunk); the rows' bits are the same."""
    mu, var = R.make_rows3(1000, (3, 2, 2), seed=1)
    front = R.make_front3(33)
    whole, n1 = chunks_of(ctx, lambda: ctx.ehvi3_compute(mu, var, front, R.REF3))
    try:
        ctx.set_workspace(128 << 10)
        cut, n8 = chunks_of(ctx, lambda: ctx.ehvi3_compute(mu, var, front, R.REF3))
    finally:
        ctx.set_workspace(4 << 30)
    print("ehvi3 chunking: %d chunk(s) by default, %d under a 128 KiB workspace" % (n1, n8))
    assert n1 == 1 and n8 >= 3 and cut.tobytes() == whole.tobytes()
    assert bar_ratio(whole[::25], [m[:, ::25] for m in mu], [v[:, ::25] for v in var], front, R.REF3) <= 1.0


def test_compute_refusals(ctx):
    mu, var = [np.zeros((1, 4))] * 3, [np.ones((1, 4))] * 3
    ok_front = np.array([[0.5, 0.9, 0.4], [0.5, 0.5, 0.5], [0.5, 0.4, 0.9]])
    ref = [1.0, 1.0, 1.0]

    def refused(code, word, fn):
        import bot7_amd
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    assert ctx.ehvi3_compute(mu, var, ok_front, ref).shape == (4,)
    refused(-1, "not sorted", lambda: ctx.ehvi3_compute(mu, var, ok_front[::-1], ref))
    refused(-1, "dominated", lambda: ctx.ehvi3_compute(mu, var, [[0.2, 0.3, 0.1], [0.5, 0.8, 0.2]], ref))
    refused(-1, "not sorted", lambda: ctx.ehvi3_compute(mu, var, [[0.2, 0.3, 0.1], [0.2, 0.3, 0.1]], ref))       # equal points
    refused(-1, "strictly inside", lambda: ctx.ehvi3_compute(mu, var, [[0.2, 0.2, 1.0]], ref))
    refused(-1, "not finite", lambda: ctx.ehvi3_compute(mu, var, ok_front, [1.0, np.inf, 1.0]))
    refused(-1, "not finite", lambda: ctx.ehvi3_compute(mu, var, [[0.2, np.nan, 0.2]], ref))
    big = np.zeros((R.SMAX + 1, 4))
    refused(-1, "hyper samples", lambda: ctx.ehvi3_compute([mu[0], mu[1], big], [var[0], var[1], big + 1.0], ok_front, ref))
    k = np.arange(R.PMAX + 1, dtype=np.float64)
    refused(-1, "front of %d points" % (R.PMAX + 1),
            lambda: ctx.ehvi3_compute(mu, var, np.stack([k / 1000, 1 - k / 1000, np.full(len(k), 0.5)], 1), [2.0, 2.0, 2.0]))
    empty = [np.zeros((1, 0))] * 3
    assert ctx.ehvi3_compute(empty, empty, ok_front, ref).shape == (0,)


# ---- 2. reduction to two objectives, and the deterministic limit -------------------------------------------------------------------
def test_reduction_to_two_objectives(ctx):
    """A front whose projections on the first two objectives are a canonical two-objective front, and a third posterior that is
    deterministic at v = r3 - 1/2, at or above every front point's third coordinate: every box below a front point scores
    T3 = (c - v)+ = 0, the final staircase's strips are the two-objective strips with T3 = r3 - v = 1/2 exactly, so
    ehvi3 = (r3 - v) b7_ehvi_compute(...), each side within its own bar of the common truth: the difference is within the sum of
    the two bars (the two-objective one times 1/2, an exact scaling)."""
    M, P, S1, S2 = 200, 5, 3, 2
    mu1, var1, mu2, var2 = R2.make_rows(M, S1, S2)
    front2 = R2.make_front(P)
    ref = np.array([R2.REF[0], R2.REF[1], 1.03125])
    v = ref[2] - 0.5
    c = np.random.default_rng(2).uniform(0.0, v, P)
    c[0] = v                                                   # "at": one front point as high as the third posterior sits
    front3, _ = R.canonical_front3(np.concatenate([front2, c[:, None]], axis=1), ref)
    assert len(front3) == P
    mu, var = [mu1, mu2, np.full((1, M), v)], [var1, var2, np.zeros((1, M))]
    got3 = ctx.ehvi3_compute(mu, var, front3, ref)
    got2 = ctx.ehvi_compute(mu1, var1, mu2, var2, front2, ref[:2])
    assert np.array_equal(np.isnan(got3), np.isnan(got2))
    ok = ~np.isnan(got2)
    hi3, lo3, scale3 = R.ehvi3_mp(mu, var, front3, ref)
    hi2, lo2 = R2.ehvi_mp(mu1, var1, mu2, var2, front2, ref[:2])
    scale2 = R2.empty_scale_mp(mu1, var1, mu2, var2, ref[:2])
    bar3 = E.gp_bar(R.err_vs_mp(R.ehvi3_numpy(mu, var, front3, ref), hi3, lo3)[ok], scale3[ok])
    bar2 = E.gp_bar(R2.err_vs_mp(R2.ehvi_numpy(mu1, var1, mu2, var2, front2, ref[:2]), hi2, lo2)[ok], scale2[ok])
    assert np.allclose(hi3[ok], 0.5 * hi2[ok], rtol=2 * E.EPS, atol=0)      # the two yardsticks agree on the truth, to their rounding
    diff, bar = np.abs(got3[ok] - 0.5 * got2[ok]), bar3 + 0.5 * bar2
    assert (diff[bar == 0.0] == 0.0).all()
    live = bar > 0.0
    print("ehvi3 = (r3 - v) ehvi2: worst difference / (sum of both bars) %.3g" % (diff[live] / bar[live]).max())
    assert (diff[live] <= bar[live]).all()


def test_the_deterministic_limit_is_the_hypervolume_improvement(ctx):
    """All variances 0, one sample each: Psi(a) = max(a - mu, 0) and the score is the hypervolume improvement of the point
    (mu1, mu2, mu3): against hv_brute's union of cells evaluated in rational arithmetic (so that the yardstick has no rounding of
    its own), to 16 eps x the row's scale, the improvement over an empty front prod_m (r_m - mu_m)+.  Points below the whole front,
    between its points, ON front points, dominated ones and ones outside the box (score exactly 0)."""
    front = R.make_front3(7)
    rng = np.random.default_rng(12)
    y = rng.uniform(0.0, 1.1, (64, 3))
    y[:7] = front
    y[7:14] = front - rng.uniform(0.0, 0.05, (7, 3))
    y[14:21] = front + rng.uniform(0.0, 0.05, (7, 3))
    y[21] = [0.1, 0.1, 0.1]
    y[22] = [0.2, 0.2, R.REF3[2]]
    zeros = [np.zeros((1, 64))] * 3
    got = ctx.ehvi3_compute([y[None, :, m] for m in range(3)], zeros, front, R.REF3)
    hi, lo = R.hv_improvement3_exact(front, R.REF3, y)
    scale = np.maximum(R.REF3 - y, 0.0).prod(axis=1)
    err = R.err_vs_mp(got, hi, lo)
    loose = R.hv_improvement3(front, R.REF3, y)                # hv_brute itself, in float64: the same volumes up to its own rounding
    assert np.allclose(loose, hi, rtol=0, atol=64 * E.EPS * float(R.REF3.prod()))
    live = scale > 0.0
    print("ehvi3 deterministic limit: worst error %.3g eps of the scale; %d rows improve" % ((err[live] / scale[live]).max() / E.EPS, (hi > 0).sum()))
    assert (got[~live] == 0.0).all() and (got[:7] == 0.0).all() and (got[14:21] == 0.0).all() and (hi[7:14] > 0).all()
    assert (err <= 16 * E.EPS * scale).all()


# ---- 3. the nomination end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx23():
    import bot7_amd
    cs = [bot7_amd.Context(0), bot7_amd.Context(0)]
    yield cs
    for c in cs:
        c.close()


def stage(c, X, y, Xc):
    c.gp_set_kernel("ardse")
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def three_objective_problem(N=30, d=2, M=333, seed=11):
    from harness import benchmarks as B
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    Y = B.three_spheres(X)
    hyps = []
    for col, S in ((0, 3), (1, 2), (2, 2)):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, 0.5 + 0.25 * s), "amp": amp * (1.0 + 0.3 * s), "noise": 1e-4 * amp,
                      "mean": float(np.mean(Y[:, col])) + 0.02 * s} for s in range(S)])
    return X, Y, Xc, hyps


def kept(c, S):
    got = [c.posterior_get(s) for s in range(S)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def test_nomination_end_to_end(ctx, ctx23):
    """Three contexts, N = 30, d = 2, M = 333, S = (3, 2, 2), responses from three_spheres.  The accumulator of b7_ehvi3_nominate
    equals b7_ehvi3_compute on the downloaded posteriors bit for bit and is within test 1's bar of the 50-digit marginal; the
    nominee is score:max(1) of it and its value is within the bar of the reference's maximum; coinciding contexts; the same call
    twice; an empty front; the other contexts' posteriors are untouched; the grid in two halves gives the same per-row bits.  On an
    MI355X: a front of 11, worst error / bar 0.0037."""
    from bot7_amd import _lib
    X, Y, Xc, hyps = three_objective_problem()
    M, cs, Ss = len(Xc), [ctx] + ctx23, (3, 2, 2)
    ref = np.array([0.9, 0.9, 0.9])
    front, rows = _lib.pareto_front3(Y, ref)
    assert 3 <= len(front) < len(Y)
    for k, c in enumerate(cs):
        stage(c, X, Y[:, k:k + 1], Xc)
        c.eval_posterior(hyps[k])
    val, idx = ctx.ehvi3_nominate(cs[1], cs[2], front, ref)
    v2, i2, acc = ctx.score_finish(1.0, download=True)
    posts = [kept(c, S) for c, S in zip(cs, Ss)]
    mu, var = [p[0] for p in posts], [p[1] for p in posts]
    want = ctx.ehvi3_compute(mu, var, front, ref)
    assert acc.tobytes() == want.tobytes()
    assert idx == i2 == R.nominee_ref(acc) + 1 and np.float64(val).tobytes() == np.float64(v2).tobytes() == acc[idx - 1].tobytes()
    worst = bar_ratio(acc, mu, var, front, ref)
    hi, lo, scale = R.ehvi3_mp(mu, var, front, ref)
    best = int(np.argmax(hi))
    bar_best = E.gp_bar(R.err_vs_mp(R.ehvi3_numpy(mu, var, front, ref), hi, lo)[[idx - 1, best]].max(), scale[[idx - 1, best]].max())
    print("ehvi3 nomination: front of %d, worst error / bar %.3g; nominee %d (reference's %d), value %.6g against %.6g"
          % (len(front), worst, idx, best + 1, val, hi[best]))
    # the values, not the indices, so a near-tie cannot fail (tests/test_gpu_ehvi.py)
    assert worst <= 1.0 and abs((val - hi[best]) - lo[best]) <= bar_best
    # the same call twice
    assert ctx.ehvi3_nominate(cs[1], cs[2], front, ref) == (val, idx) and ctx.score_finish(1.0, download=True)[2].tobytes() == acc.tobytes()
    # the other contexts' posteriors are untouched and their streams go on
    assert kept(cs[1], 2)[0].tobytes() == mu[1].tobytes() and kept(cs[2], 2)[1].tobytes() == var[2].tobytes()
    # coinciding contexts: all three the same, and the second and third the same
    ctx.ehvi3_nominate(ctx, ctx, front, ref)
    same = ctx.score_finish(1.0, download=True)[2]
    assert same.tobytes() == ctx.ehvi3_compute([mu[0]] * 3, [var[0]] * 3, front, ref).tobytes()
    v23, i23 = ctx.ehvi3_nominate(cs[1], cs[1], front, ref)
    two = ctx.score_finish(1.0, download=True)[2]
    assert two.tobytes() == ctx.ehvi3_compute([mu[0], mu[1], mu[1]], [var[0], var[1], var[1]], front, ref).tobytes() and i23 == R.nominee_ref(two) + 1
    # an empty front: T1(r1) T2(r2) T3(r3), finite everywhere and above every other score
    v0, i0 = ctx.ehvi3_nominate(cs[1], cs[2], np.zeros((0, 3)), ref)
    acc0 = ctx.score_finish(1.0, download=True)[2]
    assert np.isfinite(acc0).all() and (acc0 >= acc * (1.0 - 1e-12)).all() and bar_ratio(acc0, mu, var, np.zeros((0, 3)), ref) <= 1.0
    # grid-size independence: the two halves of the grid give the rows' bits
    for lo_, hi_ in ((0, 170), (170, M)):
        for k, c in enumerate(cs):
            c.grid_upload(Xc[lo_:hi_])
            c.eval_posterior(hyps[k])
        ctx.ehvi3_nominate(cs[1], cs[2], front, ref)
        assert ctx.score_finish(1.0, download=True)[2].tobytes() == acc[lo_:hi_].tobytes(), (lo_, hi_)


# ---- 4. state and refusals ----------------------------------------------------------------------------------------------------------
def test_state_and_refusals(ctx, ctx23):
    import bot7_amd
    X, Y, Xc, hyps = three_objective_problem(M=64)
    c2, c3 = ctx23
    ref = np.array([0.9, 0.9, 0.9])
    front = bot7_amd._lib.pareto_front3(Y, ref)[0]

    def refused(code, word, fn):
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            fn()
        assert e.value.code == code and word in str(e.value), str(e.value)

    for k, c in enumerate((ctx, c2, c3)):
        stage(c, X, Y[:, k:k + 1], Xc)
    # no kept posterior, on each side in turn
    refused(-4, "first objective", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    ctx.eval_posterior(hyps[0])
    refused(-4, "second objective", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    c2.eval_posterior(hyps[1])
    refused(-4, "third objective", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    c3.eval_posterior(hyps[2])
    val, idx = ctx.ehvi3_nominate(c2, c3, front, ref)
    # a non-canonical front, a bad reference point: by code and message, and nothing moved
    refused(-1, "not sorted", lambda: ctx.ehvi3_nominate(c2, c3, front[::-1], ref))
    refused(-1, "dominated", lambda: ctx.ehvi3_nominate(c2, c3, np.array([[0.1, 0.2, 0.1], [0.3, 0.4, 0.2]]), ref))
    refused(-1, "strictly inside", lambda: ctx.ehvi3_nominate(c2, c3, np.array([[0.1, 0.95, 0.1]]), ref))
    refused(-1, "not finite", lambda: ctx.ehvi3_nominate(c2, c3, front, [np.nan, 1.0, 1.0]))
    with pytest.raises(bot7_amd.Bot7HipError):
        ctx.ehvi3_nominate(c2, None, front, ref)
    assert ctx.ehvi3_nominate(c2, c3, front, ref) == (val, idx)
    # mismatched M; a grid change forgets the kept posterior
    c3.grid_upload(Xc[:40])
    refused(-4, "third objective", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    c3.eval_posterior(hyps[2])
    refused(-1, "third objective's grid has 40 rows, this one 64", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    c2.grid_remove(3)
    refused(-4, "second objective", lambda: ctx.ehvi3_nominate(c2, c3, front, ref))
    ctx.gp_set_data(X[:20], Y[:20, :1])
    refused(-4, "first objective", lambda: ctx.ehvi3_nominate(ctx, ctx, front, ref))
    # more samples than the kernels take are refused by the nomination, not by the posterior
    ctx.gp_set_data(X, Y[:, :1])
    many = [dict(hyps[0][0], amp=hyps[0][0]["amp"] * (1.0 + 0.01 * s)) for s in range(R.SMAX + 1)]
    ctx.eval_posterior(many)
    refused(-1, "hyper samples", lambda: ctx.ehvi3_nominate(ctx, ctx, front, ref))
    # a group member
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(Xc)
        g.gp_set_data(X, Y[:, :1])
        ctx.grid_upload(Xc[:32])
        ctx.eval_posterior(hyps[0])
        refused(-4, "group", lambda: ctx.ehvi3_nominate(ctx, g.members[0], front, ref))
        refused(-4, "group", lambda: ctx.ehvi3_nominate(g.members[1], ctx, front, ref))
    finally:
        g.close()


# ---- 5. the loop ----------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name, lo=0.0, hi=1.0):
        self.name, self.min, self.max, self.size = name, lo, hi, 1


def test_the_bot_with_three_objectives(ctx):
    """harness bayesopt with config.bot.objectives = {ref, models} on three_spheres, d = 2, 200 Sobol candidates, 3 random + 3
    model-based trials, S = 2, the slice sampler: the hypervolume against a fixed reference point never decreases; every
    model-based nominee is the arg-max of the score recomputed (b7_ehvi3_compute) from that trial's downloaded posteriors; the
    stolen row leaves all three resident grids."""
    import bot7_amd
    from bot7_amd import _lib
    from bot7_amd.grids.abstract import DeviceGrid
    from harness import benchmarks as B, bots
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    ref = [1.3, 1.3, 1.3]
    cfg = {"bot": {"verbose": 0, "budget": 6, "nInitial": 3, "nSamples": 2, "seed": 2,
                   "objectives": {"ref": ref, "models": [dict(mcfg, seed=6), dict(mcfg, seed=7)]}},
           "grid": {"type": "sobol", "size": 200, "dims": 2}, "score": {"type": "expected_hypervolume_improvement"}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 200, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    bot = bots.bayesopt(B.three_spheres, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})
    hv = []
    try:
        for t in range(6):
            before = np.asarray(bot.candidates).copy()
            x, y = bot.run_trial()
            bot.update_best(x, y)
            assert np.asarray(y).shape == (1, 3)
            front, _ = _lib.pareto_front3(bot.responses, ref)
            hv.append(_lib.hypervolume3(front, ref))
            assert hv[-1] == bot.best["hv"] and len(front) == len(bot.best["front"])
            assert abs(hv[-1] - R.hv_brute(bot.responses, ref)) <= 64 * E.EPS * 1.3 ** 3 * len(front)
            if t < 3:
                continue
            last, others = bot.last_objectives, bot.objectives23
            cs = [ctx, others[0]["ctx"], others[1]["ctx"]]
            # all three grids lost the nominee; before that they held the same rows, and the kept posteriors were of those rows
            assert np.array_equal(before[last["index"] - 1], x)
            for c in cs:
                assert np.array_equal(c.grid_download(), np.asarray(bot.candidates))
            # the nominee again, from this trial's hyper samples on fresh stagings of the grid as it stood
            n = t
            want_front, _ = _lib.pareto_front3(bot.responses[:n], ref)
            assert np.array_equal(last["front"], want_front)
            post = []
            for col, (c, hyps) in enumerate(zip(cs, last["hyps"])):
                c.grid_upload(before)
                c.gp_set_data(bot.observed[:n], bot.responses[:n, col:col + 1])
                c.eval_posterior(hyps)
                post.append(kept(c, 2))
            score = ctx.ehvi3_compute([p[0] for p in post], [p[1] for p in post], last["front"], ref)
            assert last["index"] == R.nominee_ref(score) + 1 and last["value"] == score[last["index"] - 1]
            assert ctx.ehvi3_nominate(cs[1], cs[2], last["front"], ref) == (last["value"], last["index"])
            # put the grids back as the bot left them
            for c in cs:
                c.grid_remove(last["index"])
            bot.candidates = DeviceGrid(np.asarray(bot.candidates), ctx, ctx.grid_version)
            for o in others:
                o["grid"] = DeviceGrid(np.asarray(bot.candidates), o["ctx"], o["ctx"].grid_version)
        print("three objectives: hypervolume per trial %s, front of %d" % (["%.4f" % h for h in hv], len(bot.best["front"])))
        assert all(b >= a for a, b in zip(hv, hv[1:])) and hv[-1] > 0.0
    finally:
        for o in bot.objectives23 or ():
            o["ctx"].close()
