"""b7_logehvi_compute / b7_logehvi_nominate on the GPU: two-objective nomination by the log of the exact expected hypervolume
improvement.

The kernel is measured against the log of the 50-digit marginal (tests/_logehvi_ref.logehvi_mp) with LogEI's measure and bar:
|got - ref| / max(1, |ref|) <= 1e-13 (_logei_ref.BAR), the classes (NaN, -inf) exact.  The accumulator, the nominee and the
composition with the feasibility column are compared bit for bit with the calls they restate.  Every test prints its figure."""
import numpy as np
import pytest

import _ehvi_ref as R2
import _logehvi_ref as R

pytestmark = pytest.mark.gpu


def refused(code, word, fn):
    import bot7_amd
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


# ---- 1. the kernel against 50 digits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,S1,S2", R.KERNEL_CASES)
def test_kernel_against_50_digits(ctx, M, P, S1, S2):
    """b7_logehvi_compute on _logehvi_ref.make_rows_log (z down to -1e4, sigma 1e-8 .. 1e2, var == 0 in one sample and in all, the
    NaN and var < 0 classes) against fronts whose first two points are one ulp apart.  M = 1000 spans sixteen workgroups and ends
    inside one; (11, 1) puts one sample in LDS, (32, 32) twenty-two of each.  The same call twice: the same bits; rows 37:101 alone:
    the bits they have in the whole call.  On an MI355X the worst scaled error over the seven cases is 2.6e-15 (M = 257, P = 0)."""
    mu1, var1, mu2, var2 = R.make_rows_log(M, S1, S2)
    front = R2.make_front(P)
    got = ctx.logehvi_compute(mu1, var1, mu2, var2, front, R2.REF)
    assert got.shape == (M,)
    keep = np.arange(M) if M <= 300 else np.unique(np.concatenate([np.arange(16), np.arange(M)[::4], [M - 1]]))
    err = R.scaled_errors(got[keep], R.logehvi_mp(mu1[:, keep], var1[:, keep], mu2[:, keep], var2[:, keep], front, R2.REF))
    lin = ctx.ehvi_compute(mu1, var1, mu2, var2, front, R2.REF)
    assert np.array_equal(np.isnan(got), np.isnan(lin)) and not (got == np.inf).any()        # NaN exactly where the linear score is
    print("logehvi kernel M=%d P=%d S=(%d, %d): worst scaled error %.3g; %d rows have a linear score of exactly 0"
          % (M, P, S1, S2, err.max(), int((lin == 0.0).sum())))
    assert err.max() <= R.BAR
    assert ctx.logehvi_compute(mu1, var1, mu2, var2, front, R2.REF).tobytes() == got.tobytes()
    if M >= 128:
        part = ctx.logehvi_compute(mu1[:, 37:101], var1[:, 37:101], mu2[:, 37:101], var2[:, 37:101], front, R2.REF)
        assert part.tobytes() == got[37:101].tobytes()


# ---- 3. identities, bit for bit --------------------------------------------------------------------------------------------------
def test_empty_front_one_sample_is_the_sum_of_two_logeis(ctx):
    """P = 0, S = 1 each: the output equals logei_compute(mu1, var1, r1) + logei_compute(mu2, var2, r2) bit for bit: a difference
    against -inf, a log-sum-exp of one term and the subtraction of log 1 change nothing."""
    mu1, var1, mu2, var2 = R.make_rows_log(300, 1, 1, seed=9)
    got = ctx.logehvi_compute(mu1, var1, mu2, var2, np.zeros((0, 2)), R2.REF)
    want = ctx.logei_compute(mu1[0], var1[0], np.array([R2.REF[0]])) + ctx.logei_compute(mu2[0], var2[0], np.array([R2.REF[1]]))
    ok = ~R2._bad(mu1, var1, mu2, var2)
    print("logehvi identity: %d rows compared bit for bit, %d of them -inf" % (ok.sum(), int((got[ok] == -np.inf).sum())))
    assert got[ok].tobytes() == want[ok].tobytes() and np.isnan(got[~ok]).all() and np.isnan(want[~ok]).all()


# ---- 4. it ranks where the linear score cannot --------------------------------------------------------------------------------------
def test_it_ranks_where_the_linear_score_cannot(ctx):
    """_logehvi_ref.far_rows: 256 rows, objective 1 between 45 and 200 sigma beyond every strip's edge.  b7_ehvi_compute returns
    all zeros, whose score:max(1) (b7_argmax: the nomination's own finish) is row 1; the log score returns the 50-digit arg-max (not
    row 1, a gap of 6.6 % of the value to the runner-up).  On an MI355X: nominee 145 = the 50-digit arg-max, worst scaled error 1.1e-15."""
    mu1, var1, mu2, var2, front, ref = R.far_rows()
    lin = ctx.ehvi_compute(mu1, var1, mu2, var2, front, ref)
    assert (lin == 0.0).all() and ctx.argmax(lin)[1] == 1
    ref_mp = R.logehvi_mp(mu1, var1, mu2, var2, front, ref)
    best, gap = R.argmax_mp(ref_mp)
    got = ctx.logehvi_compute(mu1, var1, mu2, var2, front, ref)
    err = R.scaled_errors(got, ref_mp)
    val, idx = ctx.argmax(got)
    print("far rows: linear scores all 0 (nominee 1); log nominee %d, 50-digit arg-max %d (gap %.3g), worst scaled error %.3g"
          % (idx, best + 1, gap, err.max()))
    assert best != 0 and gap >= 1e-6 and idx == best + 1 and err.max() <= R.BAR


# ---- 5. the nomination end to end ---------------------------------------------------------------------------------------------------
def problem(N, d, M, S, seed, nobj=2):
    """tests/test_gpu_ehvi.py's problem with further responses over the same points: -> X, Y (N x nobj), Xc, hyps[objective][sample]."""
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rng.standard_normal(N)
    cols = [y, np.cos(2.0 * X[:, :2].sum(axis=1)) + (1.0 - X[:, 0]) ** 2 + 0.05 * rng.standard_normal(N),
            ((X - 0.6) ** 2).sum(axis=1) + 0.05 * rng.standard_normal(N)][:nobj]
    hyps = []
    for col in cols:
        amp = float(np.var(col))
        hyps.append([{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
                      "mean": float(np.mean(col)) + 0.05 * s} for s in range(S)])
    return X, np.stack(cols, axis=1), Xc, hyps


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def kept(c, S):
    got = [c.posterior_get(s) for s in range(S)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


@pytest.fixture(scope="module")
def ctx2():
    import bot7_amd
    c = bot7_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("N,d,S,kernels,far_ref", [(24, 3, 2, ("ardse", "ardse"), False), (160, 4, 1, ("ardse", "ardmatern52"), False),
                                                   (24, 3, 2, ("ardse", "ardmatern52"), True)])
def test_nomination_end_to_end(ctx, ctx2, N, d, S, kernels, far_ref):
    """Kept posteriors from eval_posterior on the small-regime route (N = 24) and the general route (N = 160), M = 300; far_ref: a
    reference point that no observation has reached, so P = 0.  The accumulator (score_finish(1.0, download=True)) equals
    logehvi_compute on the posterior_get downloads bit for bit, the nominee is its first maximum, and the values are within BAR of
    the 50-digit log marginal.  On an MI355X: 1.4e-15 at the worst (the P = 0 case, where 19 of 300 linear scores are exactly 0)."""
    from bot7_amd import _lib
    X, Y, Xc, hyps = problem(N, d, 300, S, 4)
    ref = Y.min(axis=0) - 0.5 if far_ref else Y.max(axis=0) - 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    front, _ = _lib.pareto_front2(Y, ref)
    assert (len(front) == 0) if far_ref else (len(front) >= 2)
    for c, k in ((ctx, 0), (ctx2, 1)):
        stage(c, X, Y[:, k:k + 1], Xc, kernels[k])
        c.eval_posterior(hyps[k])
    val, idx = ctx.logehvi_nominate(ctx2, front, ref)
    v2, i2, acc = ctx.score_finish(1.0, download=True)
    (mu1, var1), (mu2, var2) = kept(ctx, S), kept(ctx2, S)
    want = ctx.logehvi_compute(mu1, var1, mu2, var2, front, ref)
    assert acc.tobytes() == want.tobytes()
    assert idx == i2 == R2.nominee_ref(acc) + 1 and np.float64(val).tobytes() == np.float64(v2).tobytes() == acc[idx - 1].tobytes()
    err = R.scaled_errors(acc[::3], R.logehvi_mp(mu1[:, ::3], var1[:, ::3], mu2[:, ::3], var2[:, ::3], front, ref))
    lin = ctx.ehvi_compute(mu1, var1, mu2, var2, front, ref)
    print("logehvi nomination N=%d S=%d P=%d: nominee %d, log value %.6g, worst scaled error %.3g; %d of 300 linear scores are exactly 0"
          % (N, S, len(front), idx, val, err.max(), int((lin == 0.0).sum())))
    assert err.max() <= R.BAR
    assert ctx.logehvi_nominate(ctx2, front, ref) == (val, idx) and ctx.score_finish(1.0, download=True)[2].tobytes() == acc.tobytes()
    assert kept(ctx2, S)[0].tobytes() == mu2.tobytes()                     # the second context's posterior is untouched


# ---- 7. constrained composition -----------------------------------------------------------------------------------------------------
def test_constrained_composition_through_the_feasibility_column(ctx, ctx2):
    """After logehvi_nominate the accumulator is a log one: feas_reset, feas_add(L) with one -inf on the unconstrained nominee's
    row, feas_add_acc(ctx), feas_nominate: the value equals max(acc + L) from the downloads bit for bit and the masked row is not
    chosen.  After the linear ehvi_nominate, feas_add_acc still refuses."""
    from bot7_amd import _lib
    X, Y, Xc, hyps = problem(24, 3, 300, 2, 4)
    ref = Y.max(axis=0)
    front, _ = _lib.pareto_front2(Y, ref)
    for c, k in ((ctx, 0), (ctx2, 1)):
        stage(c, X, Y[:, k:k + 1], Xc)
        c.eval_posterior(hyps[k])
    val, idx = ctx.logehvi_nominate(ctx2, front, ref)
    acc = ctx.score_finish(1.0, download=True)[2]
    L = -np.random.default_rng(1).random(300)
    L[idx - 1] = -np.inf
    ctx.feas_reset()
    ctx.feas_add(L)
    ctx.feas_add_acc(ctx)
    v, i = ctx.feas_nominate()
    want = (0.0 + L) + acc
    print("constrained composition: unconstrained nominee %d (%.6g), constrained nominee %d (%.6g)" % (idx, val, i, v))
    assert i != idx and i == R2.nominee_ref(want) + 1 and np.float64(v).tobytes() == want[i - 1].tobytes()
    assert ctx.feas_get().tobytes() == want.tobytes()
    ctx.ehvi_nominate(ctx2, front, ref)
    refused(-4, "linear sum", lambda: ctx.feas_add_acc(ctx))


# ---- 8. state and refusals ----------------------------------------------------------------------------------------------------------
def test_state_and_refusals(ctx, ctx2):
    import bot7_amd
    X, Y, Xc, hyps = problem(24, 3, 64, 2, 4)
    ref = Y.max(axis=0)
    front = bot7_amd._lib.pareto_front2(Y, ref)[0]
    assert len(front) >= 2
    stage(ctx, X, Y[:, :1], Xc)
    stage(ctx2, X, Y[:, 1:], Xc)
    refused(-4, "first objective", lambda: ctx.logehvi_nominate(ctx2, front, ref))
    ctx.eval_posterior(hyps[0])
    refused(-4, "second objective", lambda: ctx.logehvi_nominate(ctx2, front, ref))
    ctx2.eval_posterior(hyps[1])
    val, idx = ctx.logehvi_nominate(ctx2, front, ref)
    refused(-1, "not sorted", lambda: ctx.logehvi_nominate(ctx2, front[::-1], ref))
    refused(-1, "dominated", lambda: ctx.logehvi_nominate(ctx2, np.array([front[0], [front[-1, 0], front[0, 1]]]), ref))
    refused(-1, "strictly inside", lambda: ctx.logehvi_nominate(ctx2, np.array([[front[0, 0], ref[1]]]), ref))
    refused(-1, "not finite", lambda: ctx.logehvi_nominate(ctx2, front, [np.nan, 1.0]))
    assert ctx.logehvi_nominate(ctx2, front, ref) == (val, idx)
    ctx2.grid_upload(Xc[:40])
    refused(-4, "second objective", lambda: ctx.logehvi_nominate(ctx2, front, ref))
    ctx2.eval_posterior(hyps[1])
    refused(-1, "40 rows, this one 64", lambda: ctx.logehvi_nominate(ctx2, front, ref))
    many = [dict(hyps[0][0], amp=hyps[0][0]["amp"] * (1.0 + 0.01 * s)) for s in range(R2.SMAX + 1)]
    ctx.eval_posterior(many)
    refused(-1, "hyper samples", lambda: ctx.logehvi_nominate(ctx, front, ref))
    # the compute call: S and P beyond the caps, a non-canonical front, M = 0
    mu, var = np.zeros((1, 4)), np.ones((1, 4))
    big = np.zeros((R2.SMAX + 1, 4))
    refused(-1, "hyper samples", lambda: ctx.logehvi_compute(big, big + 1.0, mu, var, front, ref))
    k = np.arange(R2.PMAX + 1, dtype=np.float64)
    refused(-1, "front of %d points" % (R2.PMAX + 1), lambda: ctx.logehvi_compute(mu, var, mu, var, np.stack([k / 1000, 1 - k / 1000], 1), [2.0, 2.0]))
    refused(-1, "not sorted", lambda: ctx.logehvi_compute(mu, var, mu, var, front[::-1], ref))
    e = np.zeros((1, 0))
    assert ctx.logehvi_compute(e, e, e, e, front, ref).shape == (0,)
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(Xc)
        g.gp_set_data(X, Y[:, :1])
        ctx.grid_upload(Xc[:32])
        ctx.eval_posterior(hyps[0])
        refused(-4, "group", lambda: ctx.logehvi_nominate(g.members[0], front, ref))
    finally:
        g.close()
