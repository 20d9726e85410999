"""b7_logehvi3_compute / b7_logehvi3_nominate on the GPU: three-objective nomination by the log of the exact expected hypervolume
improvement over the box decomposition.

Measured as tests/test_gpu_logehvi.py measures: |got - ref| / max(1, |ref|) <= 1e-13 (_logei_ref.BAR) against the log of the
50-digit marginal (_logehvi_ref.logehvi3_mp, a decomposition of its own), the classes (NaN, -inf) exact; the accumulator, the nominee
and the chunked walk bit for bit.  Every test prints its figure."""
import mpmath
import numpy as np
import pytest

import _ehvi3_ref as R3
import _ehvi_ref as R2
import _logehvi_ref as R
from test_gpu_logehvi import kept, problem, refused, stage

pytestmark = pytest.mark.gpu


# ---- 1. the kernels against 50 digits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,P,S1,S2,S3", R.KERNEL_CASES3)
def test_kernel_against_50_digits(ctx, M, P, S1, S2, S3):
    """b7_logehvi3_compute on _logehvi_ref.make_rows3_log (z down to -1e4; the special classes in each objective) against
    _ehvi3_ref's fronts (one-ulp-apart and shared coordinates).  M = 1000 ends inside a workgroup of either kernel; P = 33 and 256 end
    inside a block of eight cuts.  The same call twice: the same bits; rows 37:101 alone: the bits they have in the whole call.  On an
    MI355X the worst scaled error over the seven cases is 2.3e-15 (M = 257, P = 0)."""
    mu, var = R.make_rows3_log(M, (S1, S2, S3))
    front = R3.make_front3(P)
    got = ctx.logehvi3_compute(mu, var, front, R3.REF3)
    assert got.shape == (M,)
    keep = np.arange(M) if M <= 100 else np.unique(np.concatenate([np.arange(16), np.arange(M)[:: max(1, M // 60)], [M - 1]]))
    err = R.scaled_errors(got[keep], R.logehvi3_mp([m[:, keep] for m in mu], [v[:, keep] for v in var], front, R3.REF3))
    lin = ctx.ehvi3_compute(mu, var, front, R3.REF3)
    assert np.array_equal(np.isnan(got), np.isnan(lin)) and not (got == np.inf).any()
    print("logehvi3 kernels M=%d P=%d S=(%d, %d, %d): worst scaled error %.3g; %d rows have a linear score of exactly 0"
          % (M, P, S1, S2, S3, err.max(), int((lin == 0.0).sum())))
    assert err.max() <= R.BAR
    assert ctx.logehvi3_compute(mu, var, front, R3.REF3).tobytes() == got.tobytes()
    if M >= 128:
        part = ctx.logehvi3_compute([m[:, 37:101] for m in mu], [v[:, 37:101] for v in var], front, R3.REF3)
        assert part.tobytes() == got[37:101].tobytes()


# ---- 2. chunk independence ----------------------------------------------------------------------------------------------------------
def test_chunking_does_not_change_a_bit(ctx):
    """M = 300, P = 33 (852 bytes of table per candidate): one chunk under the default workspace, three under the smallest one
    b7_set_workspace takes (128 KiB: 128 candidates per chunk); the rows' bits are the same."""
    mu, var = R.make_rows3_log(300, (3, 2, 2), seed=1)
    front = R3.make_front3(33)

    def counted():
        ctx.profile_enable(True)
        try:
            ctx.profile_reset()
            out = ctx.logehvi3_compute(mu, var, front, R3.REF3)
            return out, ctx.profile_get("logehvi3_tab")[1]
        finally:
            ctx.profile_enable(False)
    whole, n1 = counted()
    try:
        ctx.set_workspace(128 << 10)
        cut, n3 = counted()
    finally:
        ctx.set_workspace(4 << 30)
    print("logehvi3 chunking: %d chunk(s) by default, %d under a 128 KiB workspace" % (n1, n3))
    assert n1 == 1 and n3 >= 3 and cut.tobytes() == whole.tobytes()


# ---- 3. identities, bit for bit --------------------------------------------------------------------------------------------------
def test_empty_front_one_sample_is_the_sum_of_three_logeis(ctx):
    """P = 0, S = 1 each: the output equals (l1 + l2) + l3, l_m = logei_compute(mu_m, var_m, r_m), bit for bit."""
    mu, var = R.make_rows3_log(300, (1, 1, 1), seed=9)
    got = ctx.logehvi3_compute(mu, var, np.zeros((0, 3)), R3.REF3)
    l = [ctx.logei_compute(mu[m][0], var[m][0], np.array([R3.REF3[m]])) for m in range(3)]
    want = (l[0] + l[1]) + l[2]
    ok = ~R3._bad3(mu, var)
    print("logehvi3 identity: %d rows compared bit for bit, %d of them -inf" % (ok.sum(), int((got[ok] == -np.inf).sum())))
    assert got[ok].tobytes() == want[ok].tobytes() and np.isnan(got[~ok]).all() and np.isnan(want[~ok]).all()


# ---- 4. it ranks where the linear score cannot --------------------------------------------------------------------------------------
def test_it_ranks_where_the_linear_score_cannot(ctx):
    """_logehvi_ref.far_rows3: 256 rows, objective 1 between 45 and 200 sigma beyond every box's edge.  b7_ehvi3_compute returns all
    zeros, whose score:max(1) (b7_argmax: the nomination's own finish) is row 1; the log score returns the 50-digit arg-max.  On an
    MI355X: nominee 165 = the 50-digit arg-max (gap 1.9 %), worst scaled error 7.2e-16."""
    mu, var, front, ref = R.far_rows3()
    lin = ctx.ehvi3_compute(mu, var, front, ref)
    assert (lin == 0.0).all() and ctx.argmax(lin)[1] == 1
    ref_mp = R.logehvi3_mp(mu, var, front, ref)
    best, gap = R.argmax_mp(ref_mp)
    got = ctx.logehvi3_compute(mu, var, front, ref)
    err = R.scaled_errors(got, ref_mp)
    val, idx = ctx.argmax(got)
    print("far rows, three objectives: linear scores all 0 (nominee 1); log nominee %d, 50-digit arg-max %d (gap %.3g), worst scaled error %.3g"
          % (idx, best + 1, gap, err.max()))
    assert best != 0 and gap >= 1e-6 and idx == best + 1 and err.max() <= R.BAR


# ---- 5. the nomination end to end ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx23():
    import bot7_amd
    cs = [bot7_amd.Context(0), bot7_amd.Context(0)]
    yield cs
    for c in cs:
        c.close()


@pytest.mark.parametrize("N,d,S,kernels,far_ref", [(24, 3, 2, ("ardse", "ardse", "ardse"), False),
                                                   (160, 4, 1, ("ardse", "ardmatern52", "ardse"), False),
                                                   (24, 3, 2, ("ardse", "ardse", "ardmatern52"), True)])
def test_nomination_end_to_end(ctx, ctx23, N, d, S, kernels, far_ref):
    """Kept posteriors of three contexts on the small-regime route (N = 24) and the general route (N = 160), M = 300; far_ref: a
    reference point no observation has reached, so P = 0.  The accumulator equals logehvi3_compute on the posterior_get downloads
    bit for bit, the nominee is its first maximum, the values are within BAR of the 50-digit log marginal.  On an MI355X: 1.8e-15 at
    the worst (the P = 0 case, where 150 of 300 linear scores are exactly 0)."""
    from bot7_amd import _lib
    X, Y, Xc, hyps = problem(N, d, 300, S, 4, nobj=3)
    ref = Y.min(axis=0) - 0.5 if far_ref else Y.max(axis=0) - 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    front, _ = _lib.pareto_front3(Y, ref)
    assert (len(front) == 0) if far_ref else (len(front) >= 3)
    cs = [ctx] + ctx23
    for k, c in enumerate(cs):
        stage(c, X, Y[:, k:k + 1], Xc, kernels[k])
        c.eval_posterior(hyps[k])
    val, idx = ctx.logehvi3_nominate(cs[1], cs[2], front, ref)
    v2, i2, acc = ctx.score_finish(1.0, download=True)
    posts = [kept(c, S) for c in cs]
    mu, var = [p[0] for p in posts], [p[1] for p in posts]
    want = ctx.logehvi3_compute(mu, var, front, ref)
    assert acc.tobytes() == want.tobytes()
    assert idx == i2 == R2.nominee_ref(acc) + 1 and np.float64(val).tobytes() == np.float64(v2).tobytes() == acc[idx - 1].tobytes()
    step = 10 if len(front) > 10 else 4
    err = R.scaled_errors(acc[::step], R.logehvi3_mp([m[:, ::step] for m in mu], [v[:, ::step] for v in var], front, ref))
    lin = ctx.ehvi3_compute(mu, var, front, ref)
    print("logehvi3 nomination N=%d S=%d P=%d: nominee %d, log value %.6g, worst scaled error %.3g; %d of 300 linear scores are exactly 0"
          % (N, S, len(front), idx, val, err.max(), int((lin == 0.0).sum())))
    assert err.max() <= R.BAR
    assert ctx.logehvi3_nominate(cs[1], cs[2], front, ref) == (val, idx) and ctx.score_finish(1.0, download=True)[2].tobytes() == acc.tobytes()
    assert kept(cs[1], S)[0].tobytes() == mu[1].tobytes() and kept(cs[2], S)[1].tobytes() == var[2].tobytes()


# ---- 6. reductions ------------------------------------------------------------------------------------------------------------------
def test_reduction_to_two_objectives(ctx):
    """tests/test_gpu_ehvi3.py's reduction: a third posterior deterministic at v = r3 - 1/2, at or above every front point's third
    coordinate, so the score is (r3 - v) x the two-objective one: log score = log(1/2) + b7_logehvi_compute(...).  Each side is
    within BAR of its own 50-digit truth, the truths agree, and the two sides differ by no more than the sum of their bars."""
    M, P, S1, S2 = 120, 5, 3, 2
    mu1, var1, mu2, var2 = R.make_rows_log(M, S1, S2)
    front2 = R2.make_front(P)
    ref = np.array([R2.REF[0], R2.REF[1], 1.03125])
    v = ref[2] - 0.5
    c = np.random.default_rng(2).uniform(0.0, v, P)
    c[0] = v
    front3, _ = R3.canonical_front3(np.concatenate([front2, c[:, None]], axis=1), ref)
    assert len(front3) == P
    mu, var = [mu1, mu2, np.full((1, M), v)], [var1, var2, np.zeros((1, M))]
    got3 = ctx.logehvi3_compute(mu, var, front3, ref)
    got2 = ctx.logehvi_compute(mu1, var1, mu2, var2, front2, ref[:2])
    t3, t2 = R.logehvi3_mp(mu, var, front3, ref), R.logehvi_mp(mu1, var1, mu2, var2, front2, ref[:2])
    e3, e2 = R.scaled_errors(got3, t3), R.scaled_errors(got2, t2)
    worst = 0.0
    with mpmath.workdps(R.DPS):
        for j in range(M):
            if t2[j] is None or t2[j] == mpmath.mpf("-inf"):
                continue
            assert abs(t3[j] - (t2[j] + mpmath.log(mpmath.mpf("0.5")))) <= mpmath.mpf("1e-40") * max(1, abs(t3[j]))
            worst = max(worst, abs(got3[j] - (got2[j] + np.log(0.5))) / max(1.0, abs(got3[j])))
    print("logehvi3 = log(1/2) + logehvi: worst scaled errors %.3g / %.3g, worst scaled difference %.3g" % (e3.max(), e2.max(), worst))
    assert e3.max() <= R.BAR and e2.max() <= R.BAR and worst <= 2 * R.BAR + 2.0 ** -52


def test_the_deterministic_limit_is_the_log_hypervolume_improvement(ctx):
    """All variances 0, one sample each: the log score is the log of the hypervolume improvement of the point (mu1, mu2, mu3), against
    hv_brute's union of cells in rational arithmetic, within BAR; -inf exactly for points on the front, dominated ones and ones
    outside the box."""
    front = R3.make_front3(7)
    rng = np.random.default_rng(12)
    y = rng.uniform(0.0, 1.1, (64, 3))
    y[:7] = front
    y[7:14] = front - rng.uniform(0.0, 0.05, (7, 3))
    y[14:21] = front + rng.uniform(0.0, 0.05, (7, 3))
    y[21] = [0.1, 0.1, 0.1]
    y[22] = [0.2, 0.2, R3.REF3[2]]
    zeros = [np.zeros((1, 64))] * 3
    got = ctx.logehvi3_compute([y[None, :, m] for m in range(3)], zeros, front, R3.REF3)
    hi, lo = R3.hv_improvement3_exact(front, R3.REF3, y)
    with mpmath.workdps(R.DPS):
        truth = [mpmath.log(mpmath.mpf(h) + mpmath.mpf(l)) if h > 0 else mpmath.mpf("-inf") for h, l in zip(hi, lo)]
    err = R.scaled_errors(got, truth)
    print("logehvi3 deterministic limit: worst scaled error %.3g; %d rows improve, %d are -inf" % (err.max(), (hi > 0).sum(), (got == -np.inf).sum()))
    assert (got[:7] == -np.inf).all() and (got[14:21] == -np.inf).all() and (hi[7:14] > 0).all() and err.max() <= R.BAR


# ---- 7. constrained composition -----------------------------------------------------------------------------------------------------
def test_constrained_composition_through_the_feasibility_column(ctx, ctx23):
    """tests/test_gpu_logehvi.py's composition after logehvi3_nominate; after the linear ehvi3_nominate feas_add_acc still refuses."""
    from bot7_amd import _lib
    X, Y, Xc, hyps = problem(24, 3, 300, 2, 4, nobj=3)
    ref = Y.max(axis=0)
    front, _ = _lib.pareto_front3(Y, ref)
    cs = [ctx] + ctx23
    for k, c in enumerate(cs):
        stage(c, X, Y[:, k:k + 1], Xc)
        c.eval_posterior(hyps[k])
    val, idx = ctx.logehvi3_nominate(cs[1], cs[2], front, ref)
    acc = ctx.score_finish(1.0, download=True)[2]
    L = -np.random.default_rng(1).random(300)
    L[idx - 1] = -np.inf
    ctx.feas_reset()
    ctx.feas_add(L)
    ctx.feas_add_acc(ctx)
    v, i = ctx.feas_nominate()
    want = (0.0 + L) + acc
    print("constrained composition, three objectives: unconstrained nominee %d (%.6g), constrained nominee %d (%.6g)" % (idx, val, i, v))
    assert i != idx and i == R2.nominee_ref(want) + 1 and np.float64(v).tobytes() == want[i - 1].tobytes()
    ctx.ehvi3_nominate(cs[1], cs[2], front, ref)
    refused(-4, "linear sum", lambda: ctx.feas_add_acc(ctx))


# ---- 8. state and refusals ----------------------------------------------------------------------------------------------------------
def test_state_and_refusals(ctx, ctx23):
    import bot7_amd
    X, Y, Xc, hyps = problem(24, 3, 64, 2, 4, nobj=3)
    c2, c3 = ctx23
    ref = Y.max(axis=0)
    front = bot7_amd._lib.pareto_front3(Y, ref)[0]
    assert len(front) >= 3
    for k, c in enumerate((ctx, c2, c3)):
        stage(c, X, Y[:, k:k + 1], Xc)
    refused(-4, "first objective", lambda: ctx.logehvi3_nominate(c2, c3, front, ref))
    ctx.eval_posterior(hyps[0])
    refused(-4, "second objective", lambda: ctx.logehvi3_nominate(c2, c3, front, ref))
    c2.eval_posterior(hyps[1])
    refused(-4, "third objective", lambda: ctx.logehvi3_nominate(c2, c3, front, ref))
    c3.eval_posterior(hyps[2])
    val, idx = ctx.logehvi3_nominate(c2, c3, front, ref)
    refused(-1, "not sorted", lambda: ctx.logehvi3_nominate(c2, c3, front[::-1], ref))
    refused(-1, "dominated", lambda: ctx.logehvi3_nominate(c2, c3, np.array([front[0], front[0] + 1e-6]), ref))
    refused(-1, "strictly inside", lambda: ctx.logehvi3_nominate(c2, c3, np.array([[front[0, 0], front[0, 1], ref[2]]]), ref))
    refused(-1, "not finite", lambda: ctx.logehvi3_nominate(c2, c3, front, [1.0, np.nan, 1.0]))
    assert ctx.logehvi3_nominate(c2, c3, front, ref) == (val, idx)
    c3.grid_upload(Xc[:40])
    refused(-4, "third objective", lambda: ctx.logehvi3_nominate(c2, c3, front, ref))
    c3.eval_posterior(hyps[2])
    refused(-1, "40 rows, this one 64", lambda: ctx.logehvi3_nominate(c2, c3, front, ref))
    many = [dict(hyps[0][0], amp=hyps[0][0]["amp"] * (1.0 + 0.01 * s)) for s in range(R2.SMAX + 1)]
    ctx.eval_posterior(many)
    refused(-1, "hyper samples", lambda: ctx.logehvi3_nominate(ctx, ctx, front, ref))
    # the compute call: S and P beyond the caps, a non-canonical front, M = 0
    mu, var = [np.zeros((1, 4))] * 3, [np.ones((1, 4))] * 3
    big = np.zeros((R2.SMAX + 1, 4))
    refused(-1, "hyper samples", lambda: ctx.logehvi3_compute([mu[0], mu[1], big], [var[0], var[1], big + 1.0], front, ref))
    k = np.arange(R3.PMAX + 1, dtype=np.float64)
    refused(-1, "front of %d points" % (R3.PMAX + 1),
            lambda: ctx.logehvi3_compute(mu, var, np.stack([k / 1000, 1 - k / 1000, np.full(len(k), 0.5)], 1), [2.0, 2.0, 2.0]))
    refused(-1, "not sorted", lambda: ctx.logehvi3_compute(mu, var, front[::-1], ref))
    empty = [np.zeros((1, 0))] * 3
    assert ctx.logehvi3_compute(empty, empty, front, ref).shape == (0,)
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(Xc)
        g.gp_set_data(X, Y[:, :1])
        ctx.grid_upload(Xc[:32])
        ctx.eval_posterior(hyps[0])
        refused(-4, "group", lambda: ctx.logehvi3_nominate(g.members[0], c2, front, ref))
    finally:
        g.close()
