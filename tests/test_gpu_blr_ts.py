"""Thompson sampling on the Bayesian-linear head: b7_blr_paths_compute, b7_blr_ts_nominate, b7_blr_ts_last_draws and the harness bot
with the dngo model.  Needs an MI355X: run with -m gpu.

References and bars: tests/_blr_ts_ref.py (host tests: tests/test_blr_ts_host.py).  The paths kernel against integer arithmetic bit
for bit on dyadic operands, and against the exact evaluation of its own operands within _blr_ref.mean_bar otherwise; the draws
against the numpy restatement of the counter generator; the weights against L^-T eps in double-double, GIVEN the device's own L^-1, m
(b7_blr_fit_x + b7_gp_download of the same head) and eps, within 8 x numpy's own error + 16 eps sum |L^-1| |eps|; the nominees by
_ts_ref.nominees_ref on the device's own paths, exactly.  The heads of the one-launch route are given hypers that make A and b exact
in float64 (_blr_ref.exact_head), so that both routes factor the same matrix.  Every test prints its worst error / bar ratio
(DESIGN.md section 8 records them)."""
import numpy as np
import pytest

import _blr_ref as B
import _blr_ts_ref as R
from conftest import make_network

pytestmark = pytest.mark.gpu
ACT = "ReLU"
M = 257
SEED = 20262
ROWS = np.unique(np.concatenate([np.linspace(0, M - 1, 24).astype(int), [15, 16, 17, 255, 256]]))
# (alpha, beta, mean) of up to three heads: powers of two and dyadic means (_blr_ref.exact_head's conditions)
HYPS = [(2.0 ** -4, 2.0 ** 6, 2.0 ** -2), (2.0 ** -3, 2.0 ** 5, -(2.0 ** -1)), (2.0 ** -6, 2.0 ** 6, 0.0)]
FAST_NZ, GENERAL_NZ = [(10, 64), (65, 49), (200, 50)], [(15, 65), (300, 256)]
SQ = [(1, 1), (3, 5), (1, 16), (3, 16)]
_PROBLEMS = {}


def problem(N, z):
    if (N, z) not in _PROBLEMS:
        _PROBLEMS[(N, z)] = B.problem(N, z, M)
    return _PROBLEMS[(N, z)]


def nominate(c, p, hyps, q, seed=SEED, grid=None):
    c.grid_upload(p.Xg if grid is None else grid)
    a, b, m = zip(*hyps)
    vals, idx, rep = c.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, a, b, m, q, seed=seed, want_report=True)
    return vals, idx, rep, c.ts_last_paths(), [c.blr_ts_last_draws(j) for j in range(q)]


def heads(c, p, hyps):
    """(L^-1, m) of every head as b7_blr_fit_x leaves it: the device's own operands of the weight draw."""
    out = []
    for a, b, mn in hyps:
        c.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, a, b, mn)
        _, m, Li = c.gp_download(p.z)
        out.append((Li, m[:, 0]))
    return out


def check_rule(P, vals, idx):
    assert (idx - 1).tolist() == R.nominees_ref(P)
    assert all(np.float64(vals[j]).tobytes() == P[idx[j] - 1, j].tobytes() for j in range(len(idx)))


def check_call(c, p, hyps, q, out, tag):
    """The whole chain of one nomination: draws, weights, paths, nominees.  Returns the worst ratios."""
    vals, idx, rep, P, dr = out
    S, z = len(hyps), p.z
    assert P.shape == (M, q) and np.isfinite(P).all()
    worst_u = max(float(R.T.ulps(dr[j]["eps"], R.eps_ref(SEED, j, z)).max()) for j in range(q))
    assert worst_u <= R.DRAW_ULPS, (tag, worst_u)
    hd = heads(c, p, hyps)
    rw = 0.0
    for j in range(q):
        Li, m = hd[j % S]
        rw = max(rw, float(R.judge_weights(R.weights_exact(Li, m, dr[j]["eps"]), dr[j]["weight"]).max()))
    W = np.stack([d_["weight"] for d_ in dr], axis=1)
    rp = float(R.judge_paths(W, [hyps[j % S][2] for j in range(q)], p.Z1[ROWS], P[ROWS]).max())
    print("%s: eps %.2f ulp; weights error / bar %.3f; paths error / bar %.3f" % (tag, worst_u, rw, rp))
    assert rw <= 1.0 and rp <= 1.0, (tag, rw, rp)
    check_rule(P, vals, idx)
    return rw, rp


# ---- 1. the kernel on dyadic operands: bit for bit --------------------------------------------------------------------------------
EXACT_CASES = [(1, 1, 1), (3, 2, 15), (4, 15, 16), (5, 16, 17), (16, 1, 63), (17, 2, 65), (63, 15, 1025), (64, 16, 1025), (65, 16, 1),
               (255, 1, 15), (256, 2, 16), (256, 16, 1025), (1, 16, 17), (64, 1, 63), (65, 15, 65), (255, 16, 17), (3, 16, 1),
               (16, 15, 15), (17, 16, 1025), (5, 1, 16)]


@pytest.mark.parametrize("z,q,M1", EXACT_CASES)
def test_kernel_equals_integer_arithmetic(ctx, z, q, M1):
    """Dyadic features (multiples of 2^-13), W multiples of 2^-10 with |W| <= 8, mean0 multiples of 2^-10: every product is a multiple
    of 2^-23 and -- asserted on the inputs -- sum |terms| 2^23 < 2^53, so every partial sum in any order is exact and the kernel must
    return the integer result, bit for bit."""
    rng = np.random.default_rng(1000 * z + 10 * q + M1)
    Wn, bn = B.dyadic_relu_net(B.D, z, z + q)
    Z = B.dyadic_features(B.dyadic_points(M1, B.D, M1 + z), Wn, bn)
    Wi = rng.integers(-8192, 8193, (z, q))
    mi = rng.integers(-4096, 4097, q)
    Zi = B._ints(Z, B.Z_BITS)
    assert int((np.abs(Zi) @ np.abs(Wi) + (np.abs(mi) << B.Z_BITS)[None, :]).max()) < 2 ** 53
    want = np.ldexp((Zi @ Wi + (mi << B.Z_BITS)[None, :]).astype(np.float64), -(B.Z_BITS + 10))
    got = ctx.blr_paths_compute(Z, np.ldexp(Wi.astype(np.float64), -10), np.ldexp(mi.astype(np.float64), -10))
    assert got.shape == (M1, q) and got.tobytes() == want.tobytes()


# ---- 2, 3. the kernel on general operands, and against the head's mean -------------------------------------------------------------------
@pytest.mark.parametrize("M1,z,q", [(65, 50, 5), (257, 64, 16), (33, 65, 3), (65, 200, 16), (17, 256, 1)])
def test_kernel_against_exact_rows(ctx, M1, z, q):
    rng = np.random.default_rng(M1 + z + q)
    Z, W, mean0 = rng.normal(size=(M1, z)), rng.normal(size=(z, q)), rng.normal(size=q)
    got = ctx.blr_paths_compute(Z, W, mean0)
    r = float(R.judge_paths(W, mean0, Z, got).max())
    print("paths kernel M1 %d z %d q %d: error / mean_bar %.3f" % (M1, z, q, r))
    assert r <= 1.0


@pytest.mark.parametrize("N,z", [(65, 49), (300, 200)])
def test_kernel_with_the_heads_weights_is_the_heads_mean(ctx, N, z):
    """W = m, mean0 = mean: the output and b7_blr_predict's mean are both within mean_bar of the exact rows, and of each other."""
    p = problem(N, z)
    alpha, beta, mean = B.SMALL_HYP if z <= 64 else B.WIDE_HYP
    ctx.grid_upload(p.Xg)
    ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean)
    assert ctx.blr_basis(p.W, p.b, ACT, download=True).tobytes() == p.Z1.tobytes()   # the device's features ARE the dyadic ones
    mu, _ = ctx.blr_predict()
    _, m, _ = ctx.gp_download(z)
    got = ctx.blr_paths_compute(p.Z1, m, [mean])
    hi, lo, ab = B.exact_mean_rows(m[:, 0], p.Z1, mean)
    bar = B.mean_bar(z, mean, ab)
    r_k, r_p = float((R.E.abs_errors(got[:, 0], hi, lo) / bar).max()), float((R.E.abs_errors(mu[:, 0], hi, lo) / bar).max())
    r_d = float((np.abs(got[:, 0] - mu[:, 0]) / bar).max())
    print("head's mean N %d z %d: kernel / bar %.3f, b7_blr_predict / bar %.3f, their distance / bar %.3f" % (N, z, r_k, r_p, r_d))
    assert r_k <= 1.0 and r_p <= 1.0 and r_d <= 1.0


# ---- 4. the nomination ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,q", SQ)
@pytest.mark.parametrize("N,z", FAST_NZ + GENERAL_NZ)
def test_nomination(ctx, N, z, S, q):
    """The one-launch heads (z <= 64) and the head-by-head route (z > 64), S in {1, 3}, q in {1, 5, 16}, M = 257: draws, weights,
    paths, nominees and path minima (check_call), and the evidence of every head against b7_blr_fit_x's.  MI355X: eps within 2.0 ulp;
    weights at most 0.186 of their bar (N 300, z 256, q 16), paths at most 0.030 of mean_bar.  The evidence is
    b7_blr_eval_nominate_marg's own code on the one-launch route (tests/test_gpu_blr.py holds it to the 50-digit truth) and
    b7_blr_fit_x's on the other: the comparison at 1e-9 only checks that nll_out[s] is head s's, not its accuracy."""
    p = problem(N, z)
    hyps = HYPS[:S]
    for a, b, mn in hyps:
        B.exact_head(p.Z0, p.Y, a, b, mn)                 # asserts that A and b are exact in float64
    out = nominate(ctx, p, hyps, q)
    assert out[2]["jitter"] == 0.0 and np.isfinite(out[2]["nll"]).all() and len(out[2]["nll"]) == S
    check_call(ctx, p, hyps, q, out, "N %d z %d S %d q %d" % (N, z, S, q))
    nll = [ctx.blr_fit_x(p.W, p.b, ACT, p.X, p.Y, a, b, mn, want_nll=True) for a, b, mn in hyps]
    assert np.allclose(out[2]["nll"], nll, rtol=1e-9, atol=1e-9)


# ---- 5. the head of a path ---------------------------------------------------------------------------------------------------------------
def test_path_three_of_five_uses_head_zero(ctx):
    p = problem(65, 49)
    _, _, _, _, dr = nominate(ctx, p, HYPS, 5)
    hd = heads(ctx, p, HYPS)
    ratios = [float(R.judge_weights(R.weights_exact(Li, m, dr[3]["eps"]), dr[3]["weight"]).max()) for Li, m in hd]
    print("path 3 against heads 0, 1, 2: error / bar", ratios)
    assert ratios[0] <= 1.0 and min(ratios[1:]) > 1e3


# ---- 6. bit-for-bit properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,z", [(200, 50), (15, 65)])
def test_bits_do_not_depend_on_q_on_m_or_on_the_run(ctx, N, z):
    p = problem(N, z)
    v5, i5, _, P5, d5 = nominate(ctx, p, HYPS, 5)
    v5b, i5b, _, P5b, d5b = nominate(ctx, p, HYPS, 5)
    assert P5b.tobytes() == P5.tobytes() and v5b.tobytes() == v5.tobytes() and np.array_equal(i5, i5b)
    assert all(d5[j][k].tobytes() == d5b[j][k].tobytes() for j in range(5) for k in ("eps", "weight"))
    _, _, _, P3, d3 = nominate(ctx, p, HYPS, 3)
    assert np.ascontiguousarray(P5[:, :3]).tobytes() == P3.tobytes()
    assert all(d5[j][k].tobytes() == d3[j][k].tobytes() for j in range(3) for k in ("eps", "weight"))
    _, _, _, P100, _ = nominate(ctx, p, HYPS, 5, grid=p.Xg[:100])
    assert P100.shape == (100, 5) and P100.tobytes() == np.ascontiguousarray(P5[:100]).tobytes()
    _, _, _, Pseed, _ = nominate(ctx, p, HYPS, 5, seed=SEED + 1)
    assert Pseed.tobytes() != P5.tobytes()


# ---- 7, 8. shared minimisers and NaN rows ------------------------------------------------------------------------------------------------
def test_sixteen_paths_on_twenty_rows_take_sixteen_rows(ctx):
    p = problem(65, 49)
    vals, idx, _, P, _ = nominate(ctx, p, HYPS[:1], 16, grid=p.Xg[:20])
    free = P.argmin(axis=0)
    print("unconstrained arg-mins:", free.tolist(), "nominees:", (idx - 1).tolist())
    assert len(set(free.tolist())) < 16, "sixteen paths of one head on twenty rows share minimisers"
    assert len(set(idx.tolist())) == 16 and idx.min() >= 1 and idx.max() <= 20
    check_rule(P, vals, idx)


def test_nan_rows_give_nan_paths_and_are_never_nominated(ctx):
    """A tanh network (a NaN coordinate reaches every feature of its row); rows 3 and 17 of 20 carry a NaN; q = 16."""
    d, z, N = 3, 50, 30
    Wn, bn = make_network(d, [16, z], seed=3)
    rng = np.random.default_rng(8)
    X, G = rng.random((N, d)), rng.random((20, d))
    Y = np.sin(3.0 * X.sum(1))
    G[3, 1], G[17, 0] = np.nan, np.nan
    ctx.grid_upload(G)
    vals, idx = ctx.blr_ts_nominate(Wn, bn, "Tanh", X, Y, [0.5], [100.0], [0.1], 16, seed=4)
    P = ctx.ts_last_paths()
    assert np.isnan(P[[3, 17]]).all() and np.isfinite(np.delete(P, [3, 17], axis=0)).all()
    assert not {4, 18} & set(idx.tolist()) and len(set(idx.tolist())) == 16
    check_rule(P, vals, idx)


# ---- 9. the jitter schedule ----------------------------------------------------------------------------------------------------------------
def test_failed_pivot_redoes_the_heads_and_draws_from_the_jittered_factor(ctx):
    Wn, bn, X, Y, alpha, beta = B.pivot_case()
    p = B.Problem()
    p.N, p.z, p.W, p.b, p.X, p.Y, p.Xg = 64, 8, Wn, bn, X, Y, B.dyadic_points(M, B.D, 99)
    p.Z1 = B.dyadic_features(p.Xg, Wn, bn)
    hyps = [(alpha, beta, 0.0)]
    ctx.grid_upload(p.Xg)
    vals, idx, rep = ctx.blr_ts_nominate(Wn, bn, ACT, X, Y, [alpha], [beta], [0.0], 3, seed=SEED, want_report=True)
    assert rep["jitter"] < 0.0
    out = (vals, idx, rep, ctx.ts_last_paths(), [ctx.blr_ts_last_draws(j) for j in range(3)])
    check_call(ctx, p, hyps, 3, out, "pivot case (jittered factor)")


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_case(ctx):
    import bot7_amd
    p = problem(65, 49)
    ctx.grid_upload(p.Xg[:9])
    a, b, m = zip(*HYPS)

    def refused(code, what, **kw):
        args = dict(alphas=a, betas=b, means=m, q=2)
        args.update(kw)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            ctx.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, args["alphas"], args["betas"], args["means"], args["q"])
        assert e.value.code == code and what in str(e.value), str(e.value)

    refused(-1, "blr_ts_nominate: q = 0 not in [1, 16]", q=0)
    refused(-1, "blr_ts_nominate: q = 17 not in [1, 16]", q=17)
    refused(-1, "blr_ts_nominate: q = 10 exceeds the grid's 9 rows", q=10)
    refused(-1, "blr_ts_nominate: S = 0 hyper samples", alphas=[], betas=[], means=[])
    refused(-1, "precisions must be > 0 (sample 1)", alphas=[1.0, 0.0, 1.0])
    c = bot7_amd.Context(0)
    try:
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.blr_ts_last_draws(0)
        assert e.value.code == -4 and "no successful b7_blr_ts_nominate" in str(e.value)
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            c.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, a, b, m, 2)
        assert e.value.code == -4 and "no candidate grid" in str(e.value)
    finally:
        c.close()
    ctx.grid_upload(p.Xg)
    ctx.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, a, b, m, 2)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        ctx.ts_last_draws(0)                              # the GP entry's inspection does not read this call's draws
    assert e.value.code == -4 and "b7_blr_ts_last_draws" in str(e.value)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        ctx.blr_ts_last_draws(2)
    assert e.value.code == -1 and "path 2" in str(e.value)


# ---- 11. the context afterwards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,z", [(200, 50), (15, 65)])
def test_context_after_a_nomination_behaves_as_a_fresh_one(N, z):
    import bot7_amd
    p = problem(N, z)
    alpha, beta, mean = B.SMALL_HYP
    fmin = [float(p.Y.min())]

    def usual(c):
        v, i = c.blr_eval_nominate(p.W, p.b, ACT, p.X, p.Y, alpha, beta, mean, score="ei", fmin=fmin)
        return np.float64(v).tobytes(), i, c.score_finish(1.0, download=True)[2].tobytes(), c.grid_download().tobytes()

    fresh, used = bot7_amd.Context(0), bot7_amd.Context(0)
    try:
        fresh.grid_upload(p.Xg)
        want = usual(fresh)
        used.grid_upload(p.Xg)
        a, b, m = zip(*HYPS)
        used.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, a, b, m, 5, seed=1)
        assert usual(used) == want
        P = used.ts_last_paths()                          # the paths of the last nomination survive the score call
        used.blr_ts_nominate(p.W, p.b, ACT, p.X, p.Y, a, b, m, 5, seed=1)
        assert used.ts_last_paths().tobytes() == P.tobytes()
    finally:
        fresh.close()
        used.close()


# ---- 12. the bot ---------------------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, seed=4):
    import bot7_amd
    from harness import benchmarks, bots
    grid = bot7_amd.grids.sobol({"size": 512, "dims": 3, "mins": np.zeros(3), "maxes": np.ones(3)}, context=ctx)()
    Wn, bn = make_network(3, [16, 16, 16], seed=2)
    cfg = {"bot": {"verbose": 0, "budget": 7, "nInitial": 4, "nSamples": 1, "seed": seed, "batch": 2},
           "grid": {"type": "sobol", "size": 512, "dims": 3}, "score": {"type": "thompson_sampling"}}
    model = bot7_amd.models.dngo({"network": {"weights": Wn, "biases": bn, "activation": "Tanh"}}, context=ctx)
    return bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(3)], cfg, cache={"candidates": grid, "model": model})


def test_bot_with_dngo_and_thompson_sampling(ctx):
    """harness bayesopt, dngo (3 x 16 tanh) + thompson_sampling, batch 2, M = 512: four random trials leave 8 observations, then three
    model-based trials, each with two distinct nominees by the rule on the device's own paths; the rows leave the grid; a fixed seed
    gives the same bits."""
    runs = []
    for rep in range(2):
        bot = _bot(ctx)
        inner, seen = bot._ts_nominate, []

        def traced(q, cand, inner=inner, seen=seen, bot=bot):
            assert len(bot.observed) == 8 + 2 * len(seen) and q == 2
            idx = inner(q, cand)
            P = ctx.ts_last_paths()
            assert P.shape == (512 - 8 - 2 * len(seen), 2) and [i - 1 for i in idx] == R.nominees_ref(P) and idx[0] != idx[1]
            seen.append(idx)
            return idx
        bot._ts_nominate = traced
        rows = [bot.run_trial()[0] for _ in range(7)]
        assert len(seen) == 3
        obs = bot.observed
        assert obs.shape == (14, 3) and len({r.tobytes() for r in obs}) == 14
        assert np.asarray(bot.candidates).shape == (512 - 14, 3) and np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
        runs.append((np.array(rows).tobytes(), obs.tobytes(), bot.responses.tobytes()))
    assert runs[0] == runs[1]
