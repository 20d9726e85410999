"""b7_ts_nominate_refine / b7_ts_path_grad_at on the GPU: Thompson nominees refined off the grid by descent on their own paths.
Needs an MI355X: run with -m gpu.

Reference: tests/_ts_refine_ref.py (float64 restatement and 50 digits, checked on the CPU by tests/test_ts_refine_host.py), fed with
the device's own draws (b7_ts_last_draws) and the update weights v solved on the host (_ts_ref.paths_ref).  The bar is
tests/_exact.gp_bar: 8 x numpy float64's own error against the same 50 digits + 16 eps x the sum of the absolute terms.  The ladder
is replayed from the kernel's own records with tests/_refine_ref.ladder_candidates / ladder_decide on the negated values and
gradients, bit for bit.  Every test prints its figures."""
import numpy as np
import pytest

import _exact as E
import _post_ref as PR
import _refine_ref as RR
import _ts_ref as TR
import _ts_refine_ref as R

pytestmark = pytest.mark.gpu
SEED = 4711
ITERS = 5
ETA0 = 1.0 / 16.0
SQ = [(1, 1), (3, 5), (3, 16)]
FMP = [(16, 7, 1), (256, 1037, 4), (16, 1037, 16), (256, 7, 4), (256, 1037, 16), (16, 7, 4)]     # F, M - q, starts


def cases():
    """(N, d, kernel, S, q, F, M, starts): every (N, d) x kernel x (S, q); (F, M - q, starts) rotates so that each F, each M and each
    number of starts meets every (N, d), every kernel and every (S, q)."""
    out = []
    for a, (N, d) in enumerate(TR.EXACT_ND):
        for b, kern in enumerate(TR.KERNELS):
            for c, (S, q) in enumerate(SQ):
                F, M, P = FMP[(a + 2 * b + c) % len(FMP)]
                M = M + q if M == 7 else M
                out.append((N, d, kern, S, q, F, M, min(P, M - q + 1)))
    return out


def stage(c, X, y, G, kernel):
    c.gp_set_kernel(kernel)
    c.grid_upload(G)
    c.gp_set_data(X, y)


def host_v(X, Y, hyps, kern, draws_, jitter):
    return TR.paths_ref(X, Y, X[:1], hyps, kern, draws_, jitter=jitter, want_v=True)[1]


def judge(X, hyp, kern, dr, v, xs, got_v, got_g, label):
    """error / bar of the kernel's value and gradient at the rows xs against 50 digits; the bar from numpy's own error."""
    rv, rg, sv, sg = R.value_grad64(X, hyp, kern, dr, v, xs, want_scale=True)
    tv, tg = R.value_grad_mp(X, hyp, kern, dr, v, xs)
    worst = 0.0
    for p in range(len(xs)):
        bar_v = E.gp_bar(RR.err_vs_truth(rv[p:p + 1], tv[p:p + 1]), sv[p])
        bar_g = E.gp_bar(RR.err_vs_truth(rg[p], tg[p]), sg[p])
        ev, eg = RR.err_vs_truth(got_v[p:p + 1], tv[p:p + 1]), RR.err_vs_truth(got_g[p], tg[p])
        worst = max(worst, ev / bar_v, eg / bar_g)
    print("%s: worst error / bar %.3g over %d points" % (label, worst, len(xs)))
    return worst


def replay(tr, lo, hi, iters):
    """A start's records against the ladder's pure functions, on the kernel's own numbers.  -> whether it moved."""
    assert tr["rung"][0] == -1 and np.isnan(tr["cand"][0]).all() and tr["eta"][0] == ETA0
    moved = False
    for t in range(1, iters + 1):
        x, g, v, eta, st = tr["x"][t - 1], tr["grad"][t - 1], tr["val"][t - 1], tr["eta"][t], int(tr["status"][t - 1])
        ran = not np.isnan(tr["cand"][t]).all()
        cand = None if st & (RR.NOT_RUN | RR.CONVERGED) else RR.ladder_candidates(x, -g, eta, lo, hi)
        if cand is None:
            assert not ran and tr["rung"][t] == -1 and tr["x"][t].tobytes() == x.tobytes() and tr["val"][t] == v
            if not st & (RR.NOT_RUN | RR.CONVERGED):
                assert int(tr["status"][t]) & RR.FLAT
            continue
        k, nv, neta, conv = RR.ladder_decide(-v, eta, -tr["cand"][t])
        assert int(tr["rung"][t]) == k and tr["val"][t] == -nv, (t, k, tr["rung"][t])
        assert tr["x"][t].tobytes() == (cand[k] if k >= 0 else x).tobytes(), "the point is the rung's, bit for bit"
        if t < iters:
            assert tr["eta"][t + 1] == neta
        assert bool(int(tr["status"][t]) & RR.CONVERGED) == bool(conv or st & RR.CONVERGED)
        moved = moved or k >= 0
        assert bool(int(tr["status"][t]) & RR.MOVED) == moved
    return moved


@pytest.mark.parametrize("N,d,kern,S,q,F,M,P", cases())
def test_refinement_case(ctx, N, d, kern, S, q, F, M, P):
    """Checks 1-6 of one shape on one staging: the nomination's outputs and kept paths equal b7_ts_nominate's bit for bit; the
    starts equal the stable-argsort restatement; the same call twice gives the same bits; every record replays through the ladder's
    pure functions bit for bit; values never increase, points stay inside the box, the winner rule holds; the kernel's value and
    gradient at grid rows, traced points and results are within the bar of 50 digits, and its values at grid rows agree with the
    kept paths; on the (64, 9) and (65, 33) problems the float64 reference moves at least half of the starts, and the library's
    winner is strictly below its nominee's value.  MI355X: value and gradient worst 0.65 of the bar (typically 0.1 - 0.2), against
    the kept paths worst 0.022 of theirs; every start of every case moved, the reference's too."""
    X, Y, hyps, G, rows = TR.case_problem(N, d, S, M)
    lo, hi = np.zeros(d), np.ones(d)
    try:
        stage(ctx, X, Y, G, kern)
        pm0, idx0, rep0 = ctx.ts_nominate(hyps, q, n_features=F, seed=SEED, want_report=True)
        paths0 = ctx.ts_last_paths()
        ctx.ts_refine_trace_enable(True)
        outs = []
        for _ in range(2):
            o = ctx.ts_nominate_refine(hyps, q, n_features=F, seed=SEED, starts=P, iters=ITERS, eta0=ETA0, want_report=True)
            outs.append((o, ctx.ts_last_paths(), [ctx.ts_refine_last(j) for j in range(q)],
                         [[ctx.ts_refine_trace(j, p) for p in range(P)] for j in range(q)]))
        draws_ = [ctx.ts_last_draws(j) for j in range(q)]
        jrows = rows[:3]
        gv, gg = ctx.ts_path_grad_at(G[jrows])
        paths_after = ctx.ts_last_paths()
    finally:
        ctx.ts_refine_trace_enable(False)
        ctx.gp_set_kernel("ardse")
    (pm, idx, x, val, start, rep), paths1, last, traces = outs[0]
    # 2. the nomination half is b7_ts_nominate's
    assert pm.tobytes() == pm0.tobytes() and idx.tobytes() == idx0.tobytes() and paths1.tobytes() == paths0.tobytes()
    assert rep["jitter"].tobytes() == rep0["jitter"].tobytes() and rep["info"].tobytes() == rep0["info"].tobytes()
    assert paths_after.tobytes() == paths0.tobytes(), "b7_ts_path_grad_at disturbs nothing"
    # 5. the same call twice
    (o2, _, last2, traces2) = outs[1][0], None, outs[1][2], outs[1][3]
    for a, b in zip(o2[:5], (pm, idx, x, val, start)):
        assert a.tobytes() == b.tobytes()
    for j in range(q):
        for key in last[j]:
            assert last[j][key].tobytes() == last2[j][key].tobytes()
        for p in range(P):
            for key in traces[j][p]:
                assert traces[j][p][key].tobytes() == traces2[j][p][key].tobytes()
    # the starts
    want = R.starts_ref(paths0, idx0 - 1, P)
    for j in range(q):
        assert (last[j]["start_idx1"] - 1).tolist() == want[j].tolist(), (j, last[j]["start_idx1"], want[j])
    vs = host_v(X, Y, hyps, kern, draws_, rep["jitter"])
    vg = lambda j: (lambda xs: R.value_grad64(X, hyps[j % S], kern, draws_[j], vs[j], xs))
    # 6. the inputs make something move, by the reference alone
    if (N, d) in ((64, 9), (65, 33)):
        n_moved = n_all = 0
        for j in range(q):
            ref = R.descend(vg(j), G[want[j]], ITERS, ETA0, lo, hi)
            n_moved += int(np.count_nonzero(ref["status"] & RR.MOVED))
            n_all += P
        print("reference: %d of %d starts moved" % (n_moved, n_all))
        assert 2 * n_moved >= n_all
        for j in range(q):
            assert val[j] < traces[j][0]["val"][0], (j, val[j], traces[j][0]["val"][0])
    # 3. and 4. the records
    n_moved = 0
    for j in range(q):
        for p in range(P):
            tr = traces[j][p]
            assert tr["x"][0].tobytes() == G[want[j][p]].tobytes(), "iteration 0 is the start itself, unclipped"
            n_moved += replay(tr, lo, hi, ITERS)
            assert (np.diff(tr["val"]) <= 0.0).all(), "a start's path value never increases"
            assert (tr["x"] >= lo).all() and (tr["x"] <= hi).all()
            assert tr["x"][-1].tobytes() == last[j]["x"][p].tobytes() and tr["val"][-1] == last[j]["val"][p]
            assert int(tr["status"][-1]) == int(last[j]["status"][p])
        lj = last[j]
        win = 0
        if (lj["status"] & RR.MOVED).any():
            ok = [p for p in range(P) if not lj["status"][p] & RR.NOT_RUN and np.isfinite(lj["val"][p])]
            win = min(ok, key=lambda p: (lj["val"][p], p)) if ok else 0
        assert x[j].tobytes() == lj["x"][win].tobytes() and val[j] == lj["val"][win] and start[j] == lj["start_idx1"][win]
    print("device: %d of %d starts moved" % (n_moved, q * P))
    # 1. values and gradients against 50 digits: grid rows, and per judged path one traced point and the result
    worst = 0.0
    for j in sorted({0, q // 2, q - 1}):
        s = j % S
        worst = max(worst, judge(X, hyps[s], kern, draws_[j], vs[j], G[jrows], gv[:, j], gg[:, j], "path %d grid rows" % j))
        tr = traces[j][P - 1]
        pts = np.stack([tr["x"][1], tr["x"][-1]])
        worst = max(worst, judge(X, hyps[s], kern, draws_[j], vs[j], pts, tr["val"][[1, -1]], tr["grad"][[1, -1]], "path %d traced" % j))
    assert worst <= 1.0
    # ... and the kept paths at the same rows, at the bar tests/test_gpu_ts_exact.py holds them to
    al = TR.host_alphas(X, Y, hyps, kern, draws_, rep["jitter"])
    ref = TR.paths_exact(X, G[jrows], hyps, kern, draws_, al)
    dev = float(np.max(np.abs(gv - paths0[jrows]) / ref.bar))
    print("b7_ts_path_grad_at against the kept paths: worst difference / bar %.3g" % dev)
    assert dev <= 1.0


def small_problem(kern=PR.SE, N=64, d=9, S=3, M=1037):
    X, Y, hyps, G, _ = TR.case_problem(N, d, S, M)
    return X, Y, hyps, G, kern


def test_iters_zero_returns_the_grid_nominees(ctx):
    X, Y, hyps, G, kern = small_problem()
    stage(ctx, X, Y, G, kern)
    for P in (1, 4, 16):
        pm, idx, x, val, start = ctx.ts_nominate_refine(hyps, 5, n_features=16, seed=SEED, starts=P, iters=0)
        assert x.tobytes() == G[idx - 1].tobytes() and start.tolist() == idx.tolist()
        assert all(ctx.ts_refine_last(j)["val"][0] == val[j] for j in range(5))
        gv, _ = ctx.ts_path_grad_at(G[idx - 1])
        assert [gv[j, j] for j in range(5)] == val.tolist(), "iteration 0's value is the kernel's own at the row"


@pytest.mark.parametrize("kern", TR.KERNELS)
def test_independence_of_starts_and_iterations(ctx, kern):
    """Bit for bit: start rank r of path j is the same for starts in {r + 1, 16}; the first T1 iterations of a trace are the same
    for iters = T1 and T2 > T1; a path of a q = 5 call is the same path of a q = 16 call when its starts are (q alone changes the
    rows barred from the starts, so rank 0, the nominee of path 0, is compared)."""
    X, Y, hyps, G, _ = small_problem(kern, 65, 33)
    try:
        stage(ctx, X, Y, G, kern)
        ctx.ts_refine_trace_enable(True)
        run = lambda q, P, T: (ctx.ts_nominate_refine(hyps, q, n_features=256, seed=SEED, starts=P, iters=T, eta0=ETA0),
                               [[ctx.ts_refine_trace(j, p) for p in range(P)] for j in range(q)])
        _, t16 = run(5, 16, 6)
        for r in (0, 3, 8):
            _, tr = run(5, r + 1, 6)
            for j in range(5):
                for key in tr[j][r]:
                    assert tr[j][r][key].tobytes() == t16[j][r][key].tobytes(), (r, j, key)
        _, t3 = run(5, 16, 3)
        for j in range(5):
            for p in range(16):
                for key in ("x", "val", "grad", "eta", "cand", "rung", "status"):
                    assert t3[j][p][key][:4].tobytes() == t16[j][p][key][:4].tobytes(), (j, p, key)
        _, tq = run(16, 1, 6)
        for key in tq[0][0]:
            assert tq[0][0][key].tobytes() == t16[0][0][key].tobytes()
    finally:
        ctx.ts_refine_trace_enable(False)
        ctx.gp_set_kernel("ardse")


def test_box_holds_the_points(ctx):
    """A box that is not the unit cube: every traced point of every moving start lies inside [lo, hi]; the start itself is not clipped."""
    X, Y, hyps, G, kern = small_problem()
    lo, hi = np.full(9, 0.25), np.full(9, 0.75)
    Gb = lo + G * (hi - lo)
    try:
        stage(ctx, X, Y, Gb, kern)
        ctx.ts_refine_trace_enable(True)
        pm, idx, x, val, start = ctx.ts_nominate_refine(hyps, 5, n_features=256, seed=SEED, starts=4, iters=8, eta0=0.5, lo=lo, hi=hi)
        moved = 0
        for j in range(5):
            for p in range(4):
                tr = ctx.ts_refine_trace(j, p)
                assert (tr["x"] >= lo).all() and (tr["x"] <= hi).all()
                moved += int(int(tr["status"][-1]) & RR.MOVED != 0)
        assert moved > 0 and (x >= lo).all() and (x <= hi).all()
    finally:
        ctx.ts_refine_trace_enable(False)


def test_refusals(ctx):
    """Every refusal a single GPU can reach, by code and by name."""
    import bot7_amd
    X, Y, hyps, G, kern = small_problem(M=10)

    def refused(call, code, word):
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            call()
        assert e.value.code == code and word in str(e.value), (code, word, str(e.value))

    def nominate(**kw):
        args = dict(q=5, n_features=16, seed=1, starts=4, iters=2)
        args.update(kw)
        return lambda: ctx.ts_nominate_refine(hyps, **args)

    from conftest import make_network
    fresh = bot7_amd.Context(0)
    try:
        refused(lambda: fresh.ts_path_grad_at(G[:2]), -4, "no successful b7_ts_nominate")
        refused(lambda: fresh.ts_refine_last(0), -4, "no successful b7_ts_nominate_refine")
        fresh.grid_upload(G)                           # the DNGO head's paths
        Wn, bn = make_network(9, [16, 8], seed=3)
        fresh.blr_ts_nominate(Wn, bn, "Tanh", X, Y[:, 0], [0.5], [100.0], [0.1], 4, seed=4)
        refused(lambda: fresh.ts_path_grad_at(G[:2]), -5, "DNGO")
    finally:
        fresh.close()
    g = bot7_amd.Group([0, 0])                         # a group member
    try:
        g.grid_upload(G)
        g.gp_set_data(X, Y)
        refused(lambda: g.members[0].ts_nominate_refine(hyps, 2, n_features=16, seed=1, starts=2, iters=1), -4, "group")
        refused(lambda: g.members[1].ts_path_grad_at(G[:2]), -4, "group")
    finally:
        g.close()
    stage(ctx, X, Y, G, kern)
    ctx.ts_nominate_refine(hyps, 5, n_features=16, seed=1, starts=6, iters=1)      # 6 = M - q + 1 is the most
    assert (ctx.ts_refine_last(4)["start_idx1"] >= 1).all()
    refused(lambda: ctx.ts_refine_last(5), -1, "path 5")
    refused(nominate(starts=7), -1, "M - q + 1")
    refused(nominate(starts=0), -1, "starts")
    refused(nominate(starts=17), -1, "starts")
    refused(nominate(iters=-1), -1, "iters")
    refused(nominate(iters=257), -1, "iters")
    refused(nominate(eta0=0.0), -1, "eta0")
    refused(nominate(eta0=1.5), -1, "eta0")
    refused(nominate(lo=np.zeros(9)), -1, "lo and hi")
    refused(nominate(lo=np.ones(9), hi=np.ones(9)), -1, "box column")
    refused(nominate(q=17), -1, "q = 17")
    refused(nominate(n_features=24), -1, "F = 24")
    refused(lambda: ctx.ts_refine_last(0), -4, "no successful b7_ts_nominate_refine")       # a refused call leaves no result
    ctx.ts_refine_trace_enable(False)
    refused(lambda: ctx.ts_refine_trace(0, 0), -4, "no traced")
    ctx.ts_nominate(hyps, 5, n_features=16, seed=1)
    ctx.ts_path_grad_at(G[:2])                                                     # a plain nomination's paths serve
    ctx.grid_upload(G[:9])
    refused(lambda: ctx.ts_path_grad_at(G[:2]), -4, "stale")
    Y2 = np.concatenate([Y, Y], axis=1)
    ctx.gp_set_data(X, Y2)
    refused(nominate(starts=2), -5, "response columns")
    ctx.gp_set_data(X, Y)


# ---- the harness bot end to end ---------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _run_bot(ctx, tr):
    import bot7_amd
    from harness import benchmarks, bots
    D, MC = 6, 512
    cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 4, "nSamples": 2, "seed": 3, "batch": 4},
           "grid": {"type": "sobol", "size": MC, "dims": D},
           "score": {"type": "thompson_sampling", "nFeatures": 64, "refine": {"starts": 4, "iters": 4}}}
    cache = {"model": bot7_amd.models.gp_regressor({}, context=ctx)}
    if tr:
        cfg["bot"]["trust_region"] = {"length_init": 0.4}
    else:
        cache["candidates"] = bot7_amd.grids.sobol({"size": MC, "dims": D, "mins": np.zeros(D), "maxes": np.ones(D)}, context=ctx)()
    bot = bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(D)], cfg, cache=cache)
    off_grid = 0
    for t in range(12):
        before = None if tr else np.asarray(bot.candidates).copy()
        n = 0 if bot.responses is None else len(bot.responses)
        x, y = bot.run_trial()
        bot.update_best(x, y)
        new = bot.observed[n:]
        assert new.shape == (4, D) and len(bot.responses) == n + 4 and np.all(new >= 0.0) and np.all(new <= 1.0)
        if t < 4:
            continue
        if tr:
            rec = bot.tr_trace[-1]
            assert rec["kind"] == "model" and len(set(rec["index"])) == 4
            assert np.all(new >= rec["lo"]) and np.all(new <= rec["hi"]), "the observed points lie inside the trial's trust region"
            assert np.all(rec["grid_rows"] >= rec["lo"]) and np.all(rec["grid_rows"] <= rec["hi"])
            off_grid += int(np.count_nonzero(np.any(new != rec["grid_rows"], axis=1)))
        else:
            last = bot.last_ts_refine
            idx = np.asarray(last["index"])
            assert len(set(idx.tolist())) == 4 and np.array_equal(new, last["x"]), "the bot observes the refined points"
            assert np.array_equal(np.asarray(bot.candidates), np.delete(before, idx - 1, axis=0)), "the stolen rows are the grid nominees"
            assert np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
            off_grid += int(np.count_nonzero(np.any(new != before[idx - 1], axis=1)))
    return bot.observed.copy(), bot.responses.copy(), off_grid


@pytest.mark.parametrize("tr", [False, True])
def test_the_bot_end_to_end(ctx, tr):
    """harness bayesopt on ackley, d = 6, 512 Sobol candidates, nInitial 4, 12 trials of batch 4, config.score.refine = {starts 4,
    iters 4}, with and without a trust region: the observed points lie inside the box (the trial's trust region), at least one is
    off the grid, the stolen rows are the grid nominees, and a second run under the same seed gives the same bits."""
    X, Y, off = _run_bot(ctx, tr)
    X2, Y2, _ = _run_bot(ctx, tr)
    print("trust region %s: %d of 32 model-based points are off the grid, best %.4f" % (tr, off, Y.min()))
    assert off >= 1 and X.tobytes() == X2.tobytes() and Y.tobytes() == Y2.tobytes()
