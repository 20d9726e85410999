"""b7_ts_paths / b7_ts_hvi_nominate / b7_ts_hvi3_nominate / b7_hvi_compute on the GPU: multi-objective Thompson sampling.

The two score kernels are held to their numpy float64 restatement (tests/_ts_hvi_ref.py, itself held to exact rational arithmetic by
tests/test_ts_hvi_host.py) BIT FOR BIT: the formulas are differences, maxima, products and a running sum, one rounded operation per
operator, contraction off.  The paths of b7_ts_paths are b7_ts_nominate's bit for bit.  The nominations are replayed on the host from
the downloaded paths by the restated pick rule and must agree exactly: picks, values and path values.  Shape of the path tests:
N = 24, d = 3, M = 1000 (four workgroups, the last one ragged), F = 64."""
import os

import numpy as np
import pytest

import _ehvi3_ref as R3
import _ehvi_ref as R2
import _ts_hvi_ref as R

pytestmark = pytest.mark.gpu
N, D, M, F = 24, 3, 1000, 64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def refused(code, word, fn):
    import bot7_amd
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


# ---- 1. b7_hvi_compute equals the restatement bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("P", [0, 1, 2, 33, 256])
def test_hvi2_compute_equals_the_restatement(ctx, P):
    """M1 = 257: two workgroups, the second one a single row.  The special rows are the host test's."""
    front = R2.make_front(P)
    Y, n = R.special_rows(front, R2.REF, 257)
    got = ctx.hvi_compute(Y, front, R2.REF)
    want = R.hvi2_numpy(Y, front, R2.REF)
    assert got.shape == (257,) and np.array_equal(np.isnan(got), ~np.isfinite(Y).all(axis=1))
    print("hvi2, P = %d: %d rows differ; %d NaN rows, %d zero rows" % (P, int((got.view(np.int64) != want.view(np.int64)).sum()),
                                                                       int(np.isnan(got).sum()), int((got == 0.0).sum())))
    assert bits(got) == bits(want)


@pytest.mark.parametrize("P", [0, 1, 2, 24, 256])
def test_hvi3_compute_equals_the_restatement(ctx, P):
    from bot7_amd import _lib
    front = R3.make_front3(P)
    Y, n = R.special_rows(front, R3.REF3, 257)
    got = ctx.hvi_compute(Y, front, R3.REF3)
    boxes = _lib.nondominated_boxes3(front, R3.REF3)
    assert np.array_equal(boxes, R3.boxes3(front, R3.REF3))
    want = R.hvi3_numpy(Y, front, R3.REF3, boxes)
    assert got.shape == (257,) and np.array_equal(np.isnan(got), ~np.isfinite(Y).all(axis=1))
    print("hvi3, P = %d, B = %d: %d rows differ" % (P, len(boxes), int((got.view(np.int64) != want.view(np.int64)).sum())))
    assert bits(got) == bits(want)


def test_hvi_compute_refusals(ctx):
    front = R2.make_front(3)
    Y = np.zeros((4, 2))
    refused(-1, "not sorted", lambda: ctx.hvi_compute(Y, front[::-1], R2.REF))
    refused(-1, "not finite", lambda: ctx.hvi_compute(Y, front, [np.nan, 1.0]))
    refused(-1, "not canonical", lambda: ctx.hvi_compute(np.zeros((4, 3)), R3.make_front3(3)[::-1], R3.REF3))
    assert ctx.hvi_compute(np.zeros((0, 2)), front, R2.REF).shape == (0,)
    assert bits(ctx.hvi_compute(Y, front, R2.REF)) == bits(R.hvi2_numpy(Y, front, R2.REF))      # the call after a refusal works


# ---- the problem of the path tests ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prob():
    from harness import benchmarks as B
    rng = np.random.default_rng(5)
    X, Xc = rng.random((N, D)), rng.random((M, D))
    Y = B.three_spheres(X)
    hyps = []
    for col in range(3):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(D, 0.4 + 0.2 * s + 0.1 * col), "amp": amp * (1.0 + 0.3 * s), "noise": 1e-4 * amp,
                      "mean": float(np.mean(Y[:, col])) + 0.02 * s} for s in range(3)])
    return X, Y, Xc, hyps


@pytest.fixture(scope="module")
def ctx23():
    import bot7_amd
    cs = [bot7_amd.Context(0), bot7_amd.Context(0)]
    yield cs
    for c in cs:
        c.close()


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


SEEDS = (101, 202, 303)


def keep_paths(cs, prob, q, S=3):
    """Stage objective k's column on cs[k] and keep q paths there -> the m downloaded path matrices."""
    X, Y, Xc, hyps = prob
    out = []
    for k, c in enumerate(cs):
        stage(c, X, Y[:, k:k + 1], Xc)
        c.ts_paths(hyps[k][:S], q, n_features=F, seed=SEEDS[k])
        out.append(c.ts_last_paths())
    return out


def front_of(m, P):
    """A canonical front of P points inside the box of ref = 0.9 * 1 that leaves the paths room to improve on it: two objectives on
    the anti-diagonal, three on the plane y1 + y2 + y3 = 1.25 (mutually non-dominated, put in order by the restated b7_pareto_front3)."""
    ref = np.full(m, 0.9)
    if m == 2:
        a = np.linspace(0.15, 0.8, P)
        front = np.stack([a, a[::-1]], axis=1).reshape(-1, 2)
    else:
        ab = np.random.default_rng(9).uniform(0.2, 0.6, (P, 2))
        front = R.canonical(np.concatenate([ab, 1.25 - ab.sum(axis=1, keepdims=True)], axis=1), ref)
    assert len(front) == P
    return front, ref


# ---- 2. b7_ts_paths against b7_ts_nominate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("S,q", [(1, 1), (3, 5), (3, 16)])
def test_ts_paths_are_ts_nominates_paths(ctx, prob, kernel, S, q):
    X, Y, Xc, hyps = prob
    stage(ctx, X, Y[:, :1], Xc, kernel)
    vals, idx, rep = ctx.ts_nominate(hyps[0][:S], q, n_features=F, seed=77, want_report=True)
    want, draws = ctx.ts_last_paths(), ctx.ts_last_draws(q - 1)
    rep2 = ctx.ts_paths(hyps[0][:S], q, n_features=F, seed=77, want_report=True)
    got = ctx.ts_last_paths()
    assert got.shape == (M, q) and bits(got) == bits(want)
    assert np.array_equal(rep["jitter"], rep2["jitter"]) and np.array_equal(rep["info"], rep2["info"])
    d2 = ctx.ts_last_draws(q - 1)
    assert all(bits(draws[k]) == bits(d2[k]) for k in draws)
    # b7_ts_nominate after a b7_ts_paths gives its usual bits
    v2, i2 = ctx.ts_nominate(hyps[0][:S], q, n_features=F, seed=77)
    assert bits(v2) == bits(vals) and np.array_equal(i2, idx) and bits(ctx.ts_last_paths()) == bits(want)
    ctx.gp_set_kernel("ardse")


# ---- 3. the nominations against the host replay -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def strided():
    """A context of the diagnostic build whose picks read column j of [M][q] at stride q (the shipped default reads a [q][M] copy)."""
    import bot7_amd
    os.environ["B7_TS_HVI_LAYOUT"] = "0"
    try:
        c = bot7_amd.Context(0, lib="diag")
    finally:
        del os.environ["B7_TS_HVI_LAYOUT"]
    yield c
    c.close()


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("q", [1, 5, 16])
@pytest.mark.parametrize("P", [0, 7])
def test_nomination_equals_the_replay(ctx, ctx23, prob, m, q, P):
    cs = ([ctx] + ctx23)[:m]
    paths = keep_paths(cs, prob, q)
    front, ref = front_of(m, P)
    others = cs[1] if m == 2 else cs[1:]
    hvi, idx, y = ctx.ts_hvi_nominate(others, front, ref)
    hv, rows, ys, fb = R.replay(paths, front, ref)
    print("m = %d, q = %d, P = %d: picks %s, hvi %s, %d by the fallback" % (m, q, P, idx.tolist(), ["%.3g" % v for v in hvi], int(fb.sum())))
    assert np.array_equal(idx, rows + 1) and bits(hvi) == bits(hv) and bits(y) == bits(ys)
    assert len(set(idx.tolist())) == q and idx.min() >= 1 and idx.max() <= M
    assert not fb[0] and hvi[0] > 0.0                       # the room under ref: the first path improves the hypervolume
    # the same call twice gives the same bits, and the kept paths are untouched
    h2, i2, y2 = ctx.ts_hvi_nominate(others, front, ref)
    assert bits(h2) == bits(hvi) and np.array_equal(i2, idx) and bits(y2) == bits(y)
    assert all(bits(c.ts_last_paths()) == bits(p) for c, p in zip(cs, paths))
    if q == 5:
        # the first three picks are a q = 3 call's.  The draws depend on (seed, j) alone, but a hyper sample's paths are fitted as the
        # columns of ONE multi-column fit, so a path's last bits depend on how many paths share its sample: the picks are held
        # equal, the values to the posterior-mean bar of tests/test_gpu_ts.py (1e-5 relative to max(1, |value|))
        keep_paths(cs, prob, 3)
        h3, i3, y3 = ctx.ts_hvi_nominate(others, front, ref)
        assert np.array_equal(i3, idx[:3])
        assert np.abs(y3 - y[:3]).max() <= 1e-5 * max(1.0, float(np.abs(y[:3]).max())) and np.abs(h3 - hvi[:3]).max() <= 1e-4


@pytest.mark.parametrize("m", [2, 3])
def test_both_layouts_give_the_same_bits(ctx, strided, prob, m):
    """The shipped default against the strided reads (diagnostic build), on one context per layout holding all the objectives in
    turn is not possible -- a context keeps one set of paths -- so each layout gets the same paths on coinciding contexts."""
    import bot7_amd
    X, Y, Xc, hyps = prob
    front, ref = front_of(m, 7)
    extra = [bot7_amd.Context(0, lib="diag") for _ in range(m - 1)]
    try:
        out = []
        for cs in (([ctx] + [bot7_amd.Context(0) for _ in range(m - 1)]), [strided] + extra):
            try:
                paths = keep_paths(cs, prob, 16)
                out.append((cs[0].ts_hvi_nominate(cs[1] if m == 2 else cs[1:], front, ref), paths))
            finally:
                for c in cs[1:]:
                    if c not in extra:
                        c.close()
        (a, pa), (b, pb) = out
        assert all(bits(x) == bits(y) for x, y in zip(pa, pb))
        assert bits(a[0]) == bits(b[0]) and np.array_equal(a[1], b[1]) and bits(a[2]) == bits(b[2])
    finally:
        for c in extra:
            c.close()


@pytest.mark.parametrize("m", [2, 3])
def test_fallback_on_every_pick(ctx, ctx23, prob, m):
    """A reference point below every path value: nothing can improve the hypervolume, every pick is the first minimum of objective
    1 + (j mod m)'s path j over the rows not taken, and every hvi is 0."""
    cs = ([ctx] + ctx23)[:m]
    paths = keep_paths(cs, prob, 5)
    ref = np.full(m, min(float(p.min()) for p in paths) - 1.0)
    hvi, idx, y = ctx.ts_hvi_nominate(cs[1] if m == 2 else cs[1:], np.zeros((0, m)), ref)
    hv, rows, ys, fb = R.replay(paths, np.zeros((0, m)), ref)
    assert fb.all() and (hvi == 0.0).all() and np.array_equal(idx, rows + 1) and bits(y) == bits(ys)
    taken = []
    for j in range(5):
        assert idx[j] - 1 == R.ts_argmin(paths[j % m][:, j], taken)
        taken.append(int(idx[j] - 1))


@pytest.mark.parametrize("m", [2, 3])
def test_planted_nan_rows_never_win(ctx, prob, m):
    """NaN rows planted in a path matrix: b7_hvi_compute scores them NaN beside the other rows' usual bits, and the replay with the
    DEVICE's scores (b7_hvi_compute as the replay's score) never picks them and equals the replay with the restated score."""
    rng = np.random.default_rng(3)
    paths = [rng.uniform(0.0, 1.0, (300, 4)) for _ in range(m)]
    best = int(np.argmin(sum(p[:, 0] for p in paths)))      # a row that would win path 0
    bad = [best, 17, 299]
    paths[0][bad, :] = np.nan
    paths[m - 1][40, 2] = np.inf
    front, ref = front_of(m, 7)
    dev = lambda Yj, wf, rf: ctx.hvi_compute(Yj, wf, rf)
    hv, rows, ys, fb = R.replay(paths, front, ref, score=dev)
    hv2, rows2, ys2, fb2 = R.replay(paths, front, ref)
    assert np.array_equal(rows, rows2) and bits(hv) == bits(hv2) and not set(rows.tolist()) & set(bad + [40])
    s = ctx.hvi_compute(np.stack([p[:, 2] for p in paths], axis=1), front, ref)
    assert np.isnan(s[bad]).all() and np.isnan(s[40]) and np.isfinite(np.delete(s, bad + [40])).all()


# ---- 4. every error, by code and by name --------------------------------------------------------------------------------------------------
def test_state_and_refusals(ctx, ctx23, prob):
    import bot7_amd
    from conftest import make_network
    X, Y, Xc, hyps = prob
    c2, c3 = ctx23
    fresh = [bot7_amd.Context(0) for _ in range(3)]
    try:
        f2, r2 = front_of(2, 7)
        f3, r3 = front_of(3, 7)
        a, b, c = fresh
        for k, cc in enumerate(fresh):
            stage(cc, X, Y[:, k:k + 1], Xc)
        # no kept paths, on each side in turn
        refused(-4, "no kept paths of the first objective", lambda: a.ts_hvi_nominate(b, f2, r2))
        a.ts_paths(hyps[0], 4, n_features=F, seed=1)
        refused(-4, "no kept paths of the second objective", lambda: a.ts_hvi_nominate(b, f2, r2))
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        refused(-4, "no kept paths of the third objective", lambda: a.ts_hvi_nominate((b, c), f3, r3))
        c.ts_paths(hyps[2], 4, n_features=F, seed=3)
        good2, good3 = a.ts_hvi_nominate(b, f2, r2), a.ts_hvi_nominate((b, c), f3, r3)
        # the front, the reference point, NULL
        refused(-1, "not sorted", lambda: a.ts_hvi_nominate(b, f2[::-1], r2))
        refused(-1, "not finite", lambda: a.ts_hvi_nominate(b, f2, [np.nan, 1.0]))
        refused(-1, "strictly inside", lambda: a.ts_hvi_nominate((b, c), np.array([[0.1, 0.95, 0.1]]), r3))
        L, h, i8 = a._L, np.zeros(4), np.zeros(4, dtype=np.int64)
        ptr = lambda x: x.ctypes.data
        err = lambda: L.b7_last_error(a._h).decode()
        assert L.b7_ts_hvi_nominate(a._h, None, ptr(f2), 7, ptr(r2), ptr(h), ptr(i8), None) == -1 and "second objective's context is NULL" in err()
        assert L.b7_ts_hvi_nominate(a._h, b._h, ptr(f2), 7, ptr(r2), None, ptr(i8), None) == -1 and "NULL argument" in err()
        assert L.b7_ts_hvi3_nominate(a._h, b._h, None, ptr(f3), len(f3), ptr(r3), ptr(h), ptr(i8), None) == -1 and "third objective's context is NULL" in err()
        assert L.b7_ts_hvi_nominate(None, b._h, ptr(f2), 7, ptr(r2), ptr(h), ptr(i8), None) == -1
        # P + q - 1 beyond the cap: the working front can grow by a point per pick
        big2, big3 = R2.make_front(254), R3.make_front3(254)
        refused(-1, "P + q - 1 = 257 exceeds 256", lambda: a.ts_hvi_nominate(b, big2, R2.REF))
        refused(-1, "P + q - 1 = 257 exceeds 256", lambda: a.ts_hvi_nominate((b, c), big3, R3.REF3))
        a.ts_hvi_nominate(b, big2[:253], R2.REF)
        # the call after a refusal works, with the usual bits
        again = a.ts_hvi_nominate(b, f2, r2)
        assert all(bits(x) == bits(y) for x, y in zip(again, good2))
        # q differs; M differs
        b.ts_paths(hyps[1], 3, n_features=F, seed=2)
        refused(-1, "second objective keeps q = 3 paths, this one 4", lambda: a.ts_hvi_nominate(b, f2, r2))
        b.grid_upload(Xc[:40])
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        refused(-1, "second objective's grid has M = 40 rows, this one 1000", lambda: a.ts_hvi_nominate(b, f2, r2))
        b.grid_upload(Xc)
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        assert all(bits(x) == bits(y) for x, y in zip(a.ts_hvi_nominate(b, f2, r2), good2))
        # stale paths: the grid changed, the data changed; b7_ts_last_paths keeps serving them
        kept = b.ts_last_paths()
        b.grid_remove(3)
        refused(-4, "kept paths of the second objective are stale", lambda: a.ts_hvi_nominate(b, f2, r2))
        assert bits(b.ts_last_paths()) == bits(kept)
        a.gp_set_data(X[:20], Y[:20, :1])
        refused(-4, "kept paths of the first objective are stale", lambda: a.ts_hvi_nominate(a, f2, r2))
        a.gp_set_data(X, Y[:, :1])
        a.ts_paths(hyps[0], 4, n_features=F, seed=1)
        assert all(bits(x) == bits(y) for x, y in zip(a.ts_hvi_nominate((c, c), f3, r3), a.ts_hvi_nominate((c, c), f3, r3)))
        # a b7_ts_nominate's paths serve as well; the DNGO head's do not
        c.ts_nominate(hyps[2], 4, n_features=F, seed=3)
        assert all(bits(x) == bits(y) for x, y in zip(a.ts_hvi_nominate((c, c), f3, r3), a.ts_hvi_nominate((c, c), f3, r3)))
        Wn, bn = make_network(D, [16, 8], seed=3)
        c.blr_ts_nominate(Wn, bn, "Tanh", X, Y[:, 2], [0.5], [100.0], [0.1], 4, seed=4)
        refused(-5, "b7_blr_ts_nominate", lambda: a.ts_hvi_nominate(c, f2, r2))
        # a group member
        g = bot7_amd.Group([0, 0])
        try:
            g.grid_upload(Xc)
            g.gp_set_data(X, Y[:, :1])
            refused(-4, "group", lambda: a.ts_hvi_nominate(g.members[0], f2, r2))
            refused(-4, "group", lambda: g.members[1].ts_hvi_nominate(a, f2, r2))
        finally:
            g.close()
        # b7_ts_paths' own checks are b7_ts_nominate's, under its own name
        refused(-1, "ts_paths: q = 0 not in [1, 16]", lambda: a.ts_paths(hyps[0], 0, n_features=F))
        refused(-1, "ts_paths: F = 24 features", lambda: a.ts_paths(hyps[0], 4, n_features=24))
    finally:
        for cc in fresh:
            cc.close()


# ---- 5. the harness bot end to end -------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name, lo=0.0, hi=1.0):
        self.name, self.min, self.max, self.size = name, lo, hi, 1


@pytest.mark.parametrize("m", [2, 3])
def test_the_bot_with_thompson_batches(ctx, m):
    """harness bayesopt, config.score.type = 'thompson_sampling' with config.bot.objectives on two_spheres / three_spheres, d = 2, 200
    Sobol candidates, nInitial 4, batch 4, three model-based trials: 12 distinct rows are nominated, the hypervolume of the
    observations against a fixed reference point never decreases, the stolen rows leave every objective's grid, and last_objectives
    (hyps, seeds, ref, front) replays to the same picks on fresh stagings."""
    import bot7_amd
    from bot7_amd import _lib
    from harness import benchmarks as B, bots
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    ref = [1.3] * m
    obj = {"ref": ref, "model": dict(mcfg, seed=6)} if m == 2 else {"ref": ref, "models": [dict(mcfg, seed=6), dict(mcfg, seed=7)]}
    cfg = {"bot": {"verbose": 0, "budget": 7, "nInitial": 4, "nSamples": 2, "seed": 2, "batch": 4, "objectives": obj},
           "grid": {"type": "sobol", "size": 200, "dims": 2}, "score": {"type": "thompson_sampling", "nFeatures": 64}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 200, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    fn = B.two_spheres if m == 2 else B.three_spheres
    bot = bots.bayesopt(fn, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})
    front_fn, hv_fn = (_lib.pareto_front2, _lib.hypervolume2) if m == 2 else (_lib.pareto_front3, _lib.hypervolume3)
    hv, picked = [], []
    try:
        for t in range(7):
            before = np.asarray(bot.candidates).copy()
            n = 0 if bot.responses is None else len(bot.responses)
            x, y = bot.run_trial()
            bot.update_best(x, y)
            assert len(bot.responses) == n + 4 and bot.responses.shape[1] == m and len(bot.candidates) == len(before) - 4
            hv.append(hv_fn(front_fn(bot.responses, ref)[0], ref))
            assert hv[-1] == bot.best["hv"]
            if t < 4:
                continue
            last = bot.last_objectives
            others = [bot.objective2] if m == 2 else bot.objectives23
            cs = [ctx] + [o["ctx"] for o in others]
            idx = last["index"]
            assert len(set(idx)) == 4 and np.array_equal(before[np.asarray(idx) - 1], bot.observed[n:])
            picked += [tuple(r) for r in before[np.asarray(idx) - 1]]
            for c in cs:                                       # the stolen rows left every objective's grid
                assert np.array_equal(c.grid_download(), np.asarray(bot.candidates))
            assert np.array_equal(last["front"], front_fn(bot.responses[:n], ref)[0])
            # the replay: fresh contexts, this trial's hyper samples and seeds, the grid as it stood
            fresh = [bot7_amd.Context(0) for _ in range(m)]
            try:
                paths = []
                for col, (c, hyps, seed) in enumerate(zip(fresh, last["hyps"], last["seeds"])):
                    stage(c, bot.observed[:n], bot.responses[:n, col:col + 1], before)
                    c.ts_paths(hyps, 4, n_features=64, seed=seed)
                    paths.append(c.ts_last_paths())
                h2, i2, y2 = fresh[0].ts_hvi_nominate(fresh[1] if m == 2 else fresh[1:], last["front"], last["ref"])
                assert i2.tolist() == idx and bits(h2) == bits(last["hvi"]) and bits(y2) == bits(last["y"])
                rv, rr, ry, _ = R.replay(paths, last["front"], last["ref"])
                assert (rr + 1).tolist() == idx and bits(rv) == bits(h2)
            finally:
                for c in fresh:
                    c.close()
        print("m = %d: hypervolume per trial %s" % (m, ["%.4f" % h for h in hv]))
        assert len(set(picked)) == 12
        assert all(b >= a for a, b in zip(hv, hv[1:])) and hv[-1] > 0.0
    finally:
        for o in ([bot.objective2] if bot.objective2 else []) + list(bot.objectives23 or ()):
            o["ctx"].close()
