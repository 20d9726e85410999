"""b7_grid_trust_region on the GPU, and the trust-region loop of the harness bot.

The map is compared BIT FOR BIT with the numpy restatement (tests/_tr_ref.tr_map): the mask is integer arithmetic, the value two
rounded operations in a fixed order.  A mapped grid is an ordinary grid: nominations on it equal, bit for bit, the same calls on a
context into which it was uploaded.  The loop is replayed from its trace.  No optimisation-quality claim."""
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib
from bot7_amd.grids.abstract import ResidentGrid

import _tr_ref as R

pytestmark = pytest.mark.gpu
MS = (1, 255, 256, 257, 4099)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def refused(code, word, fn):
    with pytest.raises(_lib.Bot7HipError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), (code, word, str(e.value))


def make_base(c, M, d, seed, download=True):
    """Base points in [0, 1): Sobol below 40 dimensions, the counter-based uniform grid above."""
    if d < 40:
        return c.grid_sobol(M, d, 1, download=download)
    return c.grid_random(M, d, seed, download=download)


def make_box(d, seed):
    """A box inside [-2, 3]^d: column 0 has zero width and, from three dimensions on, column 1's centre sits on its lower wall."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-2.0, 1.0, d)
    hi = lo + rng.uniform(0.01, 2.0, d)
    center = lo + (hi - lo) * rng.uniform(0.0, 1.0, d)
    center = np.minimum(np.maximum(center, lo), hi)
    hi[0] = lo[0]
    center[0] = lo[0]
    if d >= 3:
        center[1] = lo[1]
    return center, lo, hi


@pytest.mark.parametrize("d", [1, 3, 6, 32, 39, 64, 96])
def test_map_equals_the_restatement_bit_for_bit(ctx, d):
    center, lo, hi = make_box(d, d)
    if d == 1:
        boxes = [(center, lo, hi), (np.array([0.25]), np.array([-0.5]), np.array([1.5])), (np.array([0.3]), np.array([0.3]), np.array([0.9]))]
    else:
        boxes = [(center, lo, hi)]
    rng = np.random.default_rng(100 + d)
    n = 0
    for M in MS:
        for prob in (0.0, 0.625, 1.0):
            for rotate in (False, True):
                cen, l, h = boxes[n % len(boxes)]
                shift = rng.random(d) if rotate else None
                seed, off = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 10 ** 6))
                base = make_base(ctx, M, d, seed + 1)
                assert base.min() >= 0.0 and base.max() < 1.0
                v0 = ctx.grid_version
                ctx.grid_trust_region(cen, l, h, prob, shift=shift, seed=seed, row_offset=off)
                assert ctx.grid_version == v0 + 1
                got = ctx.grid_download()
                want, moved = R.tr_map(base, cen, l, h, prob, shift, seed, off)
                assert np.array_equal(bits(got), bits(want)), (M, d, prob, rotate)
                assert np.array_equal(bits(got[~moved]), bits(np.broadcast_to(cen, (M, d))[~moved]))     # the centre's bits
                assert np.all(got >= l) and np.all(got <= h)
                if prob == 0.0:
                    assert np.array_equal(moved.sum(axis=1), np.ones(M, dtype=np.int64))
                if prob == 0.625 and rotate:                       # the same call on the same base: the same bits
                    make_base(ctx, M, d, seed + 1, download=False)
                    ctx.grid_trust_region(cen, l, h, prob, shift=shift, seed=seed, row_offset=off)
                    assert np.array_equal(bits(ctx.grid_download()), bits(got))
                n += 1


@pytest.mark.parametrize("d,base", [(6, "sobol"), (64, "random")])
def test_slices_with_their_row_offset_are_the_whole(ctx, d, base):
    M, cut, off0 = 1000, 333, 7                                    # 333 is no multiple of the block's 256 threads
    center, lo, hi = make_box(d, 40 + d)
    shift = np.random.default_rng(d).random(d)

    def gen(rows, first):
        if base == "sobol":
            ctx.grid_sobol(rows, d, 1 + first, download=False)
        else:
            ctx.grid_random(rows, d, 99, first, download=False)

    gen(M, 0)
    ctx.grid_trust_region(center, lo, hi, 0.625, shift=shift, seed=31, row_offset=off0)
    whole = ctx.grid_download()
    parts = []
    for first, rows in ((0, cut), (cut, M - cut)):
        gen(rows, first)
        ctx.grid_trust_region(center, lo, hi, 0.625, shift=shift, seed=31, row_offset=off0 + first)
        parts.append(ctx.grid_download())
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


def _problem(N, d, M, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (N, d))
    y = np.sin(3.0 * X.sum(axis=1, keepdims=True)) + X[:, -1:] ** 2
    amp = float(np.var(y))
    hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(y))}
    hyps = [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.3 * s), amp=amp * (1.0 + 0.2 * s)) for s in range(2)]
    center = X[int(np.argmin(y[:, 0]))]
    lo, hi = _lib.tr_box(hyps, center, 0.4, np.zeros(d), np.ones(d))
    return X, y, hyps, center, lo, hi


def test_invalidation(ctx):
    X, y, hyps, center, lo, hi = _problem(24, 6, 512, 1)
    ctx.grid_random(512, 6, 3, download=False)
    ctx.gp_set_data(X, y)
    ctx.eval_posterior(hyps)
    ctx.eval_nominate(hyps, score="ei", fmin=[float(y.min())])
    ctx.feas_reset()
    assert ctx.posterior_get(0)[0].shape == (512,) and ctx.feas_get().shape == (512,) and ctx.score_finish(1.0)[1] >= 1
    v0 = ctx.grid_version
    ctx.grid_trust_region(center, lo, hi, 0.5, seed=1)
    assert ctx.grid_version == v0 + 1
    refused(-4, "no kept posterior", lambda: ctx.posterior_get(0))          # what a grid upload leaves behind, too
    refused(-4, "score_reset", lambda: ctx.score_finish(1.0))
    refused(-4, "feas", lambda: ctx.feas_get())
    ctx.grid_upload(ctx.grid_download())
    refused(-4, "no kept posterior", lambda: ctx.posterior_get(0))
    refused(-4, "score_reset", lambda: ctx.score_finish(1.0))
    refused(-4, "feas", lambda: ctx.feas_get())


@pytest.mark.parametrize("N", [24, 130])                                     # the one-launch kernels; the general schedule
def test_a_mapped_grid_is_an_ordinary_grid(ctx, N):
    d, M = 6, 2048
    X, y, hyps, center, lo, hi = _problem(N, d, M, N)
    ctx.grid_random(M, d, 17, download=False)
    ctx.grid_trust_region(center, lo, hi, 0.625, seed=23)
    ctx.gp_set_data(X, y)
    fmin = [float(y.min())]
    ei = ctx.eval_nominate(hyps, score="ei", fmin=fmin)
    ts = ctx.ts_nominate(hyps, 3, n_features=256, seed=5)
    other = bot7_amd.Context(0)
    try:
        other.grid_upload(ctx.grid_download())
        other.gp_set_data(X, y)
        ei2 = other.eval_nominate(hyps, score="ei", fmin=fmin)
        ts2 = other.ts_nominate(hyps, 3, n_features=256, seed=5)
    finally:
        other.close()
    assert ei[1] == ei2[1] and bits([ei[0]])[0] == bits([ei2[0]])[0]
    assert np.array_equal(ts[1], ts2[1]) and np.array_equal(bits(ts[0]), bits(ts2[0]))
    assert len(set(int(i) for i in ts[1])) == 3


def test_refusals(ctx):
    d = 6
    center, lo, hi = np.full(d, 0.5), np.full(d, 0.25), np.full(d, 0.75)
    fresh = bot7_amd.Context(0)
    try:
        refused(-4, "no candidate grid", lambda: fresh.grid_trust_region(center, lo, hi, 0.5))
    finally:
        fresh.close()
    g = bot7_amd.Group([0, 0])
    try:
        g.grid_upload(np.random.default_rng(0).random((64, d)))
        refused(-4, "group", lambda: g.members[0].grid_trust_region(center, lo, hi, 0.5))
    finally:
        g.close()
    ctx.grid_random(64, d, 1, download=False)
    v0, before = ctx.grid_version, ctx.grid_download()

    def vec(v, k, x):
        w = np.array(v, dtype=np.float64)
        w[k] = x
        return w

    bad = [("non-finite", lambda: ctx.grid_trust_region(vec(center, 2, np.nan), lo, hi, 0.5)),
           ("non-finite", lambda: ctx.grid_trust_region(center, vec(lo, 0, -np.inf), hi, 0.5)),
           ("non-finite", lambda: ctx.grid_trust_region(center, lo, vec(hi, 5, np.inf), 0.5)),
           ("non-finite", lambda: ctx.grid_trust_region(center, lo, hi, 0.5, shift=vec(np.zeros(d), 1, np.nan))),
           ("lo", lambda: ctx.grid_trust_region(vec(center, 3, 0.8), vec(lo, 3, 0.9), hi, 0.5)),
           ("center", lambda: ctx.grid_trust_region(vec(center, 1, 0.8), lo, hi, 0.5)),
           ("center", lambda: ctx.grid_trust_region(vec(center, 1, 0.2), lo, hi, 0.5)),
           ("prob", lambda: ctx.grid_trust_region(center, lo, hi, -0.01)),
           ("prob", lambda: ctx.grid_trust_region(center, lo, hi, 1.01)),
           ("prob", lambda: ctx.grid_trust_region(center, lo, hi, np.nan)),
           ("shift", lambda: ctx.grid_trust_region(center, lo, hi, 0.5, shift=vec(np.zeros(d), 4, 1.0))),
           ("shift", lambda: ctx.grid_trust_region(center, lo, hi, 0.5, shift=vec(np.zeros(d), 4, -0.1))),
           ("row_offset", lambda: ctx.grid_trust_region(center, lo, hi, 0.5, row_offset=-1))]
    for word, fn in bad:
        refused(-1, word, fn)
    L = _lib.load()
    p = [v.ctypes.data_as(_lib.C.c_void_p) for v in (center, lo, hi)]
    for k in range(3):
        args = list(p)
        args[k] = None
        assert L.b7_grid_trust_region(ctx._h, args[0], args[1], args[2], 0.5, None, 0, 0) == -1            # a NULL argument
    assert L.b7_grid_trust_region(None, p[0], p[1], p[2], 0.5, None, 0, 0) == -1
    assert np.array_equal(bits(ctx.grid_download()), bits(before))           # a refused call leaves the grid alone
    assert ctx.grid_version == v0
    with pytest.raises(_lib.Bot7HipError):
        ctx.grid_trust_region(center[:3], lo, hi, 0.5)


# ---- the loop ----------------------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


D, MC = 10, 2000
TR = {"length_init": 0.1, "length_min": 0.049, "failure_tolerance": 2}       # a halving to 0.05 stays; the next one restarts


def _bot(ctx, score, batch, base, seed=4):
    from harness import benchmarks, bots
    cfg = {"bot": {"verbose": 0, "budget": 30, "nInitial": 6, "nSamples": 2, "seed": seed, "batch": batch, "trust_region": dict(TR)},
           "grid": {"type": base, "size": MC, "dims": D},
           "score": dict({"type": score}, **({"nFeatures": 256} if score == "thompson_sampling" else {}))}
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    return bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(D)], cfg, cache={"model": model})


@pytest.mark.parametrize("score,batch,base", [("thompson_sampling", 1, "sobol"), ("thompson_sampling", 4, "random"),
                                              ("expected_improvement", 1, "sobol")])
def test_the_loop(ctx, score, batch, base):
    """ackley in 10 dimensions, 2000 candidates per trial, nInitial 6, budget 30: two runs under one seed agree bit for bit; every
    nominee lies in its trial's box and in the bounds; the trace regenerates every nominee on a fresh context; b7_tr_update
    replayed on the responses gives the traced lengths; a halving and a restart occur."""
    runs = []
    for rep in range(2):
        bot = _bot(ctx, score, batch, base)
        handed = []
        inner = bot.model.stage
        bot.model.stage = lambda X, Y, grid, inner=inner: handed.append(grid) or inner(X, Y, grid)
        bot.run_experiment()
        assert bot.candidates is None and all(isinstance(g, ResidentGrid) for g in handed) and handed
        runs.append((bot.observed.copy(), bot.responses.copy(), bot.tr_trace))
    (X, Y, trace), (X2, Y2, _) = runs
    assert X.shape == (30 * batch, D) and np.array_equal(bits(X), bits(X2)) and np.array_equal(bits(Y), bits(Y2))
    assert np.all(X >= 0.0) and np.all(X <= 1.0) and len(trace) == 30
    st = _lib.TrustRegionState(D, batch, TR["length_init"], TR["length_min"], None, None, TR["failure_tolerance"])
    other = bot7_amd.Context(0)
    try:
        since, n = 0, 0
        for t, rec in enumerate(trace):
            q = len(rec["index"])
            assert q == batch and np.array_equal(bits(rec["x"]), bits(X[n:n + q])) and rec["length_before"] == st.length
            if since < 6:
                assert rec["kind"] == "initial"
                if rec["base"] == "sobol":
                    other.grid_sobol(MC, D, rec["skip"], np.zeros(D), np.ones(D), download=False)
                else:
                    other.grid_random(MC, D, rec["base_seed"], 0, np.zeros(D), np.ones(D), download=False)
            else:
                assert rec["kind"] == "model"
                assert np.all(rec["x"] >= rec["lo"]) and np.all(rec["x"] <= rec["hi"])                    # inside the trial's box
                assert np.all(rec["lo"] >= 0.0) and np.all(rec["hi"] <= 1.0)
                if rec["base"] == "sobol":
                    other.grid_sobol(MC, D, rec["skip"], download=False)
                else:
                    other.grid_random(MC, D, rec["base_seed"], download=False)
                other.grid_trust_region(rec["center"], rec["lo"], rec["hi"], rec["prob"], shift=rec["shift"], seed=rec["map_seed"])
            again = np.concatenate([other.grid_download(i - 1, 1) for i in rec["index"]])
            assert np.array_equal(bits(again), bits(rec["x"])), t                                          # the trace regenerates the nominee
            restart = st.update(Y[n:n + q, 0])
            assert restart is rec["restart"] and st.length == rec["length_after"], t
            since = 0 if restart else since + 1
            n += q
    finally:
        other.close()
    lengths = [rec["length_after"] for rec in trace]
    print("loop %s batch=%d: best %.4f, lengths %s, restarts %d" % (score, batch, Y.min(), sorted(set(lengths)), st.restarts))
    assert TR["length_init"] / 2.0 in lengths                                # a halving occurred
    assert st.restarts >= 1 and any(rec["restart"] for rec in trace)          # and a restart
