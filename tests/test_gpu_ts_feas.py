"""b7_ts_feas_nominate / b7_ts_feas_compute on the GPU: constrained Thompson sampling.

The kernels are held to their numpy float64 restatement (tests/_ts_feas_ref.py, itself held to exact rational arithmetic by
tests/test_ts_feas_host.py) BIT FOR BIT: a key is differences, maxima and a running sum, one rounded operation per operator,
contraction off, and the pick is comparisons alone.  The nominations on real contexts are replayed on the host from the downloaded
paths by the restated sequential rule and must agree exactly: picks, classes, keys and path values."""
import os

import numpy as np
import pytest

import _ts_feas_ref as R

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


def same(a, b):
    """Bit for bit, any NaN standing for any other."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a).view(np.int64), np.where(nb, 0.0, b).view(np.int64))


def refused(code, word, fn):
    import bot7_amd
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


def agrees(out, f, c, thr, viol=True):
    want = R.replay(f, c, thr)
    assert np.array_equal(out["index"], want["index"]), (out["index"], want["index"])
    assert np.array_equal(out["cls"], want["cls"]) and same(out["key"], want["key"])
    if viol:
        assert same(out["viol"], R.keys(f, c, thr)[0])
    return want


# ---- 1. b7_ts_feas_compute equals the restatement bit for bit ------------------------------------------------------------------------
def make_inputs(M1, q, C, seed):
    """Random values with, from 64 rows up: NaN and +-inf entries in f and in each constraint, one-ulp neighbours of the thresholds,
    duplicated rows; and, from five paths up: path 1 with no feasible row, path 2 with exactly one, path 3 all NaN."""
    rng = np.random.default_rng(seed)
    f, c, thr = rng.normal(0.0, 1.0, (M1, q)), rng.normal(0.0, 1.0, (C, M1, q)), rng.normal(0.0, 0.5, C)
    if M1 < 64:
        return f, c, thr
    f[3, 0], f[5, q - 1], f[7, 0], f[9, q - 1] = NAN, NAN, INF, -INF
    for k in range(C):
        c[k, 11 + k, 0], c[k, 20 + k, q - 1], c[k, 29 + k, 0] = NAN, INF, -INF
        c[k, 38 + k, :] = np.nextafter(thr[k], INF)
        c[k, 47 + k, :] = np.nextafter(thr[k], -INF)
        c[k, 56, :] = thr[k]
    f[60], c[:, 60] = f[59], c[:, 59]                      # duplicated rows: equal keys go to the lowest row
    f[62], c[:, 62] = f[61], c[:, 61]
    if q >= 5:
        if C:
            c[0, :, 1] = thr[0] + 0.01 + np.abs(c[0, :, 1])     # path 1: no feasible row
            c[:, :, 2] = thr[:, None] + 0.01 + np.abs(c[:, :, 2])
            c[:, M1 // 2, 2] = thr - 0.5                        # path 2: exactly one ...
            f[M1 // 2, 0], c[0, M1 // 2, 1] = 50.0, thr[0] + 100.0  # ... which neither earlier path takes
        f[:, 3] = NAN                                           # path 3: no row scores
    return f, c, thr


@pytest.mark.parametrize("M1", [1, 63, 64, 65, 257, 1000])
def test_compute_equals_the_restatement(ctx, M1):
    """One workgroup ragged and full, two, five; every q and C.  (M1 = 1 admits q = 1 alone.)"""
    n = 0
    for q in (1, 5, 16):
        if q > M1:
            continue
        for C in (0, 1, 3, 8):
            f, c, thr = make_inputs(M1, q, C, 1000 * q + C)
            out = ctx.ts_feas_compute(f, c, thr)
            want = agrees(out, f, c, thr)
            n += 1
            if q >= 5 and M1 >= 64:
                assert out["index"][3] == 0 and out["cls"][3] == -1 and np.isnan(out["key"][3])
                if C:
                    assert out["cls"][1] == 1 and out["cls"][2] == 0 and out["index"][2] == M1 // 2 + 1 and out["cls"][0] == 0
                assert len(set(out["index"].tolist()) - {0}) == q - 1
            assert out["viol"].shape == (M1, q) and want["reruns"] >= 0
    print("M1 = %d: %d (q, C) cases agree bit for bit" % (M1, n))
    assert n == (4 if M1 == 1 else 12)


def test_compute_where_the_grid_stride_loop_wraps(ctx):
    """More rows than the launch has lanes (the block cap times the block size): every lane takes a second row, the last ones do
    not.  The best rows of the two paths are planted in the wrapped part and in the last row."""
    from bot7_amd import _lib
    M1 = _lib.TS_FEAS_THREADS * _lib.TS_FEAS_BLOCKS_MAX + 257
    f, c, thr = make_inputs(M1, 2, 1, 3)
    c[0, M1 - 1, 0], f[M1 - 1, 0] = thr[0] - 1.0, -50.0
    c[0, M1 - 200, 1], f[M1 - 200, 1] = thr[0], -60.0
    c[0, 9, 1] = thr[0] + 1.0                              # (make_inputs' -inf objective value in row 9 of the last path: not feasible)
    out = ctx.ts_feas_compute(f, c, thr)
    agrees(out, f, c, thr)
    assert out["index"].tolist() == [M1, M1 - 199]


def test_compute_refusals(ctx):
    f, c = np.zeros((8, 2)), np.zeros((1, 8, 2))
    refused(-1, "not finite", lambda: ctx.ts_feas_compute(f, c, [INF]))
    refused(-1, "not finite", lambda: ctx.ts_feas_compute(f, c, [NAN]))
    refused(-1, "C = 9 constraints", lambda: ctx.ts_feas_compute(f, np.zeros((9, 8, 2)), np.zeros(9)))
    refused(-1, "q = 17 not in [1, 16]", lambda: ctx.ts_feas_compute(np.zeros((20, 17)), np.zeros((0, 20, 17)), []))
    refused(-1, "fewer than q = 5 paths", lambda: ctx.ts_feas_compute(np.zeros((4, 5)), np.zeros((0, 4, 5)), []))
    L, key, cls, idx = ctx._L, np.zeros(2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
    ptr = lambda x: x.ctypes.data
    thr = np.zeros(1)
    err = lambda: L.b7_last_error(ctx._h).decode()
    assert L.b7_ts_feas_compute(ctx._h, None, ptr(c), ptr(thr), 8, 2, 1, None, ptr(key), ptr(cls), ptr(idx)) == -1 and "NULL argument" in err()
    assert L.b7_ts_feas_compute(ctx._h, ptr(f), None, ptr(thr), 8, 2, 1, None, ptr(key), ptr(cls), ptr(idx)) == -1 and "cvals is NULL" in err()
    assert L.b7_ts_feas_compute(ctx._h, ptr(f), ptr(c), None, 8, 2, 1, None, ptr(key), ptr(cls), ptr(idx)) == -1 and "thresholds is NULL" in err()
    assert L.b7_ts_feas_compute(ctx._h, ptr(f), ptr(c), ptr(thr), 8, 2, 1, None, None, ptr(cls), ptr(idx)) == -1 and "NULL argument" in err()
    out = ctx.ts_feas_compute(f, c, [0.0], want_viol=False)      # the call after a refusal works; no violations asked for
    assert out["viol"] is None and out["index"].tolist() == [1, 2] and out["cls"].tolist() == [0, 0]


# ---- 2. collisions --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prof():
    """A context of the diagnostic build that scores all q paths in one pass and resolves the taken rows on the host, with phase
    profiling on: the launch count of the phase "ts_feas_rerun" is the number of reruns."""
    import bot7_amd
    os.environ["B7_TS_FEAS_ONEPASS"] = "1"
    try:
        c = bot7_amd.Context(0, lib="diag")
    finally:
        del os.environ["B7_TS_FEAS_ONEPASS"]
    c.profile_enable(True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def perpath():
    """A context of the shipped library, which picks path by path: q chained passes, each with exclusions (the default arm)."""
    import bot7_amd
    c = bot7_amd.Context(0)
    c.profile_enable(True)
    yield c
    c.close()


def reruns_of(c, f, cv, thr):
    c.profile_reset()
    out = c.ts_feas_compute(f, cv, thr)
    return out, c.profile_get("ts_feas_rerun")[1], c.profile_get("ts_feas")[1], c.profile_get("ts_feas_paths")[1]


def collision_cases():
    rng = np.random.default_rng(21)
    M1, q = 300, 5
    base_f, base_c, thr = rng.normal(0.0, 1.0, M1), rng.normal(0.0, 1.0, M1), [0.25]
    every = (np.repeat(base_f[:, None], q, 1), np.repeat(base_c[None, :, None], q, 2), thr, q - 1)     # every path the same ordering
    f, c = rng.normal(0.0, 1.0, (M1, q)), rng.normal(0.0, 1.0, (1, M1, q))
    for j in range(q):
        f[40 * j + 3, j], c[0, 40 * j + 3, j] = -100.0 - j, 0.0                                        # distinct minimisers
    distinct = (f, c, thr, 0)
    f2, c2 = f.copy(), c.copy()
    f2[3, 2], c2[0, 3, 2] = -200.0, 0.0                    # path 2's best is row 3, which path 0 takes: it re-picks ...
    f2[200, 2], c2[0, 200, 2] = -150.0, 0.0                # ... row 200, which is path 3's unexcluded best: path 3 runs again too
    f2[200, 3], c2[0, 200, 3] = -300.0, 0.0
    middle = (f2, c2, thr, 2)
    return {"every": every, "distinct": distinct, "middle": middle}


@pytest.mark.parametrize("case", ["every", "distinct", "middle"])
def test_collisions_resolve_as_the_sequential_rule(prof, perpath, case):
    f, c, thr, want_reruns = collision_cases()[case]
    out, reruns, passes, _ = reruns_of(prof, f, c, thr)
    want = agrees(out, f, c, thr)
    assert want["reruns"] == want_reruns and reruns == want_reruns and passes == 1
    assert len(set(out["index"].tolist())) == f.shape[1]
    if case == "every":                                    # the q best rows of the common ordering, in order
        _, cls, key = R.keys(f[:, :1], c[:, :, :1], thr)
        order = sorted(range(len(f)), key=lambda r: (cls[r, 0], key[r, 0], r))
        assert out["index"].tolist() == [r + 1 for r in order[:5]]
    if case == "middle":
        assert out["index"].tolist() == [4, 44, 201, 124, 164]
    # the per-path arm, the library's default: the same bits, by q chained passes and no one-pass arg-min
    out2, reruns2, passes2, chained = reruns_of(perpath, f, c, thr)
    assert reruns2 == 0 and passes2 == 1 and chained == 1      # (the one pass runs for the violations alone)
    for name in ("index", "cls"):
        assert np.array_equal(out[name], out2[name]), name
    assert same(out["key"], out2["key"]) and same(out["viol"], out2["viol"])


def test_both_arms_on_the_special_inputs(prof, perpath):
    for q, C in ((1, 0), (5, 3), (16, 8)):
        f, c, thr = make_inputs(257, q, C, 77 + q)
        a, b = prof.ts_feas_compute(f, c, thr), perpath.ts_feas_compute(f, c, thr, want_viol=False)
        agrees(a, f, c, thr)
        assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["cls"], b["cls"]) and same(a["key"], b["key"]) and b["viol"] is None


# ---- 3. real contexts -------------------------------------------------------------------------------------------------------------------
N, D, M, F, S = 12, 2, 500, 64, 2
SEEDS = (101, 202, 303)


@pytest.fixture(scope="module")
def prob():
    rng = np.random.default_rng(5)
    X, Xc = rng.random((N, D)), rng.random((M, D))
    x1, x2 = 6.0 * X[:, 0], 6.0 * X[:, 1]
    Y = np.stack([np.cos(2 * x1) * np.cos(x2) + np.sin(x1), np.cos(x1 + x2), np.sin(x1) * np.sin(x2)], axis=1)
    hyps = []
    for col in range(3):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(D, 0.3 + 0.2 * s + 0.1 * col), "amp": amp * (1.0 + 0.3 * s), "noise": 1e-4 * amp,
                      "mean": float(np.mean(Y[:, col])) + 0.02 * s} for s in range(S)])
    return X, Y, Xc, hyps


@pytest.fixture(scope="module")
def three():
    import bot7_amd
    cs = [bot7_amd.Context(0) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def keep_paths(cs, prob, q, kernel="ardse", staged=False):
    X, Y, Xc, hyps = prob
    out = []
    for k, c in enumerate(cs):
        if not staged:
            stage(c, X, Y[:, k:k + 1], Xc, kernel)
        c.ts_paths(hyps[k], q, n_features=F, seed=SEEDS[k])
        out.append(c.ts_last_paths())
    return out


THR = [0.5, 0.25]


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("q", [1, 5, 16])
def test_nomination_equals_the_replay(three, prob, kernel, q):
    X, Y, Xc, hyps = prob
    a, b, c = three
    paths = keep_paths(three, prob, q, kernel)
    # an accumulator, a feasibility column and a kept posterior on the objective's context: the nomination must leave them alone
    a.eval_posterior(hyps[0])
    a.eval_nominate(hyps[0], score="ei", fmin=[float(Y[:, 0].min())], tradeoff=0.0)
    a.feas_reset()
    a.feas_add(np.linspace(-1.0, 0.0, M))
    snap = lambda: (a.score_finish(1.0, download=True)[2].copy(), a.feas_get().copy(), a.posterior_get(0), a.posterior_get(1))
    before = snap()
    out = a.ts_feas_nominate([b, c], THR)
    after = snap()
    assert same(before[0], after[0]) and same(before[1], after[1])
    assert all(same(x, y) for s in (2, 3) for x, y in zip(before[s], after[s]))
    want = R.replay(paths[0], np.stack(paths[1:]), THR)
    print("%s, q = %d: picks %s, classes %s; %d paths' best rows were taken by earlier paths" % (kernel, q, out["index"].tolist(), out["cls"].tolist(), want["reruns"]))
    assert np.array_equal(out["index"], want["index"]) and np.array_equal(out["cls"], want["cls"]) and same(out["key"], want["key"])
    assert out["reruns"] == 0 and len(set(out["index"].tolist())) == q      # (the default arm picks path by path: nothing runs again) and out["index"].min() >= 1 and out["index"].max() <= M
    # y_out: the picks' entries of the paths
    for j in range(q):
        r = out["index"][j] - 1
        assert same(out["y"][j], [p[r, j] for p in paths])
    assert same(out["y"], want["y"])
    # the same call twice gives the same bits, and the kept paths are untouched
    again = a.ts_feas_nominate([b, c], THR)
    assert all(same(out[k], again[k]) for k in ("key", "y")) and np.array_equal(out["index"], again["index"]) and out["reruns"] == again["reruns"]
    assert all(same(cc.ts_last_paths(), p) for cc, p in zip(three, paths))
    # coinciding contexts: the objective's own paths as a constraint
    own = a.ts_feas_nominate([a], [float(np.median(paths[0]))])
    w2 = R.replay(paths[0], paths[0][None], [float(np.median(paths[0]))])
    assert np.array_equal(own["index"], w2["index"]) and same(own["key"], w2["key"])
    if q == 5:
        # the first three picks are a q = 3 call's.  The draws depend on (seed, j) alone, but a hyper sample's paths are fitted as the
        # columns of ONE multi-column fit, so a path's last bits depend on how many paths share its sample: picks and classes are held
        # equal, the values to the posterior-mean bar of tests/test_gpu_ts.py (1e-5 relative to max(1, |value|))
        keep_paths(three, prob, 3, kernel, staged=True)
        o3 = a.ts_feas_nominate([b, c], THR)
        assert np.array_equal(o3["index"], out["index"][:3]) and np.array_equal(o3["cls"], out["cls"][:3])
        assert np.abs(o3["y"] - out["y"][:3]).max() <= 1e-5 * max(1.0, float(np.abs(out["y"][:3]).max()))
    for cc in three:
        cc.gp_set_kernel("ardse")


@pytest.mark.parametrize("q", [1, 5, 16])
def test_no_constraint_is_ts_nominate(three, prob, q):
    """C = 0: the picks and the minima are b7_ts_nominate's on the same context, bit for bit."""
    X, Y, Xc, hyps = prob
    a = three[0]
    stage(a, X, Y[:, :1], Xc)
    vals, idx = a.ts_nominate(hyps[0], q, n_features=F, seed=77)
    out = a.ts_feas_nominate([], [])
    assert np.array_equal(out["index"], idx) and same(out["key"], vals) and (out["cls"] == 0).all() and out["y"].shape == (q, 1)
    assert same(out["y"][:, 0], vals)


# ---- 4. every refusal, by code and by a word of its message -------------------------------------------------------------------------------
def test_state_and_refusals(prob):
    import bot7_amd
    from conftest import make_network
    X, Y, Xc, hyps = prob
    fresh = [bot7_amd.Context(0) for _ in range(3)]
    try:
        a, b, c = fresh
        for k, cc in enumerate(fresh):
            stage(cc, X, Y[:, k:k + 1], Xc)
        refused(-4, "no kept paths of the objective", lambda: a.ts_feas_nominate([b], [0.5]))
        a.ts_paths(hyps[0], 4, n_features=F, seed=1)
        refused(-4, "no kept paths of constraint 1", lambda: a.ts_feas_nominate([b], [0.5]))
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        refused(-4, "no kept paths of constraint 2", lambda: a.ts_feas_nominate([b, c], THR))
        c.ts_paths(hyps[2], 4, n_features=F, seed=3)
        good = a.ts_feas_nominate([b, c], THR)
        # thresholds, C, NULL
        refused(-1, "threshold 2 (inf) is not finite", lambda: a.ts_feas_nominate([b, c], [0.5, INF]))
        refused(-1, "threshold 1 (nan) is not finite", lambda: a.ts_feas_nominate([b, c], [NAN, 0.5]))
        refused(-1, "C = 9 constraints", lambda: a.ts_feas_nominate([b] * 9, [0.5] * 9))
        assert a.ts_feas_nominate([b] * 8, [0.5] * 8)["index"].shape == (4,)
        L, key, cls, i8 = a._L, np.zeros(4), np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int64)
        import ctypes
        ptr = lambda x: x.ctypes.data
        err = lambda: L.b7_last_error(a._h).decode()
        thr = np.array([0.5])
        hs = (ctypes.c_void_p * 1)(b._h)
        null = (ctypes.c_void_p * 1)(None)
        cast = lambda x: ctypes.cast(x, ctypes.c_void_p)
        assert L.b7_ts_feas_nominate(a._h, None, ptr(thr), 1, ptr(key), ptr(cls), ptr(i8), None, None) == -1 and "cons is NULL" in err()
        assert L.b7_ts_feas_nominate(a._h, cast(null), ptr(thr), 1, ptr(key), ptr(cls), ptr(i8), None, None) == -1 and "constraint 1's context is NULL" in err()
        assert L.b7_ts_feas_nominate(a._h, cast(hs), None, 1, ptr(key), ptr(cls), ptr(i8), None, None) == -1 and "thresholds is NULL" in err()
        assert L.b7_ts_feas_nominate(a._h, cast(hs), ptr(thr), 1, None, ptr(cls), ptr(i8), None, None) == -1 and "NULL argument" in err()
        assert L.b7_ts_feas_nominate(a._h, cast(hs), ptr(thr), -1, ptr(key), ptr(cls), ptr(i8), None, None) == -1 and "C = -1" in err()
        assert L.b7_ts_feas_nominate(None, cast(hs), ptr(thr), 1, ptr(key), ptr(cls), ptr(i8), None, None) == -1
        assert L.b7_ts_feas_nominate(a._h, cast(hs), ptr(thr), 1, ptr(key), ptr(cls), ptr(i8), None, None) == 0      # y_out and reruns_out are optional
        # the call after a refusal works, with the usual bits
        again = a.ts_feas_nominate([b, c], THR)
        assert np.array_equal(again["index"], good["index"]) and same(again["key"], good["key"]) and same(again["y"], good["y"])
        # q differs; M differs
        b.ts_paths(hyps[1], 3, n_features=F, seed=2)
        refused(-1, "constraint 1 keeps q = 3 paths, the objective 4", lambda: a.ts_feas_nominate([b, c], THR))
        b.grid_upload(Xc[:40])
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        refused(-1, "the grid of constraint 1 has M = 40 rows, the objective's 500", lambda: a.ts_feas_nominate([b, c], THR))
        b.grid_upload(Xc)
        b.ts_paths(hyps[1], 4, n_features=F, seed=2)
        assert np.array_equal(a.ts_feas_nominate([b, c], THR)["index"], good["index"])
        # stale paths: the grid changed, the data changed, the kernel changed; b7_ts_last_paths keeps serving them
        kept = b.ts_last_paths()
        b.grid_remove(3)
        refused(-4, "kept paths of constraint 1 are stale", lambda: a.ts_feas_nominate([b, c], THR))
        assert same(b.ts_last_paths(), kept)
        a.gp_set_data(X[:10], Y[:10, :1])
        refused(-4, "kept paths of the objective are stale", lambda: a.ts_feas_nominate([c], [0.5]))
        a.gp_set_data(X, Y[:, :1])
        a.ts_paths(hyps[0], 4, n_features=F, seed=1)
        c.gp_set_kernel("ardmatern52")
        refused(-4, "kept paths of constraint 1 are stale", lambda: a.ts_feas_nominate([c], [0.5]))
        c.gp_set_kernel("ardse")
        # a b7_ts_nominate's paths serve as well; the DNGO head's do not
        c.ts_nominate(hyps[2], 4, n_features=F, seed=3)
        o1, o2 = a.ts_feas_nominate([c, c], THR), a.ts_feas_nominate([c, c], THR)
        assert np.array_equal(o1["index"], o2["index"]) and same(o1["key"], o2["key"])
        Wn, bn = make_network(D, [16, 8], seed=3)
        c.blr_ts_nominate(Wn, bn, "Tanh", X, Y[:, 2], [0.5], [100.0], [0.1], 4, seed=4)
        refused(-5, "b7_blr_ts_nominate", lambda: a.ts_feas_nominate([c], [0.5]))
        refused(-5, "b7_blr_ts_nominate", lambda: c.ts_feas_nominate([], []))
        # a group member
        g = bot7_amd.Group([0, 0])
        try:
            g.grid_upload(Xc)
            g.gp_set_data(X, Y[:, :1])
            refused(-4, "group", lambda: a.ts_feas_nominate([g.members[0]], [0.5]))
            refused(-4, "group", lambda: g.members[1].ts_feas_nominate([a], [0.5]))
        finally:
            g.close()
    finally:
        for cc in fresh:
            cc.close()


# ---- 5. the harness bot end to end -------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name, lo=0.0, hi=1.0):
        self.name, self.min, self.max, self.size = name, lo, hi, 1


def test_the_bot_on_gardner1(ctx):
    """harness bayesopt, config.score.type = 'constrained_thompson_sampling' on gardner1 (c <= 0.5), d = 2, 200 Sobol candidates,
    nInitial 4, batch 4, three model-based trials: the rows nominated within a trial are distinct, the stolen rows leave every context's
    grid, and last_constrained (hyps, seeds, thresholds) replays to the same picks on fresh stagings and through the restated rule."""
    import bot7_amd
    from harness import benchmarks as B, bots
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 5}
    cfg = {"bot": {"verbose": 0, "budget": 7, "nInitial": 4, "nSamples": 2, "seed": 2, "batch": 4,
                   "constraints": [{"threshold": B.GARDNER1_THRESHOLD, "model": dict(mcfg, seed=6)}]},
           "grid": {"type": "sobol", "size": 200, "dims": 2}, "score": {"type": "constrained_thompson_sampling", "nFeatures": 64}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": 200, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    bot = bots.bayesopt(B.gardner1, [_H("x1"), _H("x2")], cfg, cache={"candidates": grid, "model": model})
    picked = []
    try:
        for t in range(7):
            before = np.asarray(bot.candidates).copy()
            n = 0 if bot.responses is None else len(bot.responses)
            x, y = bot.run_trial()
            bot.update_best(x, y)
            assert len(bot.responses) == n + 4 and bot.responses.shape[1] == 2 and len(bot.candidates) == len(before) - 4
            if t < 4:
                continue
            last = bot.last_constrained
            cs = [ctx] + [con["ctx"] for con in bot.constraints]
            idx = last["index"]
            assert len(set(idx)) == 4 and np.array_equal(before[np.asarray(idx) - 1], bot.observed[n:])
            picked += [tuple(r) for r in before[np.asarray(idx) - 1]]
            for c in cs:                                       # the stolen rows left every context's grid
                assert np.array_equal(c.grid_download(), np.asarray(bot.candidates))
            assert len(set(last["seeds"])) == 2 and last["thresholds"] == [B.GARDNER1_THRESHOLD]
            # the replay: fresh contexts, this trial's hyper samples and seeds, the grid as it stood
            fresh = [bot7_amd.Context(0) for _ in range(2)]
            try:
                paths = []
                for col, (c, hyps, seed) in enumerate(zip(fresh, [last["hyps"]] + last["constraint_hyps"], last["seeds"])):
                    stage(c, bot.observed[:n], bot.responses[:n, col:col + 1], before)
                    c.ts_paths(hyps, 4, n_features=64, seed=seed)
                    paths.append(c.ts_last_paths())
                o2 = fresh[0].ts_feas_nominate(fresh[1:], last["thresholds"])
                assert o2["index"].tolist() == idx and same(o2["key"], last["key"]) and same(o2["y"], last["y"])
                want = R.replay(paths[0], np.stack(paths[1:]), last["thresholds"])
                assert want["index"].tolist() == idx and np.array_equal(want["cls"], last["cls"]) and same(want["key"], last["key"])
                assert same(want["y"], last["y"]) and last["reruns"] == 0
            finally:
                for c in fresh:
                    c.close()
        feas = bot.responses[:, 1] <= B.GARDNER1_THRESHOLD
        print("gardner1: %d of %d rows feasible, best feasible %s, classes of the last trial %s" % (
            int(feas.sum()), len(feas), bot.responses[feas, 0].min() if feas.any() else None, bot.last_constrained["cls"].tolist()))
        assert len(set(picked)) == 12
        if feas.any():
            assert float(np.ravel(bot.best["y"])[0]) == bot.responses[feas, 0].min()
    finally:
        for con in bot.constraints or []:
            con["ctx"].close()
