"""A reused context against a fresh one, bit for bit, across every shape and policy (the catalogue: tests/_reuse_calls.py).

A b7_ctx owns grow-only buffers that are never cleared, and flags and remembered shapes beside them; what it computes rests on
padding conventions that each relayout has to re-establish.  Here one context walks through shapes, regimes, kernels and policies,
and every call of the catalogue must return the bytes that the same call returns as the first and only work of a new Context(0)
(new partner contexts where the call takes them).  There is no tolerance in this file; a refusal is a result and must be the same
refusal, and exactly the expected ones refuse (_reuse_calls.expected_refusal); every other reference must be finite.

References are cached per module and every reference context is closed before the next is made: the walker, its two partners and
one reference set are all that is alive at a time."""
import ctypes

import numpy as np
import pytest

import _reuse_calls as R
import bot7_amd
from bot7_amd._lib import Bot7HipError

pytestmark = pytest.mark.gpu

#        N    d   M     S
BIG = R.problem(300, 33, 1100, 4, seed=100, scale=1e6, q=16, n_features=256, name="BIG")   # larger than every target in every extent
A = R.problem(25, 3, 130, 2, seed=1, name="A")       # Npad 64: small regime, one block
C = R.problem(100, 6, 257, 2, seed=2, name="C")      # Npad 128: small regime, two blocks
B = R.problem(129, 6, 300, 3, seed=3, name="B")      # Npad 256 (tall): the general regime just past the switch
D = R.problem(150, 33, 200, 2, seed=4, name="D")     # general, the wide class (dpad 48)
E = R.problem(70, 4, 150, 1, seed=5, ycols=7, name="E")   # seven response columns (yld 64)
F = R.problem(80, 5, 200, 3, seed=6, head=True, name="F")  # the context is a Bayesian-linear head (z = 50) before the data arrive
J = R.problem(40, 3, 130, 1, seed=7, dup_rows=8, zero_noise=True, name="J")   # a fit that needs the jitter schedule
A_MATERN = R.problem(25, 3, 130, 2, seed=1, kernel="ardmatern52", name="A-matern")
SHAPES = {P.name: P for P in (BIG, A, B, C, D, E, F, J, A_MATERN)}

CACHE = {}
TOTALS = {"compared": 0, "refused": set(), "tests": 0}


@pytest.fixture(autouse=True)
def _count_tests():
    yield
    TOTALS["tests"] += 1


def _fresh(partners):
    cs = [bot7_amd.Context(0) for _ in range(3 if partners else 1)]

    def close():
        for c in cs:
            c.close()
    return cs[0], (cs[1] if partners else None), (cs[2] if partners else None), close


@pytest.fixture
def walker():
    cs = []

    def make():
        cs.extend(bot7_amd.Context(0) for _ in range(3))
        return tuple(cs)
    w = R.Walker(make, _fresh, cache=CACHE)
    yield w
    TOTALS["compared"] += w.compared
    TOTALS["refused"] |= w.refused
    for c in cs:
        c.close()


def _poison(w, P=BIG):
    """The whole catalogue at P for its side effect on the buffers; what refuses there is the expected set and nothing else."""
    for name, res in w.fill(P).items():
        code = R.expected_refusal(name, P)
        got = res[1] if R.is_refusal(res) else None
        assert got == code, "poison at %s, call %r: expected %r, got %r" % (P.name, name, code, res if R.is_refusal(res) else "a result")


# ---- a. poison, then each target
TARGETS = ("A", "B", "C", "D", "E", "F")


@pytest.mark.parametrize("target", TARGETS)
def test_a_after_the_poison_every_call_equals_a_fresh_context(walker, target):
    _poison(walker)
    walker.step(target, SHAPES[target])
    assert walker.compared == len(R.CALLS)


# ---- b. NaN poison
NAN_CALLS = (["gp_fit+gp_predict"] + ["score_" + k for k in R.KINDS] + ["eval_nominate[%s,S]" % k for k in R.KINDS] + ["eval_nominate_batch"])


def test_b_after_nan_inputs_every_call_equals_a_fresh_context(walker):
    c = walker.ctx
    R.setup(walker.env(BIG))
    X = BIG.X.copy()
    X[17, 5] = np.nan
    with pytest.raises(Bot7HipError) as e:   # "matrix contains NaN": returns after K, L and the scalings were written
        c.gp_fit(X, BIG.Y, **BIG.hyps[0])
    assert e.value.code == R.INVALID, str(e.value)
    Y, G = BIG.Y.copy(), BIG.G.copy()
    Y[[3, 150, 299]] = np.nan
    G[[0, 511, 1099]] = np.nan
    nan = R.derived(BIG, BIG.X, Y, BIG.Y2, BIG.Y3, G, "nan")
    for name, res in walker.fill(nan, NAN_CALLS).items():   # the NaN row classes of DESIGN.md: results with NaN rows, or INVALID; never a HIP error
        assert not R.is_refusal(res) or res[1] == R.INVALID, "NaN poison, call %r: %r" % (name, res)
    walker.step("A after NaN", A)
    walker.step("B after NaN", B)


# ---- c. transitions without poison
TRANSITIONS = {"small-general-small": ("A", "B", "A"), "width-class": ("B", "D", "B"), "se-matern-se": ("A", "A-matern", "A"),
               "seven-columns-to-one": ("E", "A"), "head-gp-head": ("F", "A", "F"), "jittered-to-clean": ("J", "A")}


@pytest.mark.parametrize("walk", sorted(TRANSITIONS))
def test_c_transitions(walker, walk):
    for k, name in enumerate(TRANSITIONS[walk]):
        walker.step("%s[%d]=%s" % (walk, k, name), SHAPES[name])
    for name in TRANSITIONS[walk]:   # only J's fits take the jitter schedule (its K is singular); no other step's do
        ref = CACHE[(SHAPES[name].key, "gp_fit_hyp+gp_predict_hyp")]
        jitter = np.frombuffer(ref["jitter"], dtype=np.float64)[0]
        assert (ref["info"] != 0 and jitter > 0.0) if name == "J" else (ref["info"] == 0 and jitter == 0.0), (name, ref["info"], jitter)


# ---- d. order of policies
def _between(w, P):
    """Three grid rows leave and one observation arrives between two calls; the problem as it then stands."""
    c, k = w.ctx, P.N - SHAPES[P.name.split("/")[0]].N
    rng = np.random.default_rng(1000 + k)
    x = rng.random(P.d)
    y, y2, y3 = (np.array([R._smooth(x[None], ph)[0]]) for ph in (0.0, 1.9, 4.1))
    R.setup(w.env(P))
    rows = [1, P.M // 2, P.M]
    c.grid_remove_rows(rows)
    c.gp_fit_hyp(**P.hyps[0])
    try:
        c.gp_append(x, y)
    except Bot7HipError as e:   # the padded factor is full (C on its way past N = Npad = 128): "refit", as the bots then do
        assert e.code == R.STATE and P.N == 128, str(e)
        c.gp_set_data(np.vstack([P.X, x]), np.vstack([P.Y, y[None]]))
    Q = R.derived(P, np.vstack([P.X, x]), np.vstack([P.Y, y[None]]), np.append(P.Y2, y2), np.append(P.Y3, y3),
                  np.delete(P.G, np.array(rows) - 1, axis=0), "between%d" % (k + 1))
    for p, yy in ((w.p2, Q.Y2), (w.p3, Q.Y3)):
        p.grid_upload(Q.G)
        p.gp_set_data(Q.X, yy)
    return Q


ORDERS, ORDER_SHAPES = ("reverse", "permutation", "between"), ("C", "B")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", ORDER_SHAPES)
def test_d_order_of_policies(walker, shape, order):
    names = list(R.CALLS)
    if order == "reverse":
        names = names[::-1]
    elif order == "permutation":
        names = [names[i] for i in np.random.default_rng(20261020).permutation(len(names))]
    walker.step("%s %s" % (shape, order), SHAPES[shape], names=names, between=_between if order == "between" else None)
    assert walker.compared == len(R.CALLS)


# ---- e. growth by one
GROWTH = (62, 126)   # N runs n0 .. n0 + 4: across Npad 64 -> 128 and 128 -> 256


@pytest.mark.parametrize("n0", GROWTH)
def test_e_growth_by_one_across_a_padding_boundary(walker, n0):
    pool = R.problem(n0 + 4, 6, 200, 2, seed=40 + n0, q=2, name="grow%d" % n0)
    c, G = walker.ctx, pool.G
    c.gp_set_opts()
    c.grid_upload(G)
    for N in range(n0, n0 + 5):
        P = R.derived(pool, pool.X[:N], pool.Y[:N], pool.Y2[:N], pool.Y3[:N], G, "N=%d" % N)
        c.gp_set_data(P.X, P.Y)   # as the bots do: the data anew every trial, the grid resident
        for name in ("eval_nominate[ei,S]", "eval_nominate[mes,S]", "eval_nominate_batch"):
            got = R.run_call(name, walker.env(P))
            walker.compare("N=%d" % N, P, name, got)
        idx = int(np.frombuffer(got["idx"], dtype=np.int64)[0])
        row, _ = c.nominate_commit(idx, 0)   # the grid loses the nominee
        assert np.array_equal(row, G[idx - 1])
        G = np.delete(G, idx - 1, axis=0)
    assert walker.compared == 15


# ---- f. a group of two members on device 0
def _group_round(g, P):
    out = {}
    g.grid_upload(P.G)
    g.gp_set_data(P.X, P.Y)
    for kind in ("ei", "cb", "logei", "logpi"):
        v, i, rep = g.eval_nominate(P.hyps, score=kind, fmin=P.fmin, want_report=True)
        row = g.nominate_commit(i)
        out[kind] = (R._b(v), int(i), R._b(rep["jitter"]), R._b(rep["info"], np.int32), R._b(row), R._b(g.grid_download()))
    return out


def test_f_a_reused_group_equals_a_fresh_group():
    g = bot7_amd.Group([0, 0])
    try:
        _group_round(g, BIG)
        got = {name: _group_round(g, SHAPES[name]) for name in ("A", "B")}
    finally:
        g.close()
    for name in ("A", "B"):
        f = bot7_amd.Group([0, 0])
        try:
            want = _group_round(f, SHAPES[name])
        finally:
            f.close()
        for kind in want:
            assert got[name][kind] == want[kind], "group, step %s, eval_nominate[%s] + nominate_commit differs from a fresh group" % (name, kind)
            assert np.isfinite(np.frombuffer(want[kind][0], dtype=np.float64)).all()
            TOTALS["compared"] += 1


# ---- g. what a mutator forgets
# The mark of (mutator, reader): "state" -- the reader refuses with B7_ERR_STATE; "last" -- it returns the bytes it returned before
# the mutator (the last call's result, kept on purpose); "fresh" -- it computes anew from kept state that is still valid, and must
# equal a new context given the grid, data and options as they stand; "row" -- nominate_commit returns the row the index names
# in the grid as it stands (its cache of the winner's row is dropped by every grid change).  Never the old content under the new shape.
READERS = ("gp_predict", "score_finish", "feas_get", "feas_nominate", "posterior_get", "ehvi_nominate", "blr_predict", "mes_last_ystar",
           "ts_last_paths", "kg_last", "refine_last", "nominate_commit")
_GRID = dict(gp_predict="fresh", score_finish="state", feas_get="state", feas_nominate="state", posterior_get="state", ehvi_nominate="state",
             blr_predict="state", mes_last_ystar="last", ts_last_paths="last", kg_last="last", refine_last="last", nominate_commit="row")
_KEEP = dict(_GRID, gp_predict="last", score_finish="last", feas_get="last", feas_nominate="last", posterior_get="last", ehvi_nominate="last",
             blr_predict="last")
TABLE = {
    "grid_upload": _GRID, "grid_remove": _GRID, "grid_remove_rows": _GRID, "grid_sobol": _GRID, "grid_trust_region": _GRID,
    "grid_apply_onesided": _GRID,
    # new data: the fit, the predictions and a kept posterior were of the old data; the accumulator survives (marginalisation adds across fits)
    "gp_set_data": dict(_KEEP, gp_predict="state", posterior_get="state", ehvi_nominate="state", blr_predict="state"),
    # the fit is extended in place: predict computes anew; on a head gp_append itself refuses and changes nothing
    "gp_append": dict(_KEEP, gp_predict="fresh", posterior_get="state", ehvi_nominate="state"),
    # decided here (include/bot7hip.h): another kernel drops the fit, the predictions AND a kept posterior
    "gp_set_kernel": dict(_KEEP, gp_predict="state", posterior_get="state", ehvi_nominate="state", blr_predict="state"),
    # decided here (include/bot7hip.h): options are of the calls that follow; a kept posterior stays as it was made
    "gp_set_opts": dict(_KEEP, gp_predict="fresh", blr_predict="fresh"),
    "mes_set_levels": _KEEP,
}
OPTS = dict(var_with_noise=1, var_clamp=1, var_min=1e-12)


def _mutate(c, name, P):
    if name == "grid_upload":
        c.grid_upload(P.G[::-1][:P.M - 7])
    elif name == "grid_remove":
        c.grid_remove(5)
    elif name == "grid_remove_rows":
        c.grid_remove_rows([1, 9, P.M])
    elif name == "grid_sobol":
        c.grid_sobol(P.M - 20, P.d, skip=2, download=False)
    elif name == "grid_trust_region":
        c.grid_trust_region(np.full(P.d, 0.5), np.full(P.d, 0.25), np.full(P.d, 0.75), 0.5, seed=1)
    elif name == "grid_apply_onesided":
        c.grid_apply_onesided(mins=np.full(P.d, 0.25), col_ext=-c.grid_colrange()[0])
    elif name == "gp_set_data":
        c.gp_set_data(P.X[:P.N - 3], P.Y[:P.N - 3])
    elif name == "gp_append":
        try:
            c.gp_append(P.x_new, P.y_new)
        except Bot7HipError as e:   # on a head: refused, nothing changes
            assert e.code == R.STATE
    elif name == "gp_set_kernel":
        c.gp_set_kernel("ardmatern52")
    elif name == "gp_set_opts":
        c.gp_set_opts(**OPTS)
    else:
        c.mes_set_levels(5)


def _read(c, reader, P, front_ref, idx=None):
    if reader == "gp_predict":
        mu, var = c.gp_predict()
        return {"mean": R._b(mu), "var": R._b(var)}
    if reader == "blr_predict":
        mu, var = c.blr_predict()
        return {"mean": R._b(mu), "var": R._b(var)}
    if reader == "score_finish":
        return R._acc(c)
    if reader == "feas_get":
        return {"column": R._b(c.feas_get())}
    if reader == "feas_nominate":
        v, i = c.feas_nominate()
        return {"value": R._b(v), "idx": int(i)}
    if reader == "posterior_get":
        mu, var = c.posterior_get(P.S - 1)
        return {"mean": R._b(mu), "var": R._b(var)}
    if reader == "ehvi_nominate":
        v, i = c.ehvi_nominate(c, *front_ref)
        return {"value": R._b(v), "idx": int(i)}
    if reader == "mes_last_ystar":
        ys, br = c.mes_last_ystar()
        return {"ystar": R._b(ys), "bracket": R._b(br)}
    if reader == "ts_last_paths":
        return {"paths": R._b(c.ts_last_paths())}
    if reader == "kg_last":
        return {k: R._b(v, np.int64 if k == "rows" else np.float64) for k, v in c.kg_last().items()}
    if reader == "refine_last":
        last = c.refine_last()
        return {"x": R._b(last["x"]), "val": R._b(last["val"]), "idx": R._b(last["start_idx1"], np.int64), "status": R._b(last["status"], np.int32)}
    row, off = c.nominate_commit(idx, 0)
    return {"row": R._b(row), "offset": int(off)}


def _try(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Bot7HipError as e:
        return ("refused", e.code, str(e))


def _gp_scenario(c, P, upto_fit=False):
    """Every piece of kept state a GP context can hold, each made by its own call; returns the index of the last exchange's winner."""
    c.gp_set_opts()
    c.grid_upload(P.G)
    c.gp_set_data(P.X, P.Y)
    if not upto_fit:
        c.ts_nominate(P.hyps, 2, n_features=64, seed=7)
        c.kg_nominate(P.hyps, points=4)
        c.eval_nominate_refine(P.hyps, score="ei", fmin=P.fmin, starts=4, iters=4)
        c.eval_nominate(P.hyps, score="mes")
        c.feas_reset()
        c.feas_add(P.logw)
        c.eval_posterior(P.hyps)
    c.gp_fit_hyp(**P.hyps[0])
    c.gp_predict(download=False)
    c.score_reset()
    c.score_ei(P.fmin, 0.0)
    return c.score_finish_global(1.0, 0)[1]


@pytest.mark.parametrize("mutator", sorted(TABLE))
def test_g_what_a_mutator_forgets(mutator):
    P = A
    front_ref = (np.array([[float(np.median(P.Y)), float(np.median(P.Y))]]), np.array([P.Y.max() + 1.0, P.Y.max() + 1.0]))
    marks = TABLE[mutator]
    assert sorted(marks) == sorted(READERS)
    for scenario in ("gp", "head"):
        readers = [r for r in READERS if (r == "blr_predict") == (scenario == "head")]
        c = bot7_amd.Context(0)
        try:
            if scenario == "gp":
                idx = _gp_scenario(c, P)
            else:
                c.grid_upload(P.G)
                c.blr_fit_x(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr)
                c.blr_basis(P.net[0], P.net[1], "Tanh")
            before = {}
            for r in readers:   # ehvi_nominate writes the accumulator: read it first, then score again for score_finish
                if r in ("posterior_get", "ehvi_nominate"):
                    before[r] = _read(c, r, P, front_ref)
            if scenario == "gp":
                c.score_reset()
                c.score_ei(P.fmin, 0.0)
            for r in readers:
                if r not in before and r != "nominate_commit":
                    before[r] = _read(c, r, P, front_ref)
            _mutate(c, mutator, P)
            grid_now = c.grid_download()
            for r in readers:
                mark, after = marks[r], _try(_read, c, r, P, front_ref, idx if scenario == "gp" else None)
                where = "%s then %s (%s)" % (mutator, r, mark)
                if mark == "state":
                    assert R.is_refusal(after) and after[1] == R.STATE, "%s: %r" % (where, after if R.is_refusal(after) else "a result")
                elif mark == "last":
                    assert not R.is_refusal(after), "%s: %r" % (where, after)
                    assert R.first_difference(after, before[r]) is None, "%s: %s" % (where, R.first_difference(after, before[r]))
                elif mark == "row":
                    if idx <= grid_now.shape[0]:
                        assert not R.is_refusal(after) and after["row"] == R._b(grid_now[idx - 1]), "%s: not the row of the grid as it stands" % where
                    else:
                        assert R.is_refusal(after) and after[1] == R.INVALID, where
                else:
                    f = bot7_amd.Context(0)
                    try:
                        if mutator == "gp_set_opts":
                            f.gp_set_opts(**OPTS)
                        f.grid_upload(grid_now)
                        if r == "gp_predict":
                            f.gp_set_data(P.X, P.Y)
                            f.gp_fit_hyp(**P.hyps[0])
                            if mutator == "gp_append":
                                f.gp_append(P.x_new, P.y_new)
                        else:
                            f.blr_fit_x(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr)
                            f.blr_basis(P.net[0], P.net[1], "Tanh")
                        want = _read(f, r, P, front_ref)
                    finally:
                        f.close()
                    assert not R.is_refusal(after), "%s: %r" % (where, after)
                    assert R.first_difference(after, want) is None, "%s: %s" % (where, R.first_difference(after, want))
                    assert R.all_finite(want) == []
                TOTALS["compared"] += 1
        finally:
            c.close()


# ---- h. the believer's per-sample downdated variances (the diagnostic build exposes them: b7dbg_believer_var)
def _diag_context():
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_believer_var.restype = ctypes.c_int
    c._L.b7dbg_believer_var.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return c


def _batch_and_variances(c, P):
    """The catalogue's eval_nominate_batch entry, then every sample's variance over the grid as the last downdate left it: the
    believer's S x M store is a grow-only buffer whose slot stride follows M and S."""
    res = R.run_call("eval_nominate_batch", R.Env(c, None, None, P))
    assert not R.is_refusal(res), res
    for s in range(P.S):
        var = np.empty(P.M, dtype=np.float64)
        assert c._L.b7dbg_believer_var(c._h, P.S, s, var.ctypes.data) == 0
        res["var%d" % s] = var.tobytes()
    return res


BELIEVER_STEPS = ("A", "C", "B")


def test_h_the_believer_variances_of_every_sample_equal_a_fresh_context():
    w = _diag_context()
    try:
        R.Walker(lambda: (w, None, None), None).fill(BIG, [n for n in R.CALLS if n not in R.PARTNERED])   # the poison, q = 16, S = 4
        for name in BELIEVER_STEPS:
            P = SHAPES[name]
            R.setup(R.Env(w, None, None, P))
            got = _batch_and_variances(w, P)
            f = _diag_context()
            try:
                R.setup(R.Env(f, None, None, P))
                want = _batch_and_variances(f, P)
            finally:
                f.close()
            diff = R.first_difference(got, want)
            assert diff is None, "step %r after BIG, eval_nominate_batch + variances: %s" % (name, diff)
            assert R.all_finite(want) == [] and sorted(k for k in want if k.startswith("var")) == ["var%d" % s for s in range(P.S)]
            TOTALS["compared"] += 1
    finally:
        w.close()


# what the parametrisations above make: the tests ahead of test_z, and the pairs they compare
N_TESTS = len(TARGETS) + 1 + len(TRANSITIONS) + len(ORDER_SHAPES) * len(ORDERS) + len(GROWTH) + 1 + len(TABLE) + 1
EXPECTED_PAIRS = ((len(TARGETS) + 2 + sum(len(t) for t in TRANSITIONS.values()) + len(ORDER_SHAPES) * len(ORDERS)) * len(R.CALLS)   # a, b, c, d
                  + len(GROWTH) * 15 + 8 + len(TABLE) * len(READERS) + len(BELIEVER_STEPS))                                          # e, f, g, h


def test_z_the_count_of_compared_pairs_and_the_expected_refusals(request):
    """Runs last in the file: what the tests above compared, printed (pytest -s shows it), and the refusals met held to the
    enumerated set: MES on the head's one-call routes and KG / MES / the believer asked of a head, at every shape; the slice
    sampler past the small regime (B, D, and C once the appends of test d have taken it past N = 128); the one-column routes at E.
    When the whole file was selected the set and the count are held exactly; a run of a part of it (-k, a node id) holds the subset."""
    selected = [it for it in request.session.items if it.fspath == request.node.fspath and it is not request.node]
    assert TOTALS["tests"] == len(selected), "tests of this file ran after test_z, or not at all"
    cfg = request.config
    part_asked = bool(cfg.getoption("keyword") or cfg.getoption("deselect") or any("::" in a for a in cfg.args))
    whole_file = len(selected) == N_TESTS
    assert len(selected) <= N_TESTS if part_asked else whole_file, \
        "%d tests of this file were selected, N_TESTS says %d: a test was added or removed without its share of N_TESTS / EXPECTED_PAIRS" % (len(selected), N_TESTS)
    refused = sorted(TOTALS["refused"])
    print("\ncompared (step, call) pairs: %d; expected-refusal set: %d entries" % (TOTALS["compared"], len(refused)))
    for r in refused:
        print("  refused: %s %s (%d)" % r)
    want = {(P.name, n, R.expected_refusal(n, P)) for P in (A, B, C, D, E, F, J, A_MATERN) for n in R.CALLS if R.expected_refusal(n, P) is not None}
    want.add(("C", "gp_slice_sample", R.UNSUPPORTED))
    assert set(refused) <= want, sorted(set(refused) - want)
    if whole_file:
        assert set(refused) == want, sorted(want - set(refused))
        assert TOTALS["compared"] == EXPECTED_PAIRS
