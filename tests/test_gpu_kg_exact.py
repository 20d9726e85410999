"""b7_kg_nominate's lines held to EXACT arithmetic, given the device's own W = inv(K) k(X, a_i) (diagnostic build:
b7dbg_kg_operands) and its own posterior; kcol held entry by entry against 50 digits and W by its residual, with the reported
jitter; every route that hands the fits to kg_kernel held to route B's bits; and the rules (the rows of A, the nominee) held bit
for bit on the device's own output, NaN rows, exact ties and a second lap of the grid-stride loop included.  Needs an MI355X: run
with -m gpu.

Reference and bars: tests/_kg_ref.py (lines_exact), checked on the CPU by tests/test_kg_exact_host.py.  Per judged row x and line
i: c_i = k(x, a_i) - sum_j k(x, x_j) W_ji from 50-digit covariances of exact arguments, error-free products and exact sums; b_i =
c_i / sqrt(t), b_0 = var / sqrt(t), t = var + fl(noise + jitter) at 50 digits, var the device's own (b7_eval_posterior on the
same hyper samples: tests/test_gpu_ehvi.py holds it bit for bit to the per-sample predict).  Bars: gp_bar(numpy's own float64
error on the same operands) + the first-order K* terms, over sqrt(t), + 4 u |b| for the add, the square root and the division;
below 1e-9 of the scale on every row.  Every judged row is judged.  Each test prints its figures; DESIGN.md section 8 carries
the MI355X table."""
import ctypes as C

import numpy as np
import pytest

import _kg_ref as R
import _post_ref as PR

pytestmark = pytest.mark.gpu


def _diag_context():
    import bot7_amd
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_kg_operands.restype = C.c_int
    c._L.b7dbg_kg_operands.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    return c


@pytest.fixture(scope="module")
def dctx():
    """The diagnostic build: b7dbg_kg_operands (kcol and W of the last nomination) exists there only."""
    c = _diag_context()
    yield c
    c.close()


def kg_operands(c, S, N):
    """(kcol, W), [KL][S][Npad] each, of the last kg_nominate."""
    npad = PR.npad_of(N)
    kcol, W = np.empty((R.KL, S, npad)), np.empty((R.KL, S, npad))
    assert c._L.b7dbg_kg_operands(c._h, kcol.ctypes.data, W.ctypes.data) == 0
    return kcol, W


def stage(c, X, y, Xc, kern):
    c.gp_set_kernel(kern)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def fold(values):
    acc = values[0].copy()
    for s in range(1, len(values)):
        acc = acc + values[s]
    return acc / float(len(values))


def lines_of(last, s):
    M, n = last["values"].shape[1], last["alpha"].shape[1]
    a = np.empty((M, n + 1))
    a[:, 0], a[:, 1:] = last["own_alpha"][s], last["alpha"][s][None, :]
    return a, last["slopes"][s]


def run(c, hyps, arows):
    """The kept posterior of the same hyper samples, then the nomination with the caller's rows and the slopes kept."""
    S = len(hyps)
    prep = c.eval_posterior(hyps, want_report=True)
    post = [c.posterior_get(s) for s in range(S)]
    val, idx, rep = c.kg_nominate(hyps, rows=arows + 1, want_report=True, trace=True)
    assert np.array_equal(prep["jitter"], rep["jitter"]), (prep, rep)
    return val, idx, rep, post, c.kg_last(slopes=True)


def hold(tag, c, X, Xc, hyps, kern, arows, rows, val, idx, rep, post, last):
    """One nomination's alpha, slopes, kcol and W against the references, every hyper sample; its values against b7_kg_compute of
    its own lines and its nominee against the fold's arg-max, bit for bit."""
    S, N, n, M = len(hyps), len(X), len(arows), len(Xc)
    kcol, W = kg_operands(c, S, N)
    assert last["rows"].tolist() == (arows + 1).tolist()
    own = ~np.isin(rows, arows)
    jit = np.where(rep["jitter"] > 0.0, rep["jitter"], 0.0)
    for s, h in enumerate(hyps):
        mu, var = post[s]
        assert last["own_alpha"][s].tobytes() == mu.tobytes() and last["alpha"][s].tobytes() == mu[arows].tobytes()
        tnoise = h["noise"] + float(jit[s])
        Ws, ks = W[:n, s, :N].T, kcol[:n, s, :N].T
        assert not kcol[:n, s, N:].any()                               # the padding rows of the n live columns (the others are not written)
        ref = R.lines_exact(X, Xc[rows], Xc[arows], h, kern, Ws, var[rows], tnoise)
        sl = last["slopes"][s]
        assert np.isfinite(sl[:, 1:]).all() and np.isnan(sl[arows, 0]).all() and np.isfinite(np.delete(sl[:, 0], arows)).all()
        rb, r0 = R.judge_lines(ref, sl[rows], own)
        rk = R.kcol_ratio(X, Xc[arows], h, kern, ks)
        res, bound = R.w_residual(X, h, kern, tnoise, ks, Ws)
        err = R.E.abs_errors(sl[rows][:, 1:], *ref.b)
        print("%s sample %d: %d rows x %d lines: worst error / bar slopes %.3f (error %.1f u scale) own line %.3f kcol %.3f; W residual / "
              "bound %.3g; K* share of the bar %.2f; e_np %.1f u scale; bar / scale <= %.1e; jitter %.3g" % (
                  tag, s, len(rows), n, rb.max(), np.max(err / ref.scale) / R.U, r0.max(), rk.max(), np.max(res / bound),
                  np.median(ref.share), ref.e_np_u, ref.cap, jit[s]))
        assert ref.cap <= R.CAP, tag
        assert np.all(rb <= 1.0) and np.all(r0 <= 1.0), (tag, s, rows[~(rb.max(axis=1) <= 1.0)].tolist(), rows[~(r0 <= 1.0)].tolist())
        assert np.all(rk <= 1.0), (tag, s, "kcol", float(rk.max()))
        assert np.all(res <= bound), (tag, s, "W", float(np.max(res / bound)))
        assert c.kg_compute(*lines_of(last, s)).tobytes() == last["values"][s].tobytes()
    marg = fold(last["values"])
    assert idx - 1 == R.nominee_ref(marg) and np.float64(val).tobytes() == marg[idx - 1].tobytes()


@pytest.mark.parametrize("N,d,kern,n,S,M", R.EXACT_CASES, ids=["%d-%d-%s-n%d-S%d-M%d" % c for c in R.EXACT_CASES])
def test_lines_against_exact_arithmetic(dctx, N, d, kern, n, S, M):
    """The shapes of test_gpu_kg.test_slopes_against_long_double (both regimes, Npad 64 .. 384) and one per dpad class of kg_slab at
    N = 24 (d = 3, 12, 24, 40, 60, 96); n in {1, 5, 16}, M in {200, 257}, S in {1, 2, 3}.  No jitter."""
    X, y, Xc, hyps, arows, rows = R.exact_problem(N, d, M, S, n)
    try:
        stage(dctx, X, y, Xc, kern)
        val, idx, rep, post, last = run(dctx, hyps, arows)
        assert not rep["jitter"].any() and not rep["info"].any(), rep
        hold("N %d d %d %s n %d S %d M %d" % (N, d, kern, n, S, M), dctx, X, Xc, hyps, kern, arows, rows, val, idx, rep, post, last)
    finally:
        dctx.gp_set_kernel("ardse")


def _counted(c, hyps, arows, N):
    c.profile_enable(True)
    try:
        c.profile_reset()
        val, idx = c.kg_nominate(hyps, rows=arows + 1, trace=True)
        counts = {ph: c.profile_get(ph)[1] for ph in ("kxx", "ksx", "post", "kpost")}
    finally:
        c.profile_enable(False)
    S = len(hyps)
    kcol, W = kg_operands(c, S, N)
    return val, idx, c.kg_last(slopes=True), kcol, W, counts


def test_routes_b_c_d_give_the_same_bits(dctx, monkeypatch):
    """General layout (N = 150: Npad 256), d = 5, S = 3, n = 16 -- tests/test_gpu_believer_routes.py's routes into BelKeep, which
    the knowledge gradient takes its fits and posteriors through.  B: side-by-side fits, K* of all samples in the workspace.  C: the
    same fits, then the posterior one sample after the other because the workspace (128 KiB, the minimum) does not hold K*.  D: a
    context on the launch schedule (B7_POTRF_SCHED=1), which fits one sample after the other into the context's own slot;
    keep_sample copies every fit to its batch slot.  The phase counters say which ran.  B is held to the bars; rows, alpha, slopes,
    values, kcol, W and the nominee of C and D to B's bits."""
    N, d, kern, n, S, M = R.ROUTES_CASE
    X, y, Xc, hyps, arows, rows = R.exact_problem(N, d, M, S, n)
    stage(dctx, X, y, Xc, kern)
    val, idx, rep, post, last = run(dctx, hyps, arows)
    assert not rep["jitter"].any()
    hold("route B", dctx, X, Xc, hyps, kern, arows, rows, val, idx, rep, post, last)
    vb, ib, lb, kb, Wb, nb = _counted(dctx, hyps, arows, N)
    assert nb["kxx"] == 1 and nb["post"] == 1 and nb["kpost"] == 0, nb
    assert (vb, ib) == (val, idx) and all(lb[k].tobytes() == last[k].tobytes() for k in last)
    dctx.set_workspace(128 << 10)
    try:
        vc, ic, lc, kc, Wc, nc = _counted(dctx, hyps, arows, N)
    finally:
        dctx.set_workspace(PR.WORKSPACE_DEFAULT)
    assert nc["kxx"] == 1 and nc["post"] >= S and nc["ksx"] >= S and nc["kpost"] == 0, nc
    monkeypatch.setenv("B7_POTRF_SCHED", "1")
    cd = _diag_context()
    monkeypatch.delenv("B7_POTRF_SCHED")
    try:
        stage(cd, X, y, Xc, kern)
        vd, idd, ld, kd, Wd, nd = _counted(cd, hyps, arows, N)
    finally:
        cd.close()
    assert nd["kxx"] == S and nd["post"] == S and nd["kpost"] == 0, nd
    for name, v, i, l, k, W in (("C", vc, ic, lc, kc, Wc), ("D", vd, idd, ld, kd, Wd)):
        print("route %s against route B: nominee %d / %d, worst |dslope| %.3e, worst |dW| %.3e" % (
            name, i, ib, np.nanmax(np.abs(l["slopes"] - lb["slopes"])), np.max(np.abs(W[:n] - Wb[:n]))))
        assert (v, i) == (vb, ib), name
        for key in ("rows", "alpha", "own_alpha", "slopes", "values"):
            assert l[key].tobytes() == lb[key].tobytes(), (name, key)
        assert k[:n].tobytes() == kb[:n].tobytes() and W[:n].tobytes() == Wb[:n].tobytes(), name


@pytest.mark.parametrize("name", sorted(R.REDO))
def test_route_e_the_jitter_redo_carries_the_jitter(dctx, name):
    """Duplicated observations with noise = 0 under the second hyper sample, in the small regime, the general layout and the
    general layout reached by d = 33: the nomination is redone through the jitter schedule.  That sample's t(x) must be var + the
    REPORTED jitter and its W must solve (K + jitter I) W = kcol: the lines against exact arithmetic with t so formed (a t without
    the jitter leaves every own line's bar: tests/test_kg_exact_host.py), and the residual of W with the jitter on the diagonal
    (without it the residual exceeds 10 x the bound, asserted here too).  The other samples report none and are held as usual."""
    N, d, S = R.REDO[name]
    X, y, Xc, hyps, arows, rows = R.exact_problem(N, d, 200, S, 5, dup=3)
    stage(dctx, X, y, Xc, "ardse")
    val, idx, rep, post, last = run(dctx, hyps, arows)
    assert rep["jitter"][1] > 0.0 and rep["info"][1] > 0, rep
    assert not np.delete(rep["jitter"], 1).any() and not np.delete(rep["info"], 1).any(), rep
    hold("route E %s" % name, dctx, X, Xc, hyps, "ardse", arows, rows, val, idx, rep, post, last)
    kcol, W = kg_operands(dctx, S, N)
    res0, bound = R.w_residual(X, hyps[1], "ardse", 0.0, kcol[:5, 1, :N].T, W[:5, 1, :N].T)
    print("route E %s: without the jitter the residual of W is %.3g x its bound" % (name, np.min(res0 / bound)))
    assert np.all(res0 > 10.0 * bound)


@pytest.mark.parametrize("M,n", [(7, 5), (1037, 16), (262144 + 300, 16)])
def test_the_rules_on_nan_rows_ties_and_a_second_lap(dctx, M, n):
    """N = 5, d = 3, S = 2, rows = None.  One grid row carries a NaN coordinate; the row of the lowest folded mean is copied to
    a lower and to a higher index (at the largest M beyond row 262 144, where nblk = 1024 blocks of 256 make kg_rows_part_kernel's
    grid-stride loop take a second lap).  The chosen rows are the n lowest of the folded own_alpha by the kernel's rule -- lowest
    mean, then lower index, a NaN counting as +inf --, on the device's own means, bit for bit; the NaN row's value is NaN, and
    that row is the nominee (the first NaN wins)."""
    N, d, S = 5, 3, 2
    X, y, _, hyps, _, _ = R.exact_problem(N, d, 200, S, 1)
    G = np.random.default_rng(M + 1).random((M, d))
    nan_row = M - 3
    G[nan_row, 1] = np.nan
    stage(dctx, X, y, G, "ardse")
    dctx.kg_nominate(hyps, points=n)
    first = dctx.kg_last()
    r0 = int(first["rows"][0]) - 1
    assert r0 != nan_row and np.isnan(first["own_alpha"][:, nan_row]).all()
    lowc = 0 if r0 != 0 else 1
    highc = (M - 1 if r0 != M - 1 else M - 2) if M <= 262144 else 262144 + 5
    G[lowc], G[highc] = G[r0], G[r0]
    dctx.grid_upload(G)
    val, idx = dctx.kg_nominate(hyps, points=n)
    last = dctx.kg_last()
    mu = last["own_alpha"]
    assert mu[:, lowc].tobytes() == mu[:, r0].tobytes() == mu[:, highc].tobytes()
    want = R.lowest_rows(mu, n)
    assert (last["rows"] - 1).tolist() == want.tolist() and want[0] == min(lowc, r0) and nan_row not in want
    assert {lowc, r0, highc} <= set(want.tolist()) or n < 3
    for s in range(S):
        assert last["alpha"][s].tobytes() == mu[s][want].tobytes()
    marg = fold(last["values"])
    assert np.isnan(last["values"][:, nan_row]).all() and np.isfinite(np.delete(marg, nan_row)).all()
    assert idx - 1 == nan_row == R.nominee_ref(marg) and np.isnan(val)
