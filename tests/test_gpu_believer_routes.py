"""b7_eval_nominate_batch's later picks on every kernel instance, at q = B7_BATCH_MAX, on every route that hands pick 1's fits to
the believer, and at the grid's edges -- against the 50-digit refit of tests/_believer_ref.believer_truth.

Bars.  On the probe rows (all of block 0, the last block's tail, every picked row and its nearest neighbour in the grid), wherever
the observations number at most 40 (the truth's cost): |var_dev - truth| <= gp_bar(err_ref, amp) = 8 err_ref + 16 eps amp, err_ref
the error of the float64 refit (_believer_ref.refit) against the same truth on the same rows.  On the whole grid, every case:
|var_dev - var_refit64| <= 1e-5 amp.  The pick sequence is _believer_ref.greedy's, and at every pick the
reference's top-2 gap must exceed 1000 x the achieved score error (device accumulator against the float64 restatement), else the
test fails; pick 1 is held to the same rule.  The variance left by the q-pick call holds the q - 1 believed rows before its last
pick; "after pick j" below is the state the j-pick prefix call leaves.

The seeds were chosen on the CPU with _believer_ref.greedy alone (the best of seeds 1..12, of 1..24 for q = 16 and M <= 16).
Smallest absolute top-2 gap of the reference over picks 1..q of each case (the tests print every pick's):
  every instance (q = 3, 14 cases)             >= 4.7e-3 (d = 96, ARD-SE, EI)
  q = 16: small regime EI / LogEI              9.7e-4 / 1.9e-1 (scores of magnitude 5e2)        general layout, CB   2.2e-3
  routes B / C / D (q = 4, EI)                 7.0e-4
  jitter redo, small / general / wide          8.1e-2 / 4.9e-2 / 3.1e-2   (found with the schedule's first step, 1.1e-8, as jitter)
  grid edges                                   >= 3.4e-3 (M = 65, small regime); M = 16 under CB and M = 5 under LogEI, because EI
                                               underflows on grids that small once most rows are believed (gaps of 1e-79)
  sequence                                     q = 16's problems
No case had to shorten its q."""
import ctypes as C

import numpy as np
import pytest

import _believer_ref as R
import _exact as E

pytestmark = pytest.mark.gpu


def problem(N, d, M, S, seed, dup=0):
    """tests/test_gpu_believer.py's problem at given sizes; dup > 0 repeats the first dup observations at the end."""
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    if dup:
        X[N - dup:] = X[:dup]
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rng.standard_normal(N)
    if dup:
        y[N - dup:] = y[:dup]
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.05 * s} for s in range(S)]
    return X, y.reshape(-1, 1), Xc, hyps


def spec_of(kind, y):
    if kind == "cb":
        return {"score": "cb", "tradeoff": 1.0, "upper": False, "sign": -1.0}
    return {"score": kind, "fmin": [float(y.min())], "tradeoff": 0.0}


def ref_spec(kind, y):
    return {"tradeoff": 1.0, "upper": False, "sign": -1.0} if kind == "cb" else {"fmin": float(y.min()), "tradeoff": 0.0}


def _diag_context():
    import bot7_amd
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_believer_var.restype = C.c_int
    c._L.b7dbg_believer_var.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return c


@pytest.fixture(scope="module")
def dctx():
    """The diagnostic build: b7dbg_believer_var (the per-sample downdated variances) exists there only."""
    c = _diag_context()
    yield c
    c.close()


def believer_var(c, S, s, M):
    out = np.empty(M, dtype=np.float64)
    assert c._L.b7dbg_believer_var(c._h, S, s, out.ctypes.data) == 0
    return out


def all_vars(c, S, M):
    return np.stack([believer_var(c, S, s, M) for s in range(S)])


def stage(c, X, y, Xc, kernel):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def probe_rows(Xc, picks0):
    """All of block 0, the last block's partial tail (its last 8 rows where the grid ends on a block edge), every picked row and
    each one's nearest neighbour in the grid."""
    M = len(Xc)
    tail = 64 * ((M - 1) // 64)
    rows = set(range(min(64, M))) | set(range(tail if M % 64 else max(0, M - 8), M)) | set(picks0)
    for p in picks0:
        if M > 1:
            dist = np.sum((Xc - Xc[p]) ** 2, axis=1)
            dist[p] = np.inf
            rows.add(int(np.argmin(dist)))
    return sorted(rows)


def check_case(c, label, X, y, Xc, hyps, kernel, kind, q, after, jitter_from_report=False):
    """One problem on the staged context c: the q-pick call; the pick sequence against greedy; every prefix call's bits, score
    error and top-2 gap; the variances after the picks `after` against the float64 refit (whole grid) and, N <= 40, against the
    50-digit truth (probe rows).  Returns (values, indices, every sample's variance after the last pick, the report)."""
    S, M, N = len(hyps), len(Xc), len(X)
    sp = spec_of(kind, y)
    v1, i1 = c.eval_nominate(hyps, **sp)
    got1 = c.score_finish(1.0, download=True)[2]                    # pick 1's marginal score, before the batch call rewrites it
    vq, iq, rep = c.eval_nominate_batch(hyps, q, want_report=True, **sp)
    assert vq[0].tobytes() == np.float64(v1).tobytes() and iq[0] == i1
    assert len(set(iq.tolist())) == q and iq.min() >= 1 and iq.max() <= M
    jit = np.where(rep["jitter"] > 0.0, rep["jitter"], 0.0) if jitter_from_report else np.zeros(S)
    if not jitter_from_report:
        assert not rep["jitter"].any() and not rep["info"].any()
    rhyps = [dict(h, noise=h["noise"] + float(jit[s])) for s, h in enumerate(hyps)]   # what went on the diagonal that was factored
    rp, rs, rg, _ = R.greedy(X, y, Xc, rhyps, kernel, q, kind, "downdate", **ref_spec(kind, y))
    assert [p + 1 for p in rp] == iq.tolist(), (label, rp, iq)
    err1 = float(np.max(np.abs(got1 - rs[0])))
    print("%s pick 1: |dscore| %.3e (scale %.3e)  top-2 gap %.3e" % (label, err1, float(np.max(np.abs(rs[0]))), rg[0]))
    assert rg[0] > 1000.0 * err1, "%s pick 1: top-2 gap %.3e within 1000 x the score error %.3e" % (label, rg[0], err1)
    assert v1 == got1[i1 - 1]
    rows0 = [int(i) - 1 for i in iq]
    probes = probe_rows(Xc, rows0)
    truths = None
    if N <= 40:
        truths = [R.believer_truth(X, y, Xc, h, kernel, rows0[:q - 1], probes, after=[j - 1 for j in after], jitter=float(jit[s]))
                  for s, h in enumerate(hyps)]
    worst_dev = worst_ref = 0.0
    last_var = None
    for j in range(2, q + 1):                                       # the j-pick prefix call: its last pick is pick j of the batch
        vj, ij = c.eval_nominate_batch(hyps, j, **sp)
        assert vj.tobytes() == vq[:j].tobytes() and np.array_equal(ij, iq[:j]), (label, j)
        got = c.score_finish(1.0, download=True)[2]                 # the accumulator: pick j's marginal score
        want = rs[j - 1]
        err_abs = float(np.max(np.abs(got - want)))
        gap = rg[j - 1]
        print("%s pick %d: |dscore| %.3e (scale %.3e)  top-2 gap %.3e" % (label, j, err_abs, float(np.max(np.abs(want))), gap))
        assert gap > 1000.0 * err_abs, "%s pick %d: top-2 gap %.3e within 1000 x the score error %.3e" % (label, j, gap, err_abs)
        assert vq[j - 1] == got[iq[j - 1] - 1]
        if j not in after:
            continue
        dev = all_vars(c, S, M)
        last_var = dev
        for s, h in enumerate(rhyps):
            _, var64 = R.refit(X, y, Xc, h, kernel, rows0[:j - 1])
            dgrid = float(np.max(np.abs(dev[s] - var64))) / h["amp"]
            line = "%s after pick %d sample %d: whole grid |dvar|/amp %.3e" % (label, j, s, dgrid)
            if truths is not None:
                tv = truths[s][j - 1][1]
                err_dev, err_ref = R.err_vs_truth(dev[s][probes], tv), R.err_vs_truth(var64[probes], tv)
                bar = E.gp_bar(err_ref, h["amp"])
                line += "  probes (%d rows): device %.3e amp, float64 refit %.3e amp off the truth, bar %.3e amp" % (
                    len(probes), err_dev / h["amp"], err_ref / h["amp"], bar / h["amp"])
                worst_dev, worst_ref = max(worst_dev, err_dev / h["amp"]), max(worst_ref, err_ref / h["amp"])
            print(line)
            assert dgrid <= 1e-5, line
            if truths is not None:
                assert err_dev <= bar, line
    # no state leaks: the plain nomination afterwards is pick 1 again, bit for bit
    v1b, i1b = c.eval_nominate(hyps, **sp)
    assert np.float64(v1b).tobytes() == np.float64(v1).tobytes() and i1b == i1
    if truths is not None:
        print("%s worst on the probes: device %.3e amp, float64 refit %.3e amp" % (label, worst_dev, worst_ref))
    return vq, iq, last_var, rep


# ---- 1. every instance of believer_kernel<DPAD, KERN> ---------------------------------------------------------------------------
#  d -> (DPAD class, seed under ARD-SE, seed under Matern-5/2); d <= 32: the small regime, d > 32: the general layout (Npad 128, 32-row slabs)
INSTANCES = {3: (4, 5, 11), 6: (8, 11, 3), 12: (16, 11, 11), 24: (32, 2, 6), 40: (48, 8, 2), 60: (64, 2, 11), 96: (96, 10, 10)}
KINDS = ("ei", "cb", "logei")


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("d", sorted(INSTANCES))
def test_every_instance_downdates_to_the_truth(dctx, d, kernel):
    seed = INSTANCES[d][1 if kernel == "ardse" else 2]
    kind = KINDS[(sorted(INSTANCES).index(d) + (kernel != "ardse")) % 3]
    X, y, Xc, hyps = problem(24, d, 200, 2, seed)
    stage(dctx, X, y, Xc, kernel)
    try:
        check_case(dctx, "instance d=%d %s %s" % (d, kernel, kind), X, y, Xc, hyps, kernel, kind, 3, after=(2, 3))
    finally:
        dctx.gp_set_kernel("ardse")


# ---- 2. q = B7_BATCH_MAX ------------------------------------------------------------------------------------------------------------
#          name      N    d  S  {kind: seed}
Q16 = {"small": (24, 3, 3, {"ei": 21, "logei": 19}), "general": (150, 5, 2, {"cb": 23})}


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(Q16) for k in sorted(Q16[n][3])])
def test_sixteen_picks(dctx, name, kind):
    """The most the entry point reaches: 15 believed rows (the sixteenth pick is never believed), so the last downdate runs
    p.j = 14 -- a cc loop of 14 terms, 1 + 14 = 15 scalars through ssc (t_j and fourteen u_i(x_j)) at scal's stride BSC = 17, of
    which entries 15 and 16 stay unused -- and fifteen u columns in bel.  The variance after picks 2, 9 and 16; every prefix call
    (q = 9 among them) returns the first picks of the q = 16 call bit for bit (check_case)."""
    N, d, S, seeds = Q16[name]
    X, y, Xc, hyps = problem(N, d, 333, S, seeds[kind])
    stage(dctx, X, y, Xc, "ardse")
    check_case(dctx, "q16 %s %s" % (name, kind), X, y, Xc, hyps, "ardse", kind, 16, after=(2, 9, 16))


# ---- 3. the routes that feed BelKeep ---------------------------------------------------------------------------------------------
ROUTES_SEED = 4


def _counted(c, hyps, q, sp):
    c.profile_enable(True)
    try:
        c.profile_reset()
        vq, iq = c.eval_nominate_batch(hyps, q, **sp)
        counts = {ph: c.profile_get(ph)[1] for ph in ("kxx", "ksx", "post", "kpost")}
    finally:
        c.profile_enable(False)
    return vq, iq, counts


def test_routes_b_c_d_give_the_same_bits(dctx, monkeypatch):
    """General layout (N = 150: Npad 256), S = 3, q = 4.  B: side-by-side fits, K* of all samples in the workspace.  C: the same
    fits, then the posterior one sample after the other because the workspace (128 KiB, the minimum) does not hold K*.  D: a
    context on the launch schedule (B7_POTRF_SCHED=1), which fits one sample after the other into the context's own slot;
    keep_sample copies every fit to its batch slot.  The phase counters say which ran: one "kxx" phase for the side-by-side
    assembly against S, one "post" phase for the batched posterior against at least S.  B is held to the references; C and D
    to B's bits."""
    S, q, M = 3, 4, 200
    X, y, Xc, hyps = problem(150, 5, M, S, ROUTES_SEED)
    sp = spec_of("ei", y)
    stage(dctx, X, y, Xc, "ardse")
    vb, ib, var_b, _ = check_case(dctx, "route B", X, y, Xc, hyps, "ardse", "ei", q, after=(2, 4))
    vb2, ib2, nb = _counted(dctx, hyps, q, sp)
    assert vb2.tobytes() == vb.tobytes() and np.array_equal(ib2, ib)
    assert nb["kxx"] == 1 and nb["post"] == 1 and nb["kpost"] == 0, nb
    assert np.array_equal(all_vars(dctx, S, M), var_b)
    # C
    dctx.set_workspace(128 << 10)
    try:
        vc, ic, nc = _counted(dctx, hyps, q, sp)
        var_c = all_vars(dctx, S, M)
    finally:
        dctx.set_workspace(4 << 30)
    assert nc["kxx"] == 1 and nc["post"] >= S and nc["ksx"] >= S and nc["kpost"] == 0, nc
    # D
    monkeypatch.setenv("B7_POTRF_SCHED", "1")
    cd = _diag_context()
    monkeypatch.delenv("B7_POTRF_SCHED")
    try:
        stage(cd, X, y, Xc, "ardse")
        vd, idd, nd = _counted(cd, hyps, q, sp)
        var_d = all_vars(cd, S, M)
    finally:
        cd.close()
    assert nd["kxx"] == S and nd["post"] == S and nd["kpost"] == 0, nd
    for name, v, i, var in (("C", vc, ic, var_c), ("D", vd, idd, var_d)):
        worst = float(np.max(np.abs(var - var_b)))
        print("route %s against route B: picks %s / %s, worst |dvar| %.3e" % (name, i.tolist(), ib.tolist(), worst))
        assert np.array_equal(i, ib) and v.tobytes() == vb.tobytes(), name
        assert var.tobytes() == var_b.tobytes(), (name, worst)


#                   N   d  S  seed     wide: the general layout (d > 32: Npad 128) with few enough observations for the truth
REDO = {"small": (40, 3, 3, 9), "general": (150, 5, 3, 2), "wide": (24, 33, 2, 10)}


@pytest.mark.parametrize("name", sorted(REDO))
def test_route_e_the_jitter_redo_downdates_with_the_jitter(dctx, name):
    """Duplicated observations with noise = 0 under the second of three samples (of two in "wide"): the nomination is redone
    through the jitter schedule, and the believer must take t_j = var + noise + jitter for that sample.  The references are built with
    noise + the reported jitter on the diagonal.  A jitter of 1e-8 moves the variances by far less than the whole-grid bar, so
    the cases that can tell are the ones held to the truth: the small regime, and "wide", where the redo's fits reach the
    believer through the general layout's copy to the batch slots."""
    N, d, S, seed = REDO[name]
    X, y, Xc, hyps = problem(N, d, 200, S, seed, dup=3)
    hyps[1] = dict(hyps[1], noise=0.0)
    stage(dctx, X, y, Xc, "ardse")
    _, _, _, rep = check_case(dctx, "route E %s" % name, X, y, Xc, hyps, "ardse", "cb", 4, after=(2, 4), jitter_from_report=True)
    print("route E %s: reported jitter %s info %s" % (name, rep["jitter"].tolist(), rep["info"].tolist()))
    assert rep["jitter"][1] > 0.0 and rep["info"][1] > 0
    assert not np.delete(rep["jitter"], 1).any() and not np.delete(rep["info"], 1).any()


# ---- 4. grid edges ------------------------------------------------------------------------------------------------------------------
#  regime -> (N, d); the general layout is reached with 24 observations by d > 32, which keeps the truth affordable
REGIMES = {"small": (24, 3), "general": (24, 40)}
#  (regime, M) -> (seed, score kind)
EDGES = {("small", 16): (6, "cb"), ("small", 5): (2, "logei"), ("small", 64): (2, "ei"), ("small", 65): (1, "ei"),
         ("small", 100): (2, "ei"), ("small", 256): (2, "ei"), ("small", 257): (2, "ei"),
         ("general", 16): (1, "cb"), ("general", 5): (8, "logei"), ("general", 64): (1, "ei"), ("general", 65): (9, "ei"),
         ("general", 100): (2, "ei"), ("general", 256): (8, "ei"), ("general", 257): (2, "ei")}
#  the cases whose seed puts a believed row (a pick before the last) into the last, partial block
BELIEVED_IN_TAIL = {("small", 100), ("general", 100)}


@pytest.mark.parametrize("regime,M", sorted(EDGES))
def test_grid_edges(dctx, regime, M):
    """M = q = 16: the last pick is the only row left and the picks are all rows.  M = 5, 64, 65, 256, 257 with q = min(4, M): one
    block and less, the block edges of believer_kernel and of the fused score kernel.  M = 100: a believed row in the last, partial
    block (rows 64..99)."""
    N, d = REGIMES[regime]
    q = 16 if M == 16 else min(4, M)
    seed, kind = EDGES[(regime, M)]
    X, y, Xc, hyps = problem(N, d, M, 2, seed)
    stage(dctx, X, y, Xc, "ardse")
    after = (2, 9, 16) if q == 16 else (2, q)
    _, iq, _, _ = check_case(dctx, "edge %s M=%d %s" % (regime, M, kind), X, y, Xc, hyps, "ardse", kind, q, after=after)
    if M == 16:
        assert sorted(iq.tolist()) == list(range(1, 17))
    if (regime, M) in BELIEVED_IN_TAIL:
        assert any(i - 1 >= 64 * (M // 64) for i in iq[:-1].tolist()), iq


# ---- 5. a sequence of calls on one context ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Q16))
def test_sequence_of_calls_equals_fresh_contexts(name):
    """q = 2, then q = 16, then grid_remove_rows of the sixteen picks, then q = 4 on the shrunk grid: bel and belvec regrow and the
    strides of u, var and scal's readers change.  Every call equals the same call on a fresh context bit for bit: values, picks
    and every sample's variance."""
    N, d, S, seeds = Q16[name]
    kind = sorted(seeds)[0]
    X, y, Xc, hyps = problem(N, d, 333, S, seeds[kind])
    sp = spec_of(kind, y)

    def fresh(grid, q):
        c = _diag_context()
        try:
            stage(c, X, y, grid, "ardse")
            v, i = c.eval_nominate_batch(hyps, q, **sp)
            return v, i, all_vars(c, S, len(grid))
        finally:
            c.close()

    c = _diag_context()
    try:
        stage(c, X, y, Xc, "ardse")
        got = []
        for q in (2, 16):
            v, i = c.eval_nominate_batch(hyps, q, **sp)
            got.append((v, i, all_vars(c, S, len(Xc))))
        gone = np.sort(got[1][1])
        rows = c.grid_remove_rows(gone)
        assert np.array_equal(rows, Xc[gone - 1])
        shrunk = np.delete(Xc, gone - 1, axis=0)
        assert np.array_equal(c.grid_download(), shrunk)
        v, i = c.eval_nominate_batch(hyps, 4, **sp)
        got.append((v, i, all_vars(c, S, len(shrunk))))
    finally:
        c.close()
    for (v, i, var), (grid, q) in zip(got, ((Xc, 2), (Xc, 16), (shrunk, 4))):
        fv, fi, fvar = fresh(grid, q)
        assert np.array_equal(i, fi) and v.tobytes() == fv.tobytes(), (q, i, fi)
        assert var.tobytes() == fvar.tobytes(), q
    assert got[0][0].tobytes() == got[1][0][:2].tobytes() and np.array_equal(got[0][1], got[1][1][:2])
