"""b7_ts_nominate's sample paths held to EXACT arithmetic, given the device's own alpha columns (diagnostic build:
b7dbg_ts_alpha) and its own draws; the alpha columns themselves held by the identity's residual, with the reported jitter; and the
arg-min rule held bit for bit on the device's own paths, NaN rows, exact ties and a second lap of the grid-stride loop included.
Needs an MI355X: run with -m gpu.

Reference and bars: tests/_ts_ref.py (paths_exact), checked on the CPU by tests/test_ts_exact_host.py.  Per judged row x and path
j: [m + sum_i k(x, x_i) alpha_ij] from 50-digit covariances of exact arguments, error-free products and exact sums, plus the prior
term at 50 digits with W' = fl(sqrt(2 amp / F) weight); bar = gp_bar(numpy's own float64 error on the same operands) + sum |alpha_i|
dk_i + test_gpu_ts.rff_check's bar + 2 u |value|, and below 1e-9 of the scale on every row.  Every judged row of every path is
judged.  Each test prints its figures; DESIGN.md section 8 carries the MI355X table."""
import ctypes as C

import numpy as np
import pytest

import _post_ref as PR
import _ts_ref as R

pytestmark = pytest.mark.gpu
CASES = R.exact_cases()


@pytest.fixture(scope="module")
def dctx():
    """The diagnostic build: b7dbg_ts_alpha (every hyper sample's alpha columns of the last nomination) exists there only."""
    import bot7_amd
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_ts_alpha.restype = C.c_int
    c._L.b7dbg_ts_alpha.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    yield c
    c.close()


def ts_alphas(c, N, S, q):
    """alphas[s]: N x qs, the alpha columns of hyper sample s's pseudo-response fit in the last ts_nominate."""
    out = []
    for s in range(min(S, q)):
        qs = len(range(s, q, S))
        a, got = np.empty((N, qs), dtype=np.float64), C.c_int(0)
        assert c._L.b7dbg_ts_alpha(c._h, s, a.ctypes.data, C.byref(got)) == 0 and got.value == qs
        out.append(a)
    return out


def stage(c, X, Y, G, kern):
    c.gp_set_kernel(kern)
    c.grid_upload(G)
    c.gp_set_data(X, Y)


def nominate(c, hyps, q, F, N):
    vals, idx, rep = c.ts_nominate(hyps, q, n_features=F, seed=R.SEED, want_report=True)
    P = c.ts_last_paths()
    return vals, idx, rep, P, [c.ts_last_draws(j) for j in range(q)], ts_alphas(c, N, len(hyps), q)


def check_rule(P, vals, idx):
    """The nominees are the rule's on the device's own paths, bit for bit; path_min is the path's own value."""
    assert (idx - 1).tolist() == R.nominees_ref(P)
    assert all(np.float64(vals[j]).tobytes() == P[idx[j] - 1, j].tobytes() for j in range(len(idx)))


def hold(tag, ref, P):
    ratio = R.judge_paths(ref, P)
    err = R.E.abs_errors(P, ref.hi, ref.lo)
    cap = float(np.max(ref.bar / ref.scale))
    print("%s: %d rows x %d paths: worst error / bar %.3f (error %.1f u scale); K* share of the bar %.2f; e_np %.1f u scale, e_rff %.1f u "
          "scale; bar / scale <= %.1e" % (tag, P.shape[0], P.shape[1], ratio.max(), np.max(err / ref.scale) / R.U, np.median(ref.ks_share),
                                         np.max(ref.e_np[None, :] / ref.scale) / R.U, np.max(ref.e_rff[None, :] / ref.scale) / R.U, cap))
    assert np.isfinite(P).all() and cap <= R.CAP, tag
    bad = np.argwhere(~(ratio <= 1.0))
    assert bad.size == 0, "%s: entries outside the bar (position among the judged rows, path): %s, worst %.3g" % (tag, bad.tolist(), np.nanmax(ratio))


@pytest.mark.parametrize("N,d,kern,S,q,F,M", CASES, ids=["%d-%d-%s-S%d-q%d-F%d-M%d" % c for c in CASES])
def test_paths_against_exact_arithmetic(dctx, N, d, kern, S, q, F, M):
    """Every (N, d) of rff dpad 8 / 16 / 64 / 96 and Npad 64 / 128 / 256 / 384, both covariance kernels, (S, q) with qs == 1 alone, qs
    > 1 alone and both within one call ((3, 5): qs = 2, 2, 1; q = 16 becomes 7 on the 7-row grid), F in {16, 256}, M in {7, 1037}
    (tests/_ts_ref.exact_cases).  No jitter.  The nominees by the rule on the device's own paths, bit for bit."""
    X, Y, hyps, G, rows = R.case_problem(N, d, S, M)
    try:
        stage(dctx, X, Y, G, kern)
        vals, idx, rep, P, dr, al = nominate(dctx, hyps, q, F, N)
        assert not rep["jitter"].any() and not rep["info"].any(), rep
        ref = R.paths_exact(X, G[rows], hyps, kern, dr, al, [R.case_cov(N, d, kern, M, s) for s in range(min(S, q))])
        hold("N %d d %d %s S %d q %d F %d M %d" % (N, d, kern, S, q, F, M), ref, P[rows])
        check_rule(P, vals, idx)
    finally:
        dctx.gp_set_kernel(PR.SE)


@pytest.mark.parametrize("N,d", R.EXACT_ND)
def test_alpha_by_the_identity(dctx, N, d):
    """The operands themselves: with the grid the observations, paths(X_obs) + eps + noise alpha = y within the backward error of
    two stable solves, 64 N 2^-53 ||K||_inf max |alpha|, for every path of an S = 3, q = 5 call (qs = 2, 2, 1), with the device's
    own paths, eps and alpha."""
    X, Y, hyps, _, _ = R.case_problem(N, d, 3, 7)
    kern = R.KERNELS[N % 2]
    try:
        stage(dctx, X, Y, X, kern)
        _, _, rep, P, dr, al = nominate(dctx, hyps, 5, 256, N)
        assert not rep["jitter"].any()
        norms = [float(np.abs(R.cov(X, X, h["lenscale_sq"], h["amp"], kern)).sum(1).max()) + h["noise"] for h in hyps]
        res, bound = R.identity_residual(P, dr, al, Y, hyps, rep["jitter"], norms)
        print("identity N %d d %d %s: worst residual / bound %.3g (residual %.3g, max |alpha| %.3g)" % (
            N, d, kern, np.max(res / bound), res.max(), max(np.abs(a).max() for a in al)))
        assert np.all(res <= bound)
    finally:
        dctx.gp_set_kernel(PR.SE)


def test_chunked_mean_gives_the_same_bits(dctx):
    """N = 300 (Npad 384), M = 1037, S = 3, q = 5 with the workspace at its minimum, 128 KiB: ts_mean_over_grid runs five chunks of
    256 rows, the last one ragged, through launch_mean_multi (qs = 2) and the fused mean (qs = 1).  The paths, minima and nominees
    equal the one-chunk call's bit for bit (which test_paths_against_exact_arithmetic holds to the bars)."""
    N, d, S, q, F, M = 300, 6, 3, 5, 256, 1037
    X, Y, hyps, G, _ = R.case_problem(N, d, S, M)
    stage(dctx, X, Y, G, PR.SE)
    v1, i1, _, P1, _, a1 = nominate(dctx, hyps, q, F, N)
    assert PR.chunk_rows(128 << 10, PR.npad_of(N), M) == 256
    dctx.set_workspace(128 << 10)
    try:
        v2, i2, _, P2, _, a2 = nominate(dctx, hyps, q, F, N)
    finally:
        dctx.set_workspace(PR.WORKSPACE_DEFAULT)
    assert P2.tobytes() == P1.tobytes() and v2.tobytes() == v1.tobytes() and np.array_equal(i1, i2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a1, a2))


def test_jitter_case_paths_and_identity(dctx):
    """Duplicated observation rows, noise 0, N = 40: the jitter schedule takes over.  The grid is the observations followed by
    60 seeded rows.  The paths against exact arithmetic (given alpha, their value does not involve the jitter); the identity with
    noise + the REPORTED jitter on alpha's diagonal -- without it the residual would be jitter max |alpha|, far beyond the bound
    (tests/test_ts_exact_host.py)."""
    N, d, S, q, F = 40, 3, 2, 4, 256
    X, Y, hyp = PR.case_inputs(N, d)
    X[N - 5:], Y[N - 5:] = X[:5], Y[:5]
    hyps = [dict(h, noise=0.0) for h in PR.hyper_samples(hyp, S)]
    G = np.concatenate([X, np.random.default_rng(40).random((60, d))])
    stage(dctx, X, Y, G, PR.SE)
    vals, idx, rep, P, dr, al = nominate(dctx, hyps, q, F, N)
    assert (rep["jitter"] > 0).all() and (rep["info"] != 0).all(), rep
    rows = np.arange(len(G))
    ref = R.paths_exact(X, G, hyps, PR.SE, dr, al)
    hold("jitter %s" % rep["jitter"].tolist(), ref, P[rows])
    check_rule(P, vals, idx)
    norms = [float(np.abs(R.cov(X, X, h["lenscale_sq"], h["amp"])).sum(1).max()) + float(j) for h, j in zip(hyps, rep["jitter"])]
    res, bound = R.identity_residual(P[:N], dr, al, Y, hyps, rep["jitter"], norms)
    res0, _ = R.identity_residual(P[:N], dr, al, Y, hyps, np.zeros(S), norms)
    print("jitter identity: worst residual / bound %.3g (residual %.3g, max |alpha| %.3g); without the jitter the residual is %.3g" % (
        np.max(res / bound), res.max(), max(np.abs(a).max() for a in al), res0.max()))
    assert np.all(res <= bound) and np.all(res0 > 10.0 * bound)


@pytest.mark.parametrize("M,q", [(7, 7), (1037, 16), (262144 + 300, 16)])
def test_the_rule_on_nan_rows_ties_and_a_second_lap(dctx, M, q):
    """N = 5, d = 3, F = 16.  Some grid rows carry a NaN coordinate: their paths are NaN and never win.  After a first call the row
    of path 0's minimum is copied to a lower and to a higher index (at the largest M, beyond row 262 144, where nblk = 1024 blocks
    of 256 make the grid-stride loop take a second lap, with a NaN row there too): the first of the equal values wins.  (idx - 1)
    == nominees_ref(P) on the device's own paths; q = M = 7 must come out as a permutation with the NaN rows last."""
    N, d, F = 5, 3, 16
    X, Y, hyp = PR.case_inputs(N, d)
    G = np.random.default_rng(M).random((M, d))
    nan_rows = [2, M - 2] if M > 7 else [2]
    if M > 262144:
        nan_rows += [262144 + 100]
    for r in nan_rows:
        G[r, r % d] = np.nan
    stage(dctx, X, Y, G, PR.SE)
    _, idx0, _, P0, _, _ = nominate(dctx, [hyp], q, F, N)
    r0 = int(idx0[0]) - 1
    assert r0 not in nan_rows and np.isnan(P0[nan_rows]).all() and np.isfinite(np.delete(P0, nan_rows, axis=0)).all()
    lowc, highc = (0 if r0 != 0 else 1), (M - 1 if M <= 262144 else 262144 + 5)
    if M == 7:
        highc = 6 if r0 != 6 else 5
    G[lowc], G[highc] = G[r0], G[r0]
    dctx.grid_upload(G)
    vals, idx, _, P, _, _ = nominate(dctx, [hyp], q, F, N)
    assert P[lowc].tobytes() == P[r0].tobytes() == P[highc].tobytes()
    check_rule(P, vals, idx)
    assert idx[0] - 1 == min(lowc, r0) and len(set(idx.tolist())) == q
    if M == 7:
        assert sorted(idx.tolist()) == list(range(1, 8)) and idx[-1] - 1 == 2
