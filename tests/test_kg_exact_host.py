"""CPU-only checks of the exact line reference in tests/_kg_ref.py (lines_exact), which tests/test_gpu_kg_exact.py holds
b7_kg_nominate's slopes to: on every case of the GPU file a float64 restatement of the device algebra is inside the bars and
bar / scale <= 1e-9 (with the restatement's own W and with slopes_ref's long-double posterior behind it); each way kg_kernel can go
wrong puts a judged entry outside its bar; and the residual of W tells a diagonal without the jitter."""
import numpy as np
import pytest

import _kg_ref as R
import _post_ref as PR

CASES = R.EXACT_CASES + [R.ROUTES_CASE]


def _setup(N, d, kern, n, S, M, s, dup=0, jitter=0.0):
    X, y, Xc, hyps, arows, rows = R.exact_problem(N, d, M, S, n, dup)
    h = hyps[s]
    tnoise = h["noise"] + jitter
    kcol, W, var = R.host_operands(X, Xc[rows], Xc[arows], h, kern, tnoise)
    return X, y, Xc, hyps, arows, rows, h, tnoise, kcol, W, var


@pytest.mark.parametrize("N,d,kern,n,S,M", CASES, ids=["%d-%d-%s-n%d-S%d-M%d" % c for c in CASES])
def test_the_bars_can_be_met_and_stay_inside_the_cap(N, d, kern, n, S, M):
    """lines_host against lines_exact on the same W and variance, the last hyper sample of the case, every judged row; kcol
    against 50 digits entry by entry; the residual of W inside its bound; bar / scale <= 1e-9.  slopes_ref (long double, its own
    Cholesky) agrees with the exact lines to 1e-9 of the scale: the two references do not share their algebra."""
    s = S - 1
    X, y, Xc, hyps, arows, rows, h, tnoise, kcol, W, var = _setup(N, d, kern, n, S, M, s)
    ref = R.lines_exact(X, Xc[rows], Xc[arows], h, kern, W, var, tnoise)
    own = ~np.isin(rows, arows)
    rb, r0 = R.judge_lines(ref, R.lines_host(X, Xc[rows], Xc[arows], h, kern, W, var, tnoise), own)
    rk = R.kcol_ratio(X, Xc[arows], h, kern, kcol)
    res, bound = R.w_residual(X, h, kern, tnoise, kcol, W)
    print("N %d d %d %s n %d S %d M %d: host error / bar slopes %.3f own %.3f kcol %.3f, residual / bound %.3g, bar / scale %.2e, K* share "
          "%.2f, e_np %.3g" % (N, d, kern, n, S, M, rb.max(), r0[own].max(), rk.max(), np.max(res / bound), ref.cap, np.median(ref.share), ref.e_np))
    assert np.all(rb <= 1.0) and np.all(r0[own] <= 1.0) and np.all(rk <= 1.0) and np.all(res <= bound)
    assert ref.cap <= R.CAP
    _, _, slopes, _ = R.slopes_ref(X, y, Xc, [h], kern, rows0=arows)
    far = np.abs(slopes[0][rows][:, 1:] - ref.b[0]) / ref.scale
    assert far.max() <= 1e-9, far.max()


@pytest.mark.parametrize("N,d,kern,n,S,M", [R.ROUTES_CASE, R.EXACT_CASES[4], R.EXACT_CASES[12]])
def test_wrong_kernels_leave_the_bars(N, d, kern, n, S, M):
    """  slab    one 64-observation slab and one 32-observation slab (kg_slab for dpad >= 48) left out of K* W, each in turn
      swap    one W column exchanged with its neighbour, each pair
      hql     xs/2 taken from the neighbouring query
      ls0     the k(x, a_i) tile scaled with sample 0's lengthscales (S > 1: the last sample is judged)."""
    s = S - 1
    X, y, Xc, hyps, arows, rows, h, tnoise, kcol, W, var = _setup(N, d, kern, n, S, M, s)
    ref = R.lines_exact(X, Xc[rows], Xc[arows], h, kern, W, var, tnoise)
    own = ~np.isin(rows, arows)

    def ratios(wrong=None, **kw):
        return R.judge_lines(ref, R.lines_host(X, Xc[rows], Xc[arows], h, kern, W, var, tnoise, wrong, **kw), own)[0]

    assert np.all(ratios() <= 1.0)
    for width in (64, 32):
        for start in range(0, N, width):
            assert not np.all(ratios(("slab", start, width)) <= 1.0), ("slab", start, width)
    for i in range(n - 1):
        assert not np.all(ratios(("swap", i)) <= 1.0), ("swap", i)
    nxt = np.where(rows + 1 < M, rows + 1, rows - 1)
    assert np.all(ratios(("hql",), Xs_next=Xc[nxt]).max(axis=1) > 1.0)
    if S > 1:
        assert np.all(ratios(("ls0",), ls0=hyps[0]["lenscale_sq"]).max(axis=1) > 1.0)


@pytest.mark.parametrize("name", sorted(R.REDO))
def test_the_jitter_is_told(name):
    """The jitter cases, sample 1 (noise 0, duplicated observations) with the schedule's first step 1.1e-8 on the diagonal: the
    restatement meets the bars; t(x) = var + noise without the jitter leaves the bar on every row that has an own line; and the
    residual of W with the jitter left out of the diagonal exceeds 10 x its bound in every column."""
    N, d, S = R.REDO[name]
    jit = 1.1e-8
    X, y, Xc, hyps, arows, rows, h, tnoise, kcol, W, var = _setup(N, d, "ardse", 5, S, 200, 1, dup=3, jitter=jit)
    assert h["noise"] == 0.0
    ref = R.lines_exact(X, Xc[rows], Xc[arows], h, "ardse", W, var, tnoise)
    own = ~np.isin(rows, arows)
    rb, r0 = R.judge_lines(ref, R.lines_host(X, Xc[rows], Xc[arows], h, "ardse", W, var, tnoise), own)
    assert np.all(rb <= 1.0) and np.all(r0[own] <= 1.0) and ref.cap <= R.CAP
    rb, r0 = R.judge_lines(ref, R.lines_host(X, Xc[rows], Xc[arows], h, "ardse", W, var, tnoise, ("nojit", h["noise"])), own)
    assert np.all(r0[own] > 1.0) and np.all(rb.max(axis=1)[own] > 1.0)
    res, bound = R.w_residual(X, h, "ardse", tnoise, kcol, W)
    res0, _ = R.w_residual(X, h, "ardse", h["noise"], kcol, W)
    print("redo %s: residual / bound %.3g; without the jitter %.3g" % (name, np.max(res / bound), np.min(res0 / bound)))
    assert np.all(res <= bound) and np.all(res0 > 10.0 * bound)
