"""CPU-only checks of the exact path reference in tests/_ts_ref.py (paths_exact), which tests/test_gpu_ts_exact.py holds
b7_ts_nominate's paths to: on every case of the GPU file a float64 restatement of the device algebra is inside the bars and
bar / scale <= 1e-9; and each way the nomination's kernels can go wrong puts a judged entry outside its bar (or breaks the
identity's bound)."""
import numpy as np
import pytest

import _post_ref as PR
import _ts_ref as R

CASES = R.exact_cases()


def _setup(N, d, kern, S, q, F, M, jitter=None):
    X, Y, hyps, G, rows = R.case_problem(N, d, S, M)
    dr = [R.draws(R.SEED, j, F, d, N, hyps[j % S]["lenscale_sq"], hyps[j % S]["noise"], kern) for j in range(q)]
    al = R.host_alphas(X, Y, hyps, kern, dr, jitter)
    covs = [R.case_cov(N, d, kern, M, s) for s in range(min(S, q))]
    return X, Y, hyps, G, rows, dr, al, R.paths_exact(X, G[rows], hyps, kern, dr, al, covs)


@pytest.mark.parametrize("N,d,kern,S,q,F,M", CASES, ids=["%d-%d-%s-S%d-q%d-F%d-M%d" % c for c in CASES])
def test_the_bars_can_be_met_and_stay_inside_the_cap(N, d, kern, S, q, F, M):
    """paths_host with LAPACK's alpha against paths_exact with the same alpha, every judged entry; bar / scale <= 1e-9 on every
    one (paths_ref(..., want_v=True)'s v, the alpha of the true K, gives the same cap: it enters the scale as it enters the bar)."""
    X, Y, hyps, G, rows, dr, al, ref = _setup(N, d, kern, S, q, F, M)
    ratio = R.judge_paths(ref, R.paths_host(X, G[rows], hyps, kern, dr, al))
    cap = float(np.max(ref.bar / ref.scale))
    print("N %d d %d %s S %d q %d F %d M %d: host error / bar %.3f, bar / scale %.2e, K* share %.2f, e_np %.3g, e_rff %.3g" % (
        N, d, kern, S, q, F, M, ratio.max(), cap, np.median(ref.ks_share), ref.e_np.max(), ref.e_rff.max()))
    assert np.all(ratio <= 1.0), ratio.max()
    assert cap <= R.CAP
    _, vs = R.paths_ref(X, Y, G[rows], hyps, kern, dr, want_v=True)
    alv = [np.stack([vs[j] for j in range(s, q, S)], axis=1) for s in range(min(S, q))]
    ref_v = R.paths_exact(X, G[rows], hyps, kern, dr, alv, [R.case_cov(N, d, kern, M, s) for s in range(min(S, q))])
    assert float(np.max(ref_v.bar / ref_v.scale)) <= R.CAP


WRONG = [(65, 33, PR.SE, 3, 16, 256, 1037), (129, 65, PR.MATERN, 3, 5, 256, 1037), (300, 6, PR.SE, 3, 16, 16, 1037)]


@pytest.mark.parametrize("N,d,kern,S,q,F,M", WRONG)
def test_wrong_kernels_leave_the_bars(N, d, kern, S, q, F, M):
    """  slab     one 64-observation slab (and one 32-observation half, the slab of dpad >= 48) left out of K* alpha, each in turn
      swap     one alpha column exchanged with its neighbour, every pair of every sample with qs > 1
      layout   path column s + S p written to p + qs s
      chunk    one chunk of 16 features dropped, each in turn
      base     the base add skipped on the last ragged 16-row tile
      hql      xs/2 taken from the neighbouring query."""
    X, Y, hyps, G, rows, dr, al, ref = _setup(N, d, kern, S, q, F, M)
    Xs = G[rows]

    def out(wrong=None, **kw):
        return not np.all(R.judge_paths(ref, R.paths_host(X, Xs, hyps, kern, dr, al, wrong, **kw)) <= 1.0)

    assert not out()
    for width in (64, 32):
        for start in range(0, N, width):
            assert out(("slab", start, width)), ("slab", start, width)
    for s in range(S):
        for p in range(al[s].shape[1] - 1):
            assert out(("swap", s, p)), ("swap", s, p)
    assert out(("layout",))
    for c in range(F // 16):
        assert out(("chunk", c)), ("chunk", c)
    tail = rows >= 16 * ((M - 1) // 16)
    assert tail.any() and M % 16
    bad = R.judge_paths(ref, R.paths_host(X, Xs, hyps, kern, dr, al, ("base",), tail=tail))
    assert np.all(bad[tail] > 1.0) and np.all(bad[~tail] <= 1.0)
    nxt = np.where(rows + 1 < M, rows + 1, rows - 1)
    bad = R.judge_paths(ref, R.paths_host(X, Xs, hyps, kern, dr, al, ("hql",), Xs_next=G[nxt]))
    assert np.all(bad.max(axis=1) > 1.0)


def test_the_identity_tells_the_jitter():
    """Duplicated observations, noise 0: with the jitter on the diagonal the float64 restatement meets the identity's bound; with
    the jitter left out of the identity (alpha unchanged) the residual exceeds 10 x the bound."""
    N, d, S, q, F = 40, 3, 2, 4, 256
    X, Y, hyp = PR.case_inputs(N, d)
    X[N - 5:], Y[N - 5:] = X[:5], Y[:5]
    hyps = [dict(h, noise=0.0) for h in PR.hyper_samples(hyp, S)]
    jit = np.full(S, 1.1e-8)
    dr = [R.draws(R.SEED, j, F, d, N, hyps[j % S]["lenscale_sq"], 0.0, PR.SE) for j in range(q)]
    al = R.host_alphas(X, Y, hyps, PR.SE, dr, jit)
    P = R.paths_host(X, X, hyps, PR.SE, dr, al)
    norms = [float(np.abs(R.cov(X, X, h["lenscale_sq"], h["amp"])).sum(1).max()) for h in hyps]
    res, bound = R.identity_residual(P, dr, al, Y, hyps, jit, norms)
    res0, _ = R.identity_residual(P, dr, al, Y, hyps, np.zeros(S), norms)
    print("identity: residual %.3g (bound %.3g); without the jitter %.3g" % (res.max(), bound.max(), res0.max()))
    assert np.all(res <= bound) and np.all(res0 > 10.0 * bound)
