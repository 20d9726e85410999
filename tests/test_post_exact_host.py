"""CPU-only checks of tests/_post_ref.py, the reference and the bars of tests/test_gpu_post_exact.py: the exact evaluation against
plain 50-digit arithmetic; every case's bars met by a float64 restatement of the device algebra, and inside the 1e-9 cap; and
seven kinds of wrong kernel, each of which must push at least one judged row out of its bar."""
import functools

import numpy as np
import pytest

import _exact as E
import _post_ref as R

CASES = R.all_cases()


@functools.lru_cache(maxsize=None)
def _case(i):
    """Case i of the GPU file on the host: the fit by LAPACK, the grid, the judged rows, the reference of those rows under the
    host's own L^-1 and alpha, and K* of those rows as the device forms it."""
    name, N, d, kern, hyp, Ms = CASES[i]
    X, Y, _ = R.case_inputs(N, d)
    _, Linv, alpha, cond = R.host_fit(X, Y, hyp, kern)
    M, per, rows = R.case_rows(Ms)
    G = R.make_grid(M, X)
    ref = R.reference(X, hyp, kern, Linv, alpha, G, rows)
    Ks = R.device_kstar(G[rows], X, hyp["lenscale_sq"], hyp["amp"], kern)
    return X, hyp, kern, Linv, alpha, G, rows, ref, Ks, cond, per


def _index(N, d):
    return next(i for i, c in enumerate(CASES) if c[0] == "a" and c[1:3] == (N, d))


@pytest.mark.parametrize("kern", [R.SE, R.MATERN])
@pytest.mark.parametrize("N", [5, 40])
def test_the_double_double_reference_agrees_with_50_digit_arithmetic(N, kern):
    """exact_post_rows against mp_post_rows (the same formula, the same operands, 50 digits) within 2^-90 of the scale, on seeded
    rows and on candidates equal to an observation (k_i = amp there: the variance is a difference of nearly equal numbers)."""
    d = 3
    X, Y, hyp = R.case_inputs(N, d)
    _, Linv, alpha, _ = R.host_fit(X, Y, hyp, kern)
    Xs = np.concatenate([np.random.default_rng(N).random((6, d)), X[[0, N - 1]]])
    cov = R.true_cov_rows(Xs, X, hyp["lenscale_sq"], hyp["amp"], kern)
    assert cov.hi[6, 0] == hyp["amp"] and cov.hi[7, N - 1] == hyp["amp"] and cov.lo[6, 0] == 0.0
    for add in (0.0, hyp["noise"]):
        post = R.exact_post_rows(Linv, alpha, cov.hi, cov.lo, hyp["amp"], add, hyp["mean"])
        mu, var = R.mp_post_rows(Linv, alpha, cov.hi, cov.lo, hyp["amp"], add, hyp["mean"])
        with E.mpmath.workdps(50):
            for r in range(len(Xs)):
                em = abs(E.mpmath.mpf(post.mu[0][r]) + E.mpmath.mpf(post.mu[1][r]) - mu[r])
                ev = abs(E.mpmath.mpf(post.var[0][r]) + E.mpmath.mpf(post.var[1][r]) - var[r])
                assert em <= R.REF_GOOD * post.scale_m[r] and ev <= R.REF_GOOD * post.scale_v[r], (N, kern, r, em, ev)


def test_the_true_covariance_is_the_oracles_to_rounding():
    """true_cov_rows against the float64 covariance of the direct form (differences first), both kernels: within 8 d ulp."""
    X, _, hyp = R.case_inputs(40, 6)
    Xs = np.random.default_rng(1).random((5, 6))
    D = (((Xs[:, None, :] - X[None, :, :]) ** 2) / hyp["lenscale_sq"]).sum(-1)
    s = np.sqrt(5.0 * D)
    for kern, want in ((R.SE, hyp["amp"] * np.exp(-0.5 * D)), (R.MATERN, hyp["amp"] * (1 + s + s * s / 3) * np.exp(-s))):
        cov = R.true_cov_rows(Xs, X, hyp["lenscale_sq"], hyp["amp"], kern)
        assert np.all(np.abs(want - cov.hi) <= 8 * 6 * E.EPS * cov.hi), kern


@pytest.mark.parametrize("i", range(len(CASES)), ids=["%s-%d-%d-%s" % c[:4] for c in CASES])
def test_the_bars_can_be_met_and_are_not_vacuous(i):
    """On every case of the GPU file: LAPACK factors the fit without jitter (host_fit asserts it), the float64 restatement of the
    device algebra (K* by the expansion formula with np.exp) is inside the bars on every judged row, and bar / scale <= 1e-9."""
    X, hyp, kern, Linv, alpha, G, rows, ref, Ks, cond, _ = _case(i)
    mu, var = R.numpy_post(Ks, Linv, alpha, hyp["amp"], 0.0, hyp["mean"])
    rm, rv = R.judge(ref, rows, mu, var)
    cap_m, cap_v = float(np.max(ref.bar_m / ref.post.scale_m)), float(np.max(ref.bar_v / ref.post.scale_v))
    print("%s N %d d %d %s: cond %.1e, host error / bar mean %.3f var %.3f, bar / scale mean %.2e var %.2e, K* share mean %.2f var "
          "%.2f, e_np mean %.1f u scale, var %.1f u scale" % (CASES[i][:4] + (
              cond, rm.max(), rv.max(), cap_m, cap_v, np.median(ref.share_m), np.median(ref.share_v),
              ref.e_np_m / (R.U * ref.post.scale_m.max()), ref.e_np_v / (R.U * ref.post.scale_v.max()))))
    assert R.within(rm) and R.within(rv), (rm.max(), rv.max())
    assert cap_m <= R.CAP and cap_v <= R.CAP, (cap_m, cap_v)


def _caught(case, Ks=None, Linv=None, what="any"):
    """The corrupted evaluation leaves the bar on the judged rows of EACH grid size the GPU test runs (it judges each output on its
    own rows; the reference here covers their union)."""
    X, hyp, kern, Linv0, alpha, G, rows, ref, Ks0, _, per = case
    mu, var = R.numpy_post(Ks0 if Ks is None else Ks, Linv0 if Linv is None else Linv, alpha, hyp["amp"], 0.0, hyp["mean"])
    out = []
    for sub in per:
        pos = ref.pick(sub)
        rm, rv = R.judge(ref, sub, mu[pos], var[pos])
        out.append({"mean": not R.within(rm), "var": not R.within(rv), "any": not (R.within(rm) and R.within(rv))}[what])
    return any(out) if Ks is None and Linv is None else all(out)


def _caught_row(case, Ks, r, what="any"):
    """A corruption of judged row r alone: that row leaves its bar."""
    X, hyp, kern, Linv, alpha, G, rows, ref, _, _, _ = case
    mu, var = R.numpy_post(Ks[r:r + 1], Linv, alpha, hyp["amp"], 0.0, hyp["mean"])
    rm, rv = R.judge(ref, rows[r:r + 1], mu, var)
    return {"mean": not R.within(rm), "var": not R.within(rv), "any": not (R.within(rm) and R.within(rv))}[what]


@pytest.mark.parametrize("N,d", [(700, 6), (400, 33), (300, 65)])
def test_wrong_kernels_leave_the_bars(N, d):
    """The host evaluation corrupted the ways a posterior kernel goes wrong, on a three-tile case and the two cases of the 32-row
    slab classes: each corruption must put at least one judged row outside its bar (the mean's AND the variance's, where both
    read what is corrupted).
      block      one 64-observation block left out of the sum over i -- each block in turn, the ragged last one included
      slab       one 32-observation slab left out (dpad >= 48: the walk's slab there) -- each in turn
      linv       one off-diagonal 64 x 64 block of L^-1 zeroed -- each in turn (variance only)
      swap       two K* columns swapped across a 64 boundary -- each boundary in turn
      tail       an off-by-one at the ragged end: the last observation's column read at N - 2 as well, the column that belongs
                 there dropped
      entry      one K* entry times (1 + 1e-8) -- on each judged row in turn, the row's largest entry
      neighbour  one judged row evaluated with the next grid row's x* -- each judged row in turn"""
    case = _case(_index(N, d))
    X, hyp, kern, Linv, alpha, G, rows, ref, Ks, _, per = case
    assert not _caught(case)
    nb = -(-N // 64)
    for b in range(nb):
        K2 = Ks.copy()
        K2[:, 64 * b:64 * b + 64] = 0.0
        assert _caught(case, Ks=K2, what="mean") and _caught(case, Ks=K2, what="var"), ("block", b)
    if R.dpad_of(d) >= 48:
        for s in range(-(-N // 32)):
            K2 = Ks.copy()
            K2[:, 32 * s:32 * s + 32] = 0.0
            assert _caught(case, Ks=K2, what="mean") and _caught(case, Ks=K2, what="var"), ("slab", s)
    for I in range(nb):
        for J in range(I):
            L2 = Linv.copy()
            L2[64 * I:64 * I + 64, 64 * J:64 * J + 64] = 0.0
            assert _caught(case, Linv=L2, what="var"), ("linv", I, J)
    for b in range(1, nb):
        K2 = Ks.copy()
        K2[:, [64 * b - 1, 64 * b]] = K2[:, [64 * b, 64 * b - 1]]
        assert _caught(case, Ks=K2, what="mean") and _caught(case, Ks=K2, what="var"), ("swap", b)
    K2 = Ks.copy()
    K2[:, N - 2] = K2[:, N - 1]
    assert _caught(case, Ks=K2, what="mean") and _caught(case, Ks=K2, what="var"), "tail"
    for r in range(len(rows)):
        K2 = Ks.copy()
        K2[r, np.argmax(Ks[r])] *= 1.0 + 1e-8
        assert _caught_row(case, K2, r), ("entry", int(rows[r]))
        K2 = Ks.copy()
        nbr = rows[r] + 1 if rows[r] + 1 < len(G) else rows[r] - 1
        K2[r] = R.device_kstar(G[nbr:nbr + 1], X, hyp["lenscale_sq"], hyp["amp"], kern)[0]
        assert _caught_row(case, K2, r, "mean") and _caught_row(case, K2, r, "var"), ("neighbour", int(rows[r]))
