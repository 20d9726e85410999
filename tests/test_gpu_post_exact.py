"""The posterior kernels -- K(X*,X) (ksx_kernel), the variance kernels (post_kernel_w4<2>, post_kernel_w4<4>, post_kernel_w4t,
post_small_kernel), the means, and the fused kpost_small_kernel -- held to EXACT arithmetic at every N and route, given the
device's own L^-1 and alpha (gp_download; their quality is held by test_gpu_numerics.py and test_gpu_pending.py).  Needs an
MI355X: run with -m gpu.

Reference and bars: tests/_post_ref.py (checked on the CPU by tests/test_post_exact_host.py, which also shows that the judged rows
and the bars catch a dropped observation block or slab, a wrong block of L^-1, swapped or shifted K* columns, one K* entry off by
1e-8 and a row evaluated at its neighbour).  Per judged row x*: the true covariance entries from 50-digit arithmetic on an exact
argument, var = amp (+ noise) - |Linv k|^2 and mu = mean + k . alpha evaluated exactly; bar = 8 x numpy's own float64 error on the
same operands + 16 eps scale (E.gp_bar) + the first-order K* term (the suite's per-entry covariance bars and the counted rounding
of the device's argument), absolute, and below 1e-9 of the scale on every row.  Every judged row is judged; every fit has
jitter == 0.  Each test prints the worst error / bar, the K* share of the bar and the yardstick e_np."""
import os

import numpy as np
import pytest

import _exact as E
import _post_ref as R

pytestmark = pytest.mark.gpu
GENERAL = {"B7_FIT_SMALL": "0", "B7_KPOST_SMALL": "0", "B7_NLL_SMALL": "0"}


@pytest.fixture(scope="module")
def gen():
    """A context of the diagnostic build with every small-problem kernel switched off (switches are read at b7_create)."""
    import bot7_amd
    old = {k: os.environ.get(k) for k in GENERAL}
    os.environ.update(GENERAL)
    try:
        c = bot7_amd.Context(0, lib="diag")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(ctx):
    return ctx.device_info()["compute_units"]


def _fit(c, X, Y, hyp, kern):
    """gp_fit under kern without jitter; the device's own (Linv, alpha)."""
    c.gp_set_kernel(kern)
    rep = c.gp_fit(X, Y, hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
    assert rep["jitter"] == 0, rep
    _, alpha, Linv = c.gp_download(len(X))
    return Linv, alpha[:, 0]


def _hold(tag, ref, rows, mu, var):
    """Every judged row of one output inside its bars; prints the case's figures."""
    mu, var = np.asarray(mu, dtype=np.float64).reshape(len(var), -1)[:, 0], np.asarray(var, dtype=np.float64)
    assert np.isfinite(mu).all() and np.isfinite(var).all(), tag
    rm, rv = R.judge(ref, rows, mu[rows], var[rows])
    pos = ref.pick(rows)
    print("%s: %d rows of %d: worst error / bar mean %.3f var %.3f (error %.1f, %.1f u scale); K* share of the bar mean %.2f var "
          "%.2f; e_np mean %.3g (%.1f u scale) var %.3g (%.1f u scale); bar / scale <= %.1e" % (
              tag, len(rows), len(var), rm.max(), rv.max(), np.max(rm * ref.bar_m[pos] / ref.post.scale_m[pos]) / R.U,
              np.max(rv * ref.bar_v[pos] / ref.post.scale_v[pos]) / R.U, np.median(ref.share_m[pos]),
              np.median(ref.share_v[pos]), ref.e_np_m, ref.e_np_m / (R.U * ref.post.scale_m.max()), ref.e_np_v,
              ref.e_np_v / (R.U * ref.post.scale_v.max()),
              max(np.max(ref.bar_m / ref.post.scale_m), np.max(ref.bar_v / ref.post.scale_v))))
    assert np.max(ref.bar_m / ref.post.scale_m) <= R.CAP and np.max(ref.bar_v / ref.post.scale_v) <= R.CAP, tag
    bad_m, bad_v = rows[~(rm <= 1.0)], rows[~(rv <= 1.0)]
    assert bad_m.size == 0 and bad_v.size == 0, "%s: rows outside the bar: mean %s (worst %.3g), variance %s (worst %.3g)" % (
        tag, bad_m.tolist(), np.nanmax(rm), bad_v.tolist(), np.nanmax(rv))


def _single_fit_case(c, N, d, kern, Ms, tag):
    """One fit, then gp_predict over the head of one grid at every size of Ms; the reference is computed once over the union of
    the judged rows."""
    X, Y, hyp = R.case_inputs(N, d)
    chunks = [R.chunk_rows(R.WORKSPACE_DEFAULT, R.npad_of(N), M) for M in Ms]
    M, rows, allrows = R.case_rows(Ms, chunks)
    G = R.make_grid(M, X)
    try:
        Linv, alpha = _fit(c, X, Y, hyp, kern)
        ref = R.reference(X, hyp, kern, Linv, alpha, G, allrows)
        for Mi, ri in zip(Ms, rows):
            c.grid_upload(G[:Mi])
            mu, var = c.gp_predict()
            _hold("%s N %d d %d %s M %d" % (tag, N, d, kern, Mi), ref, ri, mu, var)
    finally:
        c.gp_set_kernel(R.SE)


@pytest.mark.parametrize("N,d,kern", R.CASES_A)
def test_a_general_route_against_exact_arithmetic(ctx, cus, N, d, kern):
    """gp_fit + gp_predict on the default library, S = 1, each case over a grid below one 256-candidate workgroup per CU (1037
    rows: post_kernel_w4<2>, or post_small_kernel at Npad = 64) and over 256 CUs + 77 rows, where the variance kernel is
        (64, 33)  post_small_kernel, two 32-row slabs      (65, 40)  post_kernel_w4<4>, Npad 128        (129, 6)  tall, one n-tile
        (257, 3)  post_kernel_w4<4>, three blocks          (400, 33) tall, two tiles                    (640, 17) w4<4>, N = Npad
        (700, 6)  tall, three tiles                        (300, 65) w4<4>, the widest slab class (dpad 96)."""
    _single_fit_case(ctx, N, d, kern, [R.m_small(), R.m_large(cus)], "a")


@pytest.mark.parametrize("N,d,kern", R.CASES_B)
def test_b_small_regime_against_exact_arithmetic(ctx, N, d, kern):
    """kpost_small_kernel (Npad <= 128, d <= 32: K* never stored) at N = 63 ... 128 over 1037 rows: 65 strips of 16 candidates,
    the last one ragged."""
    _single_fit_case(ctx, N, d, kern, [R.m_small()], "b small")


@pytest.mark.parametrize("N,d,kern", R.CASES_B_GENERAL)
def test_b_small_sizes_through_the_general_path(gen, N, d, kern):
    """The same sizes with the small kernels switched off (diagnostic build): ksx_kernel + post_kernel_w4<2> at Npad = 128."""
    _single_fit_case(gen, N, d, kern, [R.m_small()], "b general")


@pytest.mark.parametrize("N,d,kern,S,large", R.CASES_C)
def test_c_fits_side_by_side_against_exact_arithmetic(ctx, cus, N, d, kern, S, large):
    """eval_posterior with S hyper samples, then posterior_get(s), every sample judged directly: (100, 6, 3) the small regime;
    (256, 6, 4) over 64 CUs + 77 rows the tall kernel with grid.y = fit; (300, 6, 4) post_kernel_w4<4> with grid.y = fit.  L^-1 and
    alpha of sample s come from a gp_fit with the same hypers on the same context beforehand."""
    X, Y, hyp = R.case_inputs(N, d)
    hyps = R.hyper_samples(hyp, S)
    M = R.m_large(cus, 4) if large else R.m_small()
    rows = R.judged_rows(M)
    G = R.make_grid(M, X)
    try:
        ctx.grid_upload(G)
        refs = []
        for h in hyps:
            Linv, alpha = _fit(ctx, X, Y, h, kern)
            refs.append(R.reference(X, h, kern, Linv, alpha, G, rows))
        ctx.gp_set_data(X, Y)
        rep = ctx.eval_posterior(hyps, want_report=True)
        assert (rep["jitter"] == 0).all(), rep
        for s in range(S):
            mu, var = ctx.posterior_get(s)
            _hold("c N %d d %d %s S %d M %d sample %d" % (N, d, kern, S, M, s), refs[s], rows, mu, var)
    finally:
        ctx.gp_set_kernel(R.SE)


def test_d_options_and_chunks_against_exact_arithmetic(ctx, cus):
    """(400, 33) over 256 CUs + 77 rows with the workspace cut so that the grid spans three chunks, the last one ragged (both sides
    of every boundary are judged): the latent variance; var_with_noise (the reference adds the noise); var_clamp with var_min at the
    median of the judged variances (the reference is max(var, var_min); a row within its bar of var_min may return either)."""
    N, d, kern = R.CASE_D
    X, Y, hyp = R.case_inputs(N, d)
    M, Npad = R.m_large(cus), R.npad_of(N)
    tiles = -(-M // 256)
    chunk = -(-2 * tiles // 5) * 256
    assert -(-M // chunk) >= 3 and (256 * tiles) % chunk != 0
    rows = R.judged_rows(M, chunk)
    assert {chunk - 1, chunk, 2 * chunk - 1, 2 * chunk} <= set(rows.tolist())
    G = R.make_grid(M, X)
    try:
        Linv, alpha = _fit(ctx, X, Y, hyp, kern)
        ref = R.reference(X, hyp, kern, Linv, alpha, G, rows)
        noisy = R.reference(X, hyp, kern, Linv, alpha, G, rows, with_noise=True, cov=ref.cov)
        ctx.grid_upload(G)
        ctx.set_workspace(8 * Npad * chunk)
        assert R.chunk_rows(8 * Npad * chunk, Npad, M) == chunk
        mu, var = ctx.gp_predict()
        _hold("d chunks of %d" % chunk, ref, rows, mu, var)
        ctx.gp_set_opts(var_with_noise=1)
        mu, var = ctx.gp_predict()
        _hold("d var_with_noise", noisy, rows, mu, var)
        vh, vl = ref.post.var
        vmin = float(np.median(vh))
        below, above = vh + ref.bar_v < vmin, vh - ref.bar_v > vmin
        assert below.any() and above.any()
        ctx.gp_set_opts(var_clamp=1, var_min=vmin)
        mu, var = ctx.gp_predict()
        got = var[rows]
        inside = E.abs_errors(got, vh, vl) <= ref.bar_v
        ok = np.where(below, got == vmin, np.where(above, inside, inside | (got == vmin)))
        print("d var_clamp at %.6g: %d rows clamped, %d not, %d within their bar of var_min" % (
            vmin, int(below.sum()), int(above.sum()), int((~below & ~above).sum())))
        assert ok.all(), ("var_clamp", rows[~ok].tolist())
        rm, _ = R.judge(ref, rows, mu[rows, 0], got)
        assert R.within(rm), ("var_clamp mean", rows[~(rm <= 1.0)].tolist())
    finally:
        ctx.gp_set_opts()
        ctx.set_workspace(R.WORKSPACE_DEFAULT)
        ctx.gp_set_kernel(R.SE)
