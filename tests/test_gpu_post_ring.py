"""The tall posterior kernel (post_kernel_w4t: 256-row n-tiles, operands staged by LDS-DMA into a ring of three stage
images) at the smallest shapes at which the ring can go wrong.  Needs an MI355X: run with -m gpu.

A tile of the stream has 16 (t + 1) stages, so the ring position at a tile switch is not a multiple of three: N <= 256
is one tile (diagonal stages only), 257..512 two, 513..768 three.  The reference is the 128-candidate kernel
(post_kernel_w4<2>: register staging, two buffers), which runs whenever the grid has fewer than one 256-candidate
workgroup per CU, and the CPU oracle.  The same shapes against exact arithmetic, with bars below 1e-9 of the scale instead of the
1e-5 here: tests/test_gpu_post_exact.py."""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu
REL = 1e-5  # north_star tolerance for posterior mean / variance (tests/test_gpu_parity.py)
D, M = 3, 65536 + 77


def _objective(X):
    return np.sin(3.0 * X).sum(axis=1, keepdims=True)


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.max(np.abs(a - b) / np.abs(b)))


@pytest.mark.parametrize("N", [200, 256, 400, 512, 700])
def test_tall_route_equals_the_128_candidate_route_and_the_oracle(ctx, orc, N):
    X_obs, Y, X_hid, hyp = make_problem(None, orc, D, N, M, _objective)
    ctx.grid_upload(X_hid)                  # >= one 256-candidate workgroup per CU: the tall kernel
    ctx.gp_fit(X_obs, Y, **hyp)
    mu, var = ctx.gp_predict()
    ctx.grid_upload(X_hid[:4096])           # fewer: the 128-candidate kernel
    mu_s, var_s = ctx.gp_predict()
    assert np.array_equal(var[:4096], var_s) and np.array_equal(mu[:4096], mu_s)
    f = orc.gp.fit(X_obs, Y, **hyp)
    idx = np.linspace(0, M - 1, 300).astype(int)
    _, var_o = orc.gp.predict(f, X_hid[idx])
    assert relerr(var[idx], var_o) < REL


def test_four_fits_side_by_side_equal_the_per_sample_loop(ctx, orc):
    """S = 4, N = 256, 16 384 candidates: 64 workgroups of 256 candidates x 4 fits = one per CU, so eval_nominate runs the
    tall kernel with grid.y = fit (strided L^-1, K*, output); a single fit over the same grid runs the 128-candidate one."""
    N, Mg, S = 256, 16384, 4
    X_obs, Y, X_hid, hyp = make_problem(ctx, orc, D, N, Mg, _objective)
    hyps = [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.25 * s), amp=hyp["amp"] * (1.0 + 0.1 * s)) for s in range(S)]
    fmin = [float(Y.min())]
    ctx.grid_upload(X_hid)
    for s, h in enumerate(hyps):
        ctx.gp_fit(X_obs, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
        ctx.gp_predict(download=False)
        if s == 0:
            ctx.score_reset()
        ctx.score_ei(fmin, 0.0)
    val0, idx0, scores0 = ctx.score_finish(float(S), download=True)
    ctx.gp_set_data(X_obs, Y)
    val1, idx1 = ctx.eval_nominate(hyps, score="ei", fmin=fmin)
    _, _, scores1 = ctx.score_finish(1.0, download=True)
    assert (val1, idx1) == (val0, idx0)
    assert np.array_equal(scores1, scores0)


def test_a_repeated_prediction_sees_nothing_of_the_one_before(ctx, orc):
    """The same prediction three times in one process, another problem of another N predicted in between: whatever a
    launch leaves in LDS or in flight must not reach the next one."""
    A = make_problem(None, orc, D, 400, M, _objective)
    B = make_problem(None, orc, D, 700, M, lambda X: np.cos(2.0 * X).sum(axis=1, keepdims=True), seed_skip=5)

    def predict(P):
        X_obs, Y, X_hid, hyp = P
        ctx.grid_upload(X_hid)
        ctx.gp_fit(X_obs, Y, **hyp)
        return ctx.gp_predict()

    mu0, var0 = predict(A)
    predict(B)
    mu1, var1 = predict(A)
    predict(B)
    mu2, var2 = predict(A)
    assert np.array_equal(var0, var1) and np.array_equal(var0, var2)
    assert np.array_equal(mu0, mu1) and np.array_equal(mu0, mu2)
