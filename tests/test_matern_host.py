"""CPU checks of the ARD Matern-5/2 covariance kernel (config.model.kernel = 'ardmatern52'): the C ABI declares and exports it,
the model mirror accepts it and nothing else new, the host references of tests/_matern_ref.py agree with scikit-learn and with
40-digit arithmetic, and the Lua shims select it.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _matern_ref as R
import bot7_amd
from bot7_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "bot7hip.h")).read()


def test_header_declares_the_kernel_setters_and_codes():
    h = _header()
    assert re.search(r"^int b7_gp_set_kernel\(b7_ctx \*ctx, int kernel\);", h, re.M)
    assert re.search(r"^int b7_group_gp_set_kernel\(b7_group \*g, int kernel\);", h, re.M)
    assert re.search(r"^#define B7_KERNEL_ARDSE 0\b", h, re.M) and re.search(r"^#define B7_KERNEL_MATERN52 1\b", h, re.M)
    assert re.search(r"^#define B7_ABI_VERSION 1\b", h, re.M)      # additive: the version stays
    # b7_hyp and b7_gp_opts keep their layout (hosts allocate them)
    assert [f for f, _ in _lib.Hyp._fields_] == ["lenscale_sq", "amp", "noise", "mean"]
    assert [f for f, _ in _lib.GpOpts._fields_] == ["jitter_eps", "jitter_growth", "var_with_noise", "var_clamp", "var_min"]


def test_library_exports_the_kernel_setters():
    lib = ctypes.CDLL(bot7_amd.lib_path())
    for name in ("b7_gp_set_kernel", "b7_group_gp_set_kernel"):
        assert hasattr(lib, name), name
        assert name in _lib.SYMBOLS
    L = _lib.load()
    assert L.b7_gp_set_kernel(None, 1) < 0 and L.b7_group_gp_set_kernel(None, 1) < 0    # NULL handle: an error code


def test_kernel_names_and_codes():
    assert _lib.kernel_code("ardse") == 0 and _lib.kernel_code("ardmatern52") == 1 and _lib.kernel_code(1) == 1
    for bad in ("foo", "matern52", 2, -1):
        with pytest.raises(bot7_amd.Bot7HipError):
            _lib.kernel_code(bad)


def test_model_accepts_ardmatern52_and_refuses_other_kernels():
    m = bot7_amd.models.gp_regressor({"kernel": "ardmatern52"})
    assert m.kernel == "ardmatern52"
    assert bot7_amd.models.gp_regressor({}).kernel == "ardse"
    with pytest.raises(NotImplementedError):
        bot7_amd.models.gp_regressor({"kernel": "foo"})
    with pytest.raises(NotImplementedError):
        bot7_amd.models.gp_regressor({"kernel": "ardmatern52", "nzModel": "other"})


def test_model_sets_its_kernel_on_the_context_before_each_library_call():
    """A stand-in context records the calls: a Matern model sets the kernel before the likelihood, the fit and the nomination's
    staging, an SE model on the same context sets it back; a context without kernels serves ardse only."""
    class Ctx(object):
        fit_token, grid_version = 0, 0

        def __init__(self):
            self.log, self.kernel = [], "ardse"

        def gp_set_kernel(self, k):
            if k != self.kernel:
                self.kernel = k
                self.fit_token += 1
            self.log.append(("kernel", k))

        def gp_set_data(self, X, Y):
            self.log.append(("data", self.kernel))

        def gp_nll1(self, ls, amp, noise, mean):
            self.log.append(("nll", self.kernel))
            return 1.0, 0.0, 0

        def gp_fit(self, X, Y, ls, amp, noise, mean, want_nll=False):
            self.log.append(("fit", self.kernel))
            return {"nll": np.zeros(1), "jitter": 0.0, "info": 0}

        def grid_shape(self):
            return (0, 0)

        def grid_upload(self, X):
            self.grid_version += 1

    ctx = Ctx()
    rng = np.random.default_rng(0)
    X, Y = rng.random((10, 2)), rng.random((10, 1))
    mat = bot7_amd.models.gp_regressor({"kernel": "ardmatern52"}, context=ctx)
    se = bot7_amd.models.gp_regressor({}, context=ctx)
    mat.init(X, Y)
    se.init(X, Y)
    mat.nll(X, Y)
    assert ("nll", "ardmatern52") in ctx.log
    se.fit(X, Y)
    assert ctx.log[-1] == ("fit", "ardse")
    mat.fit(X, Y)
    assert ctx.log[-1] == ("fit", "ardmatern52")
    se.stage(X, Y, rng.random((5, 2)))
    assert ctx.kernel == "ardse"

    class Bare(object):   # a host stand-in without kernels (the oracle's context)
        fit_token = 0
    with pytest.raises(NotImplementedError):
        bot7_amd.models.gp_regressor({"kernel": "ardmatern52"}, context=Bare())._use_kernel()
    bot7_amd.models.gp_regressor({}, context=Bare())._use_kernel()


def test_numpy_reference_equals_scikit_learn():
    from sklearn.gaussian_process.kernels import Matern
    rng = np.random.default_rng(3)
    for d in (1, 3, 6):
        X, Z = rng.random((40, d)), rng.random((30, d))
        ls = np.exp(rng.uniform(-3.0, 2.0, d))
        amp = 2.7
        got = R.matern52(X, Z, ls, amp)
        want = amp * Matern(length_scale=np.sqrt(ls), nu=2.5)(X, Z)
        assert np.max(np.abs(got - want) / np.abs(want)) < 1e-14
        Kxx = R.matern52(X, None, ls, amp)
        want = amp * Matern(length_scale=np.sqrt(ls), nu=2.5)(X)
        assert np.max(np.abs(Kxx - want) / np.abs(want)) < 1e-14
        assert np.allclose(np.diag(Kxx), amp, rtol=1e-14, atol=0)    # k(x, x) = amp, as for the SE (D = 0 up to the GEMM form's rounding)


def test_numpy_reference_on_exact_arguments_equals_mpmath():
    """On rows with an exact argument the reference's only error is the libm's and the rounding of s: within (4 + s) ulp, the
    bar the device is held to -- where amp exp(-s) is normal (below that numpy's amp m exp(-s) is built from a subnormal
    exp(-s) and loses bits: the reason the device applies m before the power of two)."""
    for d in (1, 6):
        X, args = R.matern_points(d, dense=600, seed=d)
        for amp in (2.0 ** -40, 1.0, 2.0 ** 40):
            hi, lo, s = R.matern_truth(amp, args)
            got = R.matern52(X, np.zeros((1, d)), np.ones(d), amp)[:, 0]
            keep = np.exp(-s) >= 2.0 ** -1022
            ok, wu, wa = R.within_matern_bar(got[keep], hi[keep], lo[keep], s[keep])
            assert ok, (d, amp, wu, wa)
    # the band s in [700, 760] is covered, with truths on both sides of the normal range
    X, args = R.matern_points(6, dense=200)
    hi, _, s = R.matern_truth(2.0 ** 40, args)
    band = (s >= 700) & (s <= 760)
    assert band.sum() >= 1000 and (np.abs(hi[band]) >= 2.0 ** -1022).any() and (np.abs(hi[band]) < 2.0 ** -1022).any()


def test_lapack_helpers_agree_with_the_50_digit_fit():
    """lapack_fit on the Matern K against the same algebra in mpmath (small N)."""
    import mpmath
    rng = np.random.default_rng(1)
    N, d = 8, 2
    X, Xs = rng.random((N, d)), rng.random((3, d))
    Y = np.sin(3 * X.sum(1, keepdims=True))
    ls, amp, noise, mean = np.array([0.3, 0.7]), 1.3, 1e-3, 0.1
    f = R.lapack_fit(X, Y, ls, amp, noise, mean, Xs)
    assert f["jitter"] == 0.0 and f["info"] == 0
    with mpmath.workdps(50):
        mpf = mpmath.mpf

        def k(a, b):
            s = mpmath.sqrt(5 * sum((mpf(float(a[i])) - mpf(float(b[i]))) ** 2 / mpf(float(ls[i])) for i in range(d)))
            return mpf(amp) * (1 + s + s * s / 3) * mpmath.exp(-s)
        K = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(N):
                K[i, j] = k(X[i], X[j]) + (mpf(noise) if i == j else 0)
        r = mpmath.matrix([mpf(float(v)) - mpf(mean) for v in Y[:, 0]])
        alpha = mpmath.lu_solve(K, r)
        nll = sum(r[i] * alpha[i] for i in range(N)) / 2 + mpmath.log(mpmath.det(K)) / 2 + N * mpmath.log(2 * mpmath.pi) / 2
        mu = [mpf(mean) + sum(k(x, X[i]) * alpha[i] for i in range(N)) for x in Xs]
    assert abs(f["nll"] - float(nll)) < 1e-10 * max(1.0, abs(float(nll)))
    assert np.allclose(f["mu"], [float(v) for v in mu], rtol=1e-9, atol=1e-12)


def test_lua_model_reads_config_kernel_and_sets_it():
    gp = open(os.path.join(ROOT, "lua", "models_gp_hip.lua")).read()
    assert "self.config.kernel" in gp and "hip.kernel_code(self.kernel)" in gp and "hip.set_kernel(self.kernel_code)" in gp
    ffi = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    body = ffi[ffi.index("function M.set_kernel("):]
    body = body[:body.index("\nend")]
    assert "C.b7_gp_set_kernel(M.ctx, code)" in body and "C.b7_group_gp_set_kernel(M.group, code)" in body
    assert "ardmatern52 = M.KERNEL_MATERN52" in ffi and "M.KERNEL_MATERN52 = 1" in ffi
    assert "error(" in ffi[ffi.index("function M.kernel_code("):]
    bt = open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read()
    assert bt.index("hip.set_kernel(model.kernel_code)") < bt.index("b7_group_eval_nominate")
    # the group path: use_group hands the kernel chosen so far to every member
    ug = ffi[ffi.index("function M.use_group("):]
    assert "M.set_kernel(k)" in ug[:ug.index("\nend")]
