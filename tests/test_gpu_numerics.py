"""The GP and basis kernels across the sampler's hyper box against exact arithmetic (mpmath) and exact invariances, on both
paths: 'small' (the default library at N <= 128, d <= 32: gp_small_kernel, kpost_small_kernel, nll_small_kernel,
score_finish_slot_kernel) and 'general' (the diagnostic build with B7_FIT_SMALL=0 B7_KPOST_SMALL=0 B7_NLL_SMALL=0: observation
scaling, ksx_kernel, persistent Cholesky, post_kernel).  Host references: tests/_exact.py (checked by tests/test_exact_helpers.py)."""
import functools
import math
import os

import numpy as np
import pytest
from scipy.linalg import lapack, solve_triangular

import _exact as E
from oracle import cport, gp

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


def _path(request, name):
    return request.getfixturevalue("ctx" if name == "small" else "gen")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


# ---- A. the covariance exponential over its whole domain ------------------------------------------------------------------
AMPS = (2.0 ** -40, 1e-3, 1.0, 3.0, 1e3, 2.0 ** 40)


@functools.lru_cache(maxsize=None)
def _ksx_points(d):
    X, args = E.exp_points(E.exp_targets(dense=40000, seed=d), d, 0)
    Xs, sargs = E.special_exp_rows(d)
    return np.concatenate([X, Xs]), args + sargs


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_cross_covariance_exponential_against_mpmath(request, path, d):
    """K(X*, X) of one observation at the origin: mu = K* alpha = amp exp(arg) alpha for ~47 000 exact arguments per d (a dense
    sweep of [-1000, 0], every table residue at n >> 7 in {0, -1, -3, -40, -200, -1000}, [-745, -708], -1000 and below, -0.0,
    -2^-1001), amp in 2^-40 .. 2^40.  Bar: 4 ulp of the true value where it is normal, 2^-1073 absolute below.  Measured on an
    MI355X, both paths: at most 1.75 ulp (normal), 2^-1074 absolute (subnormal).  A NaN and an inf coordinate give the
    oracle's non-finite pattern in their rows and leave every other row's bits alone."""
    c = _path(request, path)
    Xc, args = _ksx_points(d)
    worst = (0.0, 0.0)
    for amp in AMPS:
        top = 4.0 ** math.ceil(math.log(amp, 4))       # amp + noise a power of 4 and y = amp + noise: alpha = 1 where it rounds so
        noise = top - amp
        c.grid_upload(Xc)
        c.gp_fit(np.zeros((1, d)), np.array([[top]]), np.ones(d), amp, noise, 0.0)
        _, alpha, _ = c.gp_download(1)
        mu, var = c.gp_predict()
        a = float(alpha[0, 0])
        with E.mpmath.workdps(40):
            hi, lo = E.pairs([E.mpmath.mpf(amp) * E.mpmath.exp(E.mpmath.mpf(t.numerator) / t.denominator) * a for t in args])
        ok, wu, wa = E.within_bar(mu[:, 0], hi, lo, 4)
        worst = (max(worst[0], wu), max(worst[1], wa))
        assert ok, "%s d %d amp %g: %.2f ulp, %.3g abs" % (path, d, amp, wu, wa)
        # non-finite coordinates: two rows replaced in the middle of a tile, the oracle's pattern there, the other rows' bits kept
        bad = Xc.copy()
        i0 = 1000
        bad[i0, d - 1] = np.nan
        bad[i0 + 1, 0] = np.inf
        c.grid_upload(bad)
        mu2, var2 = c.gp_predict()
        f = gp.fit(np.zeros((1, d)), np.array([[top]]), np.ones(d), amp, noise, 0.0)
        with np.errstate(invalid="ignore", over="ignore"):
            mo, vo = gp.predict(f, bad[i0:i0 + 2])
        for g, o in ((mu2[i0:i0 + 2, 0], mo[:, 0]), (var2[i0:i0 + 2], vo)):
            assert np.array_equal(np.isnan(g), np.isnan(o)) and np.array_equal(np.isinf(g), np.isinf(o)), (g, o)
        keep = np.ones(len(Xc), dtype=bool)
        keep[i0:i0 + 2] = False
        assert _bits(mu2[keep]) == _bits(mu[keep]) and _bits(var2[keep]) == _bits(var[keep])
    print("K(X*,X) %s d %d: worst %.3f ulp normal, %.3g absolute subnormal" % (path, d, worst[0], worst[1]))


@functools.lru_cache(maxsize=None)
def _kxx_points(d):
    X, args = E.exp_points(E.exp_targets(dense=1500, seed=100 + d), d, 0)
    Xs, sargs = E.special_exp_rows(d)
    return np.concatenate([X, Xs]), args + sargs


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("d", [1, 6, 32])
def test_observation_covariance_exponential_against_mpmath(request, path, d):
    """K(X, X): observation 0 at the origin, amp = 3, noise = 1, so L00 = 2 and column 0 of L is K[:, 0] / 2: 127 exact
    arguments per fit at N = 128, ~3 000 in all per d.  Same bar as above; measured on an MI355X: at most 2.0 ulp (d = 32), 2^-1074
    absolute in the subnormal range."""
    c = _path(request, path)
    Xc, args = _kxx_points(d)
    with E.mpmath.workdps(40):
        hi, lo = E.pairs([3 * E.mpmath.exp(E.mpmath.mpf(t.numerator) / t.denominator) for t in args])
    got = np.empty(len(args))
    for s in range(0, len(args), 127):
        rows = Xc[s:s + 127]
        X = np.concatenate([np.zeros((1, d)), rows])
        rep = c.gp_fit(X, np.zeros((len(X), 1)), np.ones(d), 3.0, 1.0, 0.0)
        assert rep["jitter"] == 0
        L, _, _ = c.gp_download(len(X))
        assert L[0, 0] == 2.0
        got[s:s + len(rows)] = 2.0 * L[1:, 0]
    ok, wu, wa = E.within_bar(got, hi, lo, 4)
    print("K(X,X) %s d %d: worst %.3f ulp normal, %.3g absolute subnormal" % (path, d, wu, wa))
    assert ok, "%s d %d: %.2f ulp, %.3g abs" % (path, d, wu, wa)


# ---- B. activations in each basis kernel ------------------------------------------------------------------------------------
ROUTES = {"resident4": (1, 16), "resident8": (1, 128), "mfma": (128, 128), "general": (1, 256)}
ACT_BAR = {"Tanh": 6.0, "Sigmoid": 4.0, "ReLU": 0.0}


@functools.lru_cache(maxsize=None)
def _act_truth(kind):
    xs = E.activation_inputs()
    return xs, E.activation_truth(kind, xs)


@pytest.mark.parametrize("kind", ["Tanh", "Sigmoid", "ReLU"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_activations_against_mpmath_in_every_basis_kernel(ctx, route, kind):
    """launch_mlp_forward_mean's three kernels -- resident weights (tanh_fast4; NT_MAX 4 at width 16, 8 at width 128),
    mlp_forward_mfma_kernel (d = 128 into 128 units: the weights do not fit in LDS) and mlp_forward_kernel (256 units) -- with
    weights that make every preactivation exactly an input: d = 1 with unit weights and zero biases, or the identity at d = 128.
    Inputs: +-0, +-subnormals, +-1e-8 .. 1e-300, [-30, 30], around |x| = 22.5, +-inf, NaN.  Bars: tanh 6 ulp, sigmoid 4, ReLU
    exact; non-finite values and signed zeros as the oracle's numpy forward pass.  A -0 preactivation reaches only
    mlp_forward_kernel (its sum starts at the bias, so a -0 bias carries -0 through): the resident and MFMA kernels add into
    accumulators that start at +0, where -0 + +0 = +0, so tanh_fast4 never sees -0 through the API; its copysign is checked
    on the smallest negative inputs instead.  Measured on an MI355X: tanh_fast4 at most
    2.9 ulp, libm tanh 0.8, sigmoid 1.9, ReLU exact (ReLU of NaN was 0 before it was made to pass NaN)."""
    d, w = ROUTES[route]
    xs, (hi, lo) = _act_truth(kind)
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324])
    if d == 1:
        W, b = [np.ones((w, 1))], [np.zeros(w)]
        X = np.concatenate([xs, special]).reshape(-1, 1)
        Z = ctx.blr_basis(W, b, kind, X=X)
        assert Z.shape == (len(X), w)
        assert all(_bits(Z[:, k]) == _bits(Z[:, 0]) for k in range(1, w))
        got = Z[:len(xs), 0]
        gs = Z[len(xs):, 0]
    else:
        W, b = [np.eye(d)], [np.zeros(d)]
        pad = (-len(xs)) % d
        X = np.concatenate([xs, np.zeros(pad)]).reshape(-1, d)
        Xsp = np.zeros((len(special), d))
        Xsp[:, 5] = special                      # a non-finite input makes every unit of its row NaN (inf * 0), as in numpy
        Z = ctx.blr_basis(W, b, kind, X=np.concatenate([X, Xsp]))
        got = Z[:len(X)].ravel()[:len(xs)]
        gs = Z[len(X):]
        X = np.concatenate([X, Xsp])
    # non-finite inputs and signed zeros: the oracle's forward pass bit for bit (NaN as NaN)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = E.numpy_activation(kind, X @ W[0].T + b[0])
    ref_s = ref[-len(special):, 0] if d == 1 else ref[-len(special):]
    assert np.array_equal(np.isnan(gs), np.isnan(ref_s)), (gs, ref_s)
    fin = ~np.isnan(ref_s)
    assert np.array_equal(gs[fin], ref_s[fin]) and np.array_equal(np.signbit(gs[fin]), np.signbit(ref_s[fin])), (gs, ref_s)
    zero = got == 0
    ref_main = ref[:len(xs), 0] if d == 1 else ref[:-len(special)].ravel()[:len(xs)]
    assert np.array_equal(np.signbit(got[zero]), np.signbit(ref_main[zero]))
    if kind == "Tanh":      # the sign of every nonzero input survives, down to -5e-324 (the subnormal bar alone would allow 0)
        nz = xs != 0
        assert np.array_equal(np.signbit(got[nz]), np.signbit(xs[nz])) and not (got[nz] == 0).any()
    if route == "general":  # mlp_forward_kernel starts its sum at the bias: a -0 bias carries -0 into the activation
        Z0 = ctx.blr_basis([np.ones((w, 1))], [np.full(w, -0.0)], kind, X=np.array([[-0.0], [0.0]]))[:, 0]
        want = E.numpy_activation(kind, np.array([-0.0, 0.0]))       # fma(1, -0, -0) = -0; fma(1, +0, -0) = +0
        assert _bits(Z0) == _bits(want), (kind, Z0, want)
    ok, wu, wa = E.within_bar(got, hi, lo, ACT_BAR[kind], sub_bar=0.0 if kind == "ReLU" else E.SUB_BAR)
    print("%s %s: worst %.3f ulp, %.3g absolute" % (route, kind, wu, wa))
    assert ok, "%s %s: %.2f ulp (bar %g), %.3g abs" % (route, kind, wu, ACT_BAR[kind], wa)


# ---- C. fits across the sampler's box against 50-digit arithmetic ----------------------------------------------------------
def _data(N, d, v, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0]) + 0.05 * rng.normal(size=N)
    if N > 1:
        y = (y - y.mean()) / y.std()
    Y = (np.sqrt(v) * y + 0.5 * np.sqrt(v)).reshape(-1, 1)
    return X, Y, rng.random((32, d))


def _box(X, Y):
    """bot7_amd/models/gp_regressor.py:_bounds_compute with its defaults (natural units)."""
    d, vy = X.shape[1], float(np.var(Y)) or 1.0
    lo = dict(ls=1e-3 * d, amp=1e-3 * vy, noise=1e-8 * vy, mean=float(Y.min()) - 3 * math.sqrt(vy))
    hi = dict(ls=1e3 * d, amp=1e3 * vy, noise=vy, mean=float(Y.max()) + 3 * math.sqrt(vy))
    return lo, hi


def _hyps(X, Y, n_interior, seed):
    lo, hi = _box(X, Y)
    d = X.shape[1]
    out = []
    for bits in range(16):
        pick = [hi if bits >> i & 1 else lo for i in range(4)]
        out.append({"lenscale_sq": np.full(d, pick[0]["ls"]), "amp": pick[1]["amp"], "noise": pick[2]["noise"],
                    "mean": pick[3]["mean"]})
    rng = np.random.default_rng(seed)
    for _ in range(n_interior):
        u = rng.random(d + 3)
        g = {k: math.exp(math.log(lo[k]) + u[i] * (math.log(hi[k]) - math.log(lo[k]))) for i, k in enumerate(("amp", "noise"))}
        out.append({"lenscale_sq": np.exp(np.log(lo["ls"]) + u[2:2 + d] * (np.log(hi["ls"]) - np.log(lo["ls"]))), "amp": g["amp"],
                    "noise": g["noise"], "mean": lo["mean"] + u[-1] * (hi["mean"] - lo["mean"])})
    return out


def _cases():
    cases = []
    for N, d in ((2, 1), (16, 2), (40, 6)):
        for iv, v in enumerate((1e-6, 1.0, 1e6)):
            X, Y, Xs = _data(N, d, v, seed=10 * N + iv)
            hyps = _hyps(X, Y, 3, seed=N + iv)
            if N == 40:               # mpmath at N = 40 costs ~15x N = 16: a seeded subset of the corners + one interior point
                keep = np.random.default_rng(iv).choice(16, 2, replace=False).tolist() + [16]
                hyps = [hyps[i] for i in keep]
            cases.append((N, d, v, X, Y, Xs, hyps))
    return cases


_TRUTH = {}


def _truth(key, X, Y, h, Xs, jitter):
    k = (key, jitter)
    if k not in _TRUTH:
        _TRUTH[k] = E.gp_truth(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xs, jitter=jitter)
    return _TRUTH[k]


def _K(X, h):
    K = gp.ardse(X, None, h["lenscale_sq"], h["amp"])
    K[np.diag_indices(len(X))] += h["noise"]
    return K


def _check_verdict(X, h, jitter):
    """The device's jitter is one of the schedule's values, and where its verdict on the plain attempt differs from LAPACK's,
    LAPACK's smallest pivot is within N eps ||K|| of zero."""
    K = _K(X, h)
    nrm = float(np.linalg.norm(K))
    if jitter > 0:
        assert jitter in E.jitter_schedule(nrm), jitter
    _, info = lapack.dpotrf(K, lower=1, clean=1)
    if (info != 0) != (jitter != 0):
        assert abs(E.min_pivot(K)) <= len(X) * E.EPS * nrm, (jitter, info, E.min_pivot(K), nrm)


def _check_gave_up(X, h):
    """The device went through the whole jitter schedule to chol(I): LAPACK must fail at the schedule's last jitter too, or
    have its smallest pivot there within N eps ||K|| of zero."""
    K = _K(X, h)
    nrm = float(np.linalg.norm(K))
    Kj = K.copy()
    Kj[np.diag_indices(len(X))] += E.jitter_schedule(nrm)[-1]
    _, info = lapack.dpotrf(Kj, lower=1, clean=1)
    if info == 0:
        assert abs(E.min_pivot(Kj)) <= len(X) * E.EPS * nrm, ("device gave up on a K that LAPACK factors", E.min_pivot(Kj), nrm)


RATIOS = {}


def _judge(path, what, got, truth, orcs, scale):
    """orcs: LAPACK on K and on K with its off-diagonal covariances 1 ulp either way -- the device's K is assembled to within 2
    ulp (section A), and at the box's worst corners (N = 2, lenscale_sq = 1e3 d, amp = 1e-3 var(Y), noise = 1e-8 var(Y)) one
    ulp there moves LAPACK's own NLL by 3e-4 while its error on the exactly rounded K is 8e-6: the device's 1e-4 measures
    the K entry, not the factorisation."""
    e_g, e_o = E.err_vs(got, truth), max(E.err_vs(o, truth) for o in orcs)
    floor = 16 * E.EPS * scale
    r = RATIOS.setdefault(path, {}).setdefault(what, [[], []])
    r[0].append(e_g / max(e_o, floor))                          # against the yardstick the bar uses
    r[1].append(e_g / max(E.err_vs(orcs[0], truth), floor))     # against LAPACK on the host's K alone: the loosening stays visible
    assert e_g <= E.gp_bar(e_o, scale), "%s %s: GPU error %.3g, LAPACK %.3g, scale %.3g" % (path, what, e_g, e_o, scale)


@pytest.mark.parametrize("path", ["small", "general"])
def test_fits_across_the_hyper_box_against_50_digit_arithmetic(request, path):
    """Corners of the sampler's box (lenscale_sq, amp, noise, mean each at a bound) plus seeded interior points, var(Y) in
    {1e-6, 1, 1e6}, (N, d) in {(2, 1), (16, 2), (40, 6)}, M = 32: the NLL of gp_fit, gp_nll_batch (all hypers of a data set in one
    batch) and gp_nll1, posterior mean and variance, and the EI / CB nominees of eval_nominate (S = 1, 3).  Bar: GPU error <= 8 x
    LAPACK's error on the same algebra + 16 eps scale; the worst ratio GPU / LAPACK error is printed per path."""
    c = _path(request, path)
    for ci, (N, d, v, X, Y, Xs, hyps) in enumerate(_cases()):
        c.gp_set_data(X, Y)
        ls = np.array([h["lenscale_sq"] for h in hyps])
        nb, jb, _ = c.gp_nll_batch(ls, [h["amp"] for h in hyps], [h["noise"] for h in hyps], [h["mean"] for h in hyps],
                                   want_info=True)
        for hi_, h in enumerate(hyps):
            key = (ci, hi_)
            n1, j1, _ = c.gp_nll1(h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
            c.grid_upload(Xs)
            rep = c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
            jit = rep["jitter"]
            assert jb[hi_] == jit and j1 == jit
            if jit < 0:       # fell through to chol(I): LAPACK must not have managed either; nothing to compare with 50 digits
                _check_gave_up(X, h)
                continue
            _check_verdict(X, h, jit)
            mu, var = c.gp_predict()
            orcs = [E.lapack_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], Xs, jitter=jit, kscale=ks)
                    for ks in (1.0, 1.0 - E.EPS, 1.0 + E.EPS)]
            orcs = [o for o in orcs if o is not None]
            if not orcs:      # LAPACK cannot factor what the device did: no yardstick
                continue
            t = _truth(key, X, Y, h, Xs, jit)
            scale_n = abs(float(t.nll))
            for what, g in (("fit nll", rep["nll"][0]), ("batch nll", nb[hi_]), ("nll1", n1)):
                _judge(path, what, [g], [t.nll], [[o[0]] for o in orcs], scale_n)
            _judge(path, "mean", mu[:, 0], t.mu, [o[1] for o in orcs], math.sqrt(h["amp"]) + abs(h["mean"]))
            _judge(path, "var", var, t.var, [o[2] for o in orcs], h["amp"])
        # nominees: S = 1 (each hyper) and S = 3 (the first three), EI and CB, where the truth's top-2 gap clears the bar
        fmin = float(Y.min())
        for S, group in [(1, [i]) for i in range(len(hyps))] + [(3, [0, 1, 2])]:
            c.gp_set_data(X, Y)
            c.grid_upload(Xs)
            for kind in ("ei", "cb"):
                val, idx, rep = c.eval_nominate([hyps[i] for i in group], score=kind, fmin=[fmin], want_report=True)
                if (rep["jitter"] != 0).any():
                    continue
                acc_t, acc_o = np.zeros(len(Xs)), np.zeros(len(Xs))
                for i in group:
                    t = _truth((ci, i), X, Y, hyps[i], Xs, 0.0)
                    orc = E.lapack_fit(X, Y, hyps[i]["lenscale_sq"], hyps[i]["amp"], hyps[i]["noise"], hyps[i]["mean"], Xs)
                    if orc is None:
                        break
                    mt, vt = E.pairs(t.mu)[0], E.pairs(t.var)[0]
                    sc = (lambda m, s: cport.ei(m, s, [fmin])) if kind == "ei" else (lambda m, s: cport.cb(m, s))
                    cport.accumulate(acc_t, sc(mt, vt))
                    cport.accumulate(acc_o, sc(orc[1], orc[2]))
                else:
                    scale = max(1.0, float(np.abs(acc_t).max()))
                    bar = 8 * float(np.abs(acc_o - acc_t).max()) + 16 * E.EPS * scale * len(group)
                    top = np.sort(acc_t)[-2:]
                    if len(Xs) > 1 and top[1] - top[0] > 2 * bar:
                        assert idx == cport.argmax_first(acc_t)[0], (path, ci, S, kind)
    for k, (vs_bar, vs_plain) in RATIOS.get(path, {}).items():
        print("%s %s: worst GPU/LAPACK error ratio %.3f (yardstick of the bar), %.3f (LAPACK on K alone)"
              % (path, k, max(vs_bar), max(vs_plain)))


def _k_corners(X, Y):
    """The eight covariance corners of the box (bit 0: lenscale_sq, bit 1: amp, bit 2: noise; mean does not enter K), with
    lenscale_sq at the powers of 4 just inside its bounds (4^-3 and 4^6 at d = 6, against 6e-3 and 6e3)."""
    lo, hi = _box(X, Y)
    d = X.shape[1]
    ls = (4.0 ** math.ceil(math.log(lo["ls"], 4)), 4.0 ** math.floor(math.log(hi["ls"], 4)))
    return [{"lenscale_sq": np.full(d, ls[i & 1]), "amp": (lo, hi)[i >> 1 & 1]["amp"], "noise": (lo, hi)[i >> 2 & 1]["noise"],
             "mean": lo["mean"]} for i in range(8)]


K_GAP = 3 * E.EPS   # ||K_device - K_host||_F / ||K||_F on the grid: each off-diagonal entry within 3 ulp, the diagonals equal
# At cond(K) >= 1e10 (corner 3: K ~ amp 11^T + 1e-8 var(Y) I) the device's factor has a larger residual than LAPACK's, and that
# is the factorisation, not K: b7_chol of the host's own K gives the same 1.5e-15 at N = 100 (LAPACK 1.4e-16).  Measured there:
# the pivots and column 0 within 2 ulp of LAPACK's, the entry residuals of L L^T - K growing with the column (mean 6.8 ulp, 8.2
# over the trailing 70 x 70, at most 109), which is what accumulating the Schur update sum_k L_ik L_jk at amp's magnitude before
# subtracting it from K gives.  Backward stable (far below N eps), but up to 11x LAPACK's; for those corners only the factor's
# bar is 8 eps, 5x the worst measured (N = 100: 1.54e-15, 129: 1.10e-15, 700: 0.93e-15).
NEAR_SINGULAR_FACTOR = 8 * E.EPS


@pytest.mark.parametrize("path,N,picks", [("small", 100, range(8)), ("general", 129, range(8)), ("general", 700, (0, 1, 3, 7))])
def test_factors_at_the_corners_have_lapack_sized_backward_errors(request, path, N, picks):
    """N = 100 (small) and 129, 700 (general, the persistent multi-tile Cholesky) at the covariance corners of the box, the near-
    singular ones (large lenscale_sq, small noise: cond(K) ~ 1e7 and ~ 1e13) included, where 50 digits are too slow.
    ||L L^T - (K + jI)||_F / ||K||_F and ||L^-1 L - I||_F in long double, each <= 4 x LAPACK's on the same K; the factor's
    bar also carries K_GAP, the documented distance between the device's K and the host's on grid inputs (3 eps), and at
    cond(K) >= 1e10 it is 8 eps instead of 4 x LAPACK's where that is larger (NEAR_SINGULAR_FACTOR: the evidence is there)."""
    c = _path(request, path)
    X, Y = E.grid_data(N, 6, seed=N)
    hyps = _k_corners(X, Y)
    compared = []
    for i in picks:
        h = hyps[i]
        rep = c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
        jit = rep["jitter"]
        if jit < 0:
            _check_gave_up(X, h)
            continue
        _check_verdict(X, h, jit)
        L, _, Li = c.gp_download(N)
        K = _K(X, h)
        Kj = K.copy()
        Kj[np.diag_indices(N)] += jit
        Ll, info = lapack.dpotrf(Kj, lower=1, clean=1)
        if info != 0:       # LAPACK fails where the device succeeded: _check_verdict has put its pivot at zero
            continue
        Lli = solve_triangular(Ll, np.eye(N), lower=True)
        g, o = E.backward_errors(K, L, Li, jit), E.backward_errors(K, Ll, Lli, jit)
        cond = np.linalg.cond(Kj)
        print("%s N %d corner %d: cond %.1e jitter %g: factor %.3g (LAPACK %.3g), inverse %.3g (LAPACK %.3g)"
              % (path, N, i, cond, jit, g[0], o[0], g[1], o[1]))
        bar = max(4 * o[0], NEAR_SINGULAR_FACTOR if cond >= 1e10 else 0.0) + K_GAP
        assert g[0] <= bar and g[1] <= 4 * o[1], (path, N, i, g, o)
        if cond >= 1e10 and N <= 129:     # the same K as LAPACK's, factored on the device: no K gap in the bar
            Lc, jc, _ = c.chol(Kj)
            gc = E.backward_errors(Kj, Lc, np.linalg.inv(np.tril(Lc)), 0.0)[0] if jc == 0 else None
            print("  b7_chol of the host's K: factor %s" % gc)
            assert jc == 0 and gc <= max(4 * o[0], NEAR_SINGULAR_FACTOR), (gc, o[0])
        compared.append(i)
    assert 1 in compared and 3 in compared, "the near-singular corners were not compared: %s" % compared


# ---- D. exact invariances --------------------------------------------------------------------------------------------------
def _inv_problem(N=40, d=3, M=2000):
    rng = np.random.default_rng(77)
    X, Xs = rng.random((N, d)), rng.random((M, d))
    Y = np.sin(3.0 * X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, 1))
    hyp = {"lenscale_sq": np.array([0.3, 0.5, 0.2]), "amp": 1.3, "noise": 1e-3, "mean": 0.1}
    return X, Y, Xs, hyp


def _hyp_set(h, S):
    return [dict(h, lenscale_sq=h["lenscale_sq"] * (1 + 0.05 * s), amp=h["amp"] * (1 + 0.03 * s)) for s in range(S)]


def _everything(c, X, Y, Xs, h):
    N = len(X)
    out = {}
    rep = c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
    assert rep["jitter"] == 0
    out["L"], out["alpha"], out["Linv"] = c.gp_download(N)
    out["nll"] = rep["nll"]
    c.gp_set_data(X, Y)
    hs = _hyp_set(h, 3)
    out["nll_batch"] = c.gp_nll_batch(np.array([x["lenscale_sq"] for x in hs]), [x["amp"] for x in hs], [x["noise"] for x in hs],
                                      [x["mean"] for x in hs])
    c.grid_upload(Xs)
    c.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    out["mu"], out["var"] = c.gp_predict()
    c.gp_set_data(X, Y)
    for kind in ("ei", "cb"):
        for S in (1, 10):
            val, idx, rep = c.eval_nominate(_hyp_set(h, S), score=kind, fmin=[float(Y.min())], want_report=True)
            assert (rep["jitter"] == 0).all()
            out["%s%d" % (kind, S)] = c.score_finish(1.0, download=True)[2]
            out["%s%d_idx" % (kind, S)] = idx
    return out


@pytest.mark.parametrize("path", ["small", "general"])
def test_y_scaling_is_exact(request, path):
    """Y and mean x 2^k, amp and noise x 4^k (k in -20, -3, 5, 20): L x 2^k, L^-1 and alpha x 2^-k, mu x 2^k, var x 4^k, EI / CB
    scores x 2^k bit for bit, the same nominee, and the NLL shifted by N k ln 2 to within a few ulp."""
    c = _path(request, path)
    X, Y, Xs, hyp = _inv_problem()
    base = _everything(c, X, Y, Xs, hyp)
    for k in (-20, -3, 5, 20):
        h2, Y2 = E.scale_y(hyp, Y, k)
        o = _everything(c, X, Y2, Xs, h2)
        for q, e in (("L", k), ("alpha", -k), ("Linv", -k), ("mu", k), ("var", 2 * k), ("ei1", k), ("ei10", k), ("cb1", k),
                     ("cb10", k)):
            want = np.ldexp(base[q], e)
            # gradual underflow is not scale-exact: an EI far below fmin that is (or becomes) subnormal is rounded once at its
            # own size, so there the bar is one subnormal ulp at the smaller of the two scales; every normal value matches bit for bit
            sub = (np.abs(base[q]) < E.TINY) | (np.abs(want) < E.TINY)
            assert _bits(o[q][~sub]) == _bits(want[~sub]), "%s k %d: %s differs in %d places" % (
                path, k, q, int((o[q][~sub] != want[~sub]).sum()))
            assert np.all(np.abs(o[q][sub] - want[sub]) <= 2.0 ** (-1074 + max(k, 0))), (path, k, q)
        for q in ("ei1_idx", "ei10_idx", "cb1_idx", "cb10_idx"):
            assert o[q] == base[q], (path, k, q)
        for q in ("nll", "nll_batch"):
            shift = np.asarray(o[q]) - np.asarray(base[q])
            tol = 8 * E.EPS * np.maximum(np.abs(o[q]), np.abs(base[q]))
            assert np.all(np.abs(shift - len(X) * k * math.log(2.0)) <= tol), (path, k, q, shift)


@pytest.mark.parametrize("path", ["small", "general"])
def test_x_scaling_is_exact(request, path):
    """X and the candidates x 2^j, lenscale_sq x 4^j (j in -4, 3): every result identical bit for bit."""
    c = _path(request, path)
    X, Y, Xs, hyp = _inv_problem()
    base = _everything(c, X, Y, Xs, hyp)
    for j in (-4, 3):
        h2, X2 = E.scale_x(hyp, X, j)
        _, Xs2 = E.scale_x(hyp, Xs, j)
        o = _everything(c, X2, Y, Xs2, h2)
        for q in base:
            assert _bits(np.asarray(o[q])) == _bits(np.asarray(base[q])), "%s j %d: %s" % (path, j, q)


@pytest.mark.parametrize("path", ["small", "general"])
@pytest.mark.parametrize("M", [1000, 65537])
def test_candidate_permutation_is_exact(request, path, M):
    """The grid reversed, and shuffled by a seeded permutation: each candidate's mu, var and EI / CB score (S = 1, 10) are the
    same bits at its new position, and a unique nominee maps through the permutation."""
    c = _path(request, path)
    X, Y, _, hyp = _inv_problem()
    Xs = np.random.default_rng(M).random((M, X.shape[1]))

    def run(G):
        c.grid_upload(G)
        c.gp_fit(X, Y, hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        o = dict(zip(("mu", "var"), c.gp_predict()))
        c.gp_set_data(X, Y)
        for kind in ("ei", "cb"):
            for S in (1, 10):
                _, idx = c.eval_nominate(_hyp_set(hyp, S), score=kind, fmin=[float(Y.min())])
                o["%s%d" % (kind, S)] = c.score_finish(1.0, download=True)[2]
                o["%s%d_idx" % (kind, S)] = idx
        return o

    base = run(Xs)
    for perm in (np.arange(M)[::-1].copy(), np.random.default_rng(3).permutation(M)):
        o = run(Xs[perm])
        for q in ("mu", "var", "ei1", "ei10", "cb1", "cb10"):
            assert _bits(o[q]) == _bits(base[q][perm]), "%s M %d: %s" % (path, M, q)
            s = base[q]
            if q[:2] in ("ei", "cb") and (s == s.max()).sum() == 1:
                assert perm[o[q + "_idx"] - 1] == base[q + "_idx"] - 1, (path, M, q)
