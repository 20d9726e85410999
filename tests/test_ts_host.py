"""Thompson sampling without a GPU: the references of tests/_ts_ref.py against what they must reproduce -- the random features'
covariance is the kernel's (this pins the Matern recipe), the pathwise sample satisfies its defining identity, the 50-digit feature
product agrees with mpmath's own arithmetic -- and the score's registry entry."""
import mpmath
import numpy as np
import pytest

import bot7_amd.scores as Scores

import _ts_ref as R


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
@pytest.mark.parametrize("d", [3, 6, 32])
@pytest.mark.parametrize("F", [256, 1024])
def test_feature_covariance_is_the_kernel(kernel, d, F):
    """Over 64 random points in [0,1]^d: max |Phi Phi' - K| <= 6 amp / sqrt(F), six Monte-Carlo standard errors (each of the F
    terms 2 amp cos(.) cos(.) has variance <= amp^2).  Seeds 11 (points) and 5 (draws); measured here 1.8 .. 3.8 standard errors."""
    rng = np.random.default_rng(11)
    X = rng.random((64, d))
    ls, amp = rng.uniform(0.5, 1.5, d) * d / 8.0, 1.7
    omega, phase = R.basis(5, F, d, ls, kernel)
    Phi = R.features(X, omega, phase, amp)
    err = np.abs(Phi @ Phi.T - R.cov(X, X, ls, amp, kernel)).max()
    print("%s d=%d F=%d: max |Phi Phi' - K| = %.3g = %.2f standard errors" % (kernel, d, F, err, err / (amp / np.sqrt(F))))
    assert err <= 6.0 * amp / np.sqrt(F)


def problem(N=37, d=3, M=1000, seed=3):
    rng = np.random.default_rng(seed)
    X, Xs = rng.random((N, d)), rng.random((M, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(N)
    amp = float(np.var(y))
    hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(y))}
    return X, y, Xs, hyp


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
def test_path_identity(kernel):
    """f_j(X) + eps_j + noise v_j = y: (K + noise I) v = y - m - Phi w - eps and f(X) = m + Phi w + K v.  To 1e-10 max |y|."""
    X, y, _, hyp = problem()
    dr = [R.draws(9, j, 256, 3, len(X), hyp["lenscale_sq"], hyp["noise"], kernel) for j in range(5)]
    f, vs = R.paths_ref(X, y, X, hyp, kernel, dr, want_v=True)
    for j in range(5):
        res = np.abs(f[:, j] + dr[j]["eps"] + hyp["noise"] * vs[j] - y).max()
        print("%s path %d: identity residual %.3g" % (kernel, j, res))
        assert res <= 1e-10 * np.abs(y).max()


def test_draws_depend_on_seed_and_path_only():
    ls = np.array([0.3, 0.5, 0.7])
    a = R.draws(4, 2, 64, 3, 10, ls, 0.01)
    b = R.draws(4, 2, 128, 3, 25, ls, 0.01)
    assert np.array_equal(a["omega"], b["omega"][:64]) and np.array_equal(a["phase"], b["phase"][:64])
    assert np.array_equal(a["weight"], b["weight"][:64]) and np.array_equal(a["eps"], b["eps"][:10])
    c = R.draws(4, 3, 64, 3, 10, ls, 0.01)
    assert np.array_equal(a["omega"], c["omega"]) and not np.array_equal(a["weight"], c["weight"])
    z = R.counter_normal(R.counter_key(1, 1), np.arange(200000))
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01
    assert R.splitmix64(0) == np.uint64(0) and R.splitmix64(R.G) == np.uint64(0xE220A8397B1DCDAF)   # SplitMix64's first output from state 0


def test_exact_feature_product_against_mpmath():
    rng = np.random.default_rng(2)
    X, om = rng.uniform(-3, 3, (3, 5)), 2.0 * rng.standard_normal((16, 5))
    ph, W = rng.uniform(0, 2 * np.pi, 16), rng.standard_normal((16, 2))
    hi, lo = R.rff_exact(X, om, ph, W)
    with mpmath.workdps(60):
        for i in range(3):
            for p in range(2):
                want = mpmath.mpf(0)
                for f in range(16):
                    arg = sum((mpmath.mpf(float(X[i, k])) * mpmath.mpf(float(om[f, k])) for k in range(5)), mpmath.mpf(float(ph[f])))
                    want += mpmath.mpf(float(W[f, p])) * mpmath.cos(arg)
                assert abs(mpmath.mpf(float(hi[i, p])) + mpmath.mpf(float(lo[i, p])) - want) < mpmath.mpf(10) ** -30
    assert R.err_vs_exact(np.cos(X @ om.T + ph) @ W, hi, lo) < 1e-13


def test_nominee_rule_on_a_reference():
    paths = np.array([[0.0, 0.0, np.nan], [1.0, -1.0, np.nan], [0.0, -1.0, 2.0], [np.nan, 5.0, 1.0]])
    assert R.nominees_ref(paths) == [0, 1, 3]
    assert R.nominees_ref(np.array([[1.0, 1.0], [1.0, 1.0]])) == [0, 1]
    assert R.nominees_ref(np.full((3, 2), np.nan)) == [0, 1]


def test_registry_and_config_defaults():
    assert Scores.registry["thompson_sampling"] is Scores.thompson_sampling
    cls = Scores.thompson_sampling
    assert cls.title == "bot7.scores.thompson_sampling" and cls().config["nFeatures"] == 1024
    assert cls({"nFeatures": 256}).config["nFeatures"] == 256
    assert not hasattr(cls, "device_spec")
    with pytest.raises(NotImplementedError, match="not a per-point score"):
        cls().add_to(None)
