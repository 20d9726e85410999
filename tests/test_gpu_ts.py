"""b7_ts_nominate / b7_rff_compute on the GPU: Thompson sampling from pathwise posterior samples.

The feature kernel is measured against 50 digits with plain numpy float64 as the yardstick; the draws against the numpy
restatement of the counter generator; the paths against tests/_ts_ref.paths_ref fed with the device's own draws (so only the
arithmetic differs), at the project's posterior-mean bar, 1e-5 relative to max(1, |ref|); the nominees against the rule
"path j's first minimum over the rows no earlier path took", with a tolerance of twice that bar so that no near-tie needs an
exclusion.  Every test prints its achieved figure; the docstrings carry the MI355X figures."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _ts_ref as R
from conftest import make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-5   # the posterior-mean bar


def _objective(X):
    return np.sin(3.0 * X.sum(axis=1, keepdims=True)) + X[:, -1:] ** 2


def hyper_samples(hyp, S):
    return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.3 * s), amp=hyp["amp"] * (1.0 + 0.2 * s), mean=hyp["mean"] + 0.05 * s)
            for s in range(S)]


def stage(c, X, y, Xc, kernel="ardse"):
    c.gp_set_kernel(kernel)
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def device_draws(c, q):
    return [c.ts_last_draws(j) for j in range(q)]


def scaled_err(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def check_nominees(ref, idx1, tol_scale=2.0 * BAR):
    """Every returned row r_j: ref_j[r_j] <= min over the rows not taken earlier + 2 bar max(1, |that minimum|); rows distinct."""
    taken, worst = [], 0.0
    for j, i1 in enumerate(idx1):
        r = int(i1) - 1
        assert 0 <= r < len(ref) and r not in taken
        col = ref[:, j].copy()
        col[taken] = np.inf
        best = col.min()
        worst = max(worst, float(ref[r, j] - best))
        assert ref[r, j] <= best + tol_scale * max(1.0, abs(best)), (j, r, ref[r, j], best)
        taken.append(r)
    return worst


# ---- 1. the feature kernel against 50 digits ------------------------------------------------------------------------------
def rff_inputs(M1, d, F, q, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3.0, 3.0, (M1, d)), 2.0 * rng.standard_normal((F, d)), rng.uniform(0.0, 2.0 * np.pi, F), rng.standard_normal((F, q))


def rff_check(c, X, om, ph, W, hi, lo, label):
    got = c.rff_compute(X, om, ph, W)
    assert got.shape == hi.shape and np.isfinite(got).all(), "padded rows / features must not make a NaN"
    e_np = R.err_vs_exact(np.cos(X @ om.T + ph) @ W, hi, lo)
    e_dev = R.err_vs_exact(got, hi, lo)
    slack = 1e-15 * float(np.abs(W).sum(axis=0).max())
    print("rff %s: device %.3g, numpy %.3g (ratio %.2f), slack %.3g, max |arg| %.0f" % (label, e_dev, e_np, e_dev / max(e_np, 1e-300), slack,
                                                                                       np.abs(X @ om.T + ph).max()))
    assert e_dev <= 16.0 * e_np + slack


@pytest.mark.parametrize("d", [1, 6, 9, 32, 33, 65, 96])
def test_rff_compute_every_dimension_class(ctx, d):
    """M1 = 65, F = 48, q = 5: every dpad class and its ragged edge.  Bar: 16 x the error of numpy float64 on the same inputs
    against the same 50 digits + 1e-15 sum |W|.  MI355X: device 9.4e-15 (d = 1) ... 2.07e-13 (d = 96, |arg| up to 128), 0.99 - 1.00 of
    numpy's error in every class."""
    X, om, ph, W = rff_inputs(65, d, 48, 5, 100 + d)
    hi, lo = R.rff_exact(X, om, ph, W)
    rff_check(ctx, X, om, ph, W, hi, lo, "d=%d" % d)


@pytest.fixture(scope="module")
def rff_big():
    """One set of inputs for the M1 / F / q sweep, its 50-digit products computed once: rows, features' prefixes and columns are
    prefixes of the same arrays (the F = 16 product is its own evaluation)."""
    X, om, ph, W = rff_inputs(257, 6, 1024, 16, 7)
    return X, om, ph, W, {1024: R.rff_exact(X, om, ph, W), 16: R.rff_exact(X, om[:16], ph[:16], W[:16])}


@pytest.mark.parametrize("q", [1, 16])
@pytest.mark.parametrize("F", [16, 1024])
@pytest.mark.parametrize("M1", [1, 63, 64, 257])
def test_rff_compute_rows_features_paths(ctx, rff_big, M1, F, q):
    """d = 6; M1 in {1, 63, 64, 257} (one ragged tile, a full one, three blocks), F in {16, 1024}, q in {1, 16}.  Same bar.
    MI355X: device 4.9e-16 ... 1.5e-13; device / numpy 0.02 ... 1.47 (worst at M1 = 257, F = 1024, q = 16: 1.52e-13 against 1.04e-13)."""
    X, om, ph, W, exact = rff_big
    hi, lo = exact[F]
    rff_check(ctx, X[:M1], om[:F], ph[:F], W[:F, :q], hi[:M1, :q], lo[:M1, :q], "M1=%d F=%d q=%d" % (M1, F, q))


# ---- 2. the draws ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(orc):
    X, y, Xc, hyp = make_problem(None, orc, 3, 37, 1000, _objective)
    return X, y, Xc, hyp


@pytest.mark.parametrize("kernel", ["ardse", "ardmatern52"])
def test_draws_equal_the_restated_generator(ctx, small, kernel):
    """b7_ts_last_draws against tests/_ts_ref.draws.  The phases (integer steps and one rounding) bit for bit.  Every quantity that
    is ONE chain of the floating steps log -> sqrt -> cos -> product (-> division) -- weight, eps, ARD-SE's omega -- within 4 ulp.
    Matern's omega is a product of two such chains, z and sqrt(5 / u) with u a sum of five squared normals: with each normal within
    4 ulp, u is within 2 x 4 + 3 (its own roundings) = 11 ulp, sqrt(5 / u) within 11 / 2 + 1 = 6.5, and z sqrt(5 / u) / sqrt(ls) within
    4 + 6.5 + 1 -> 12 ulp.  Path j's draws are the same bits in a q = 3 and a q = 5 call, and for S = 1 and S = 3 where the hyper
    sample is the same.  MI355X: worst 3.00 ulp (ARD-SE, all of it), 5.0 ulp (Matern's omega)."""
    X, y, Xc, hyp = small
    hyps, N, F, seed = hyper_samples(hyp, 3), len(X), 256, 12345
    for s in range(3):
        hyps[s]["noise"] = hyp["noise"] * (1.0 + s)
    stage(ctx, X, y, Xc, kernel)
    ctx.ts_nominate(hyps, 5, n_features=F, seed=seed)
    d5 = device_draws(ctx, 5)
    worst = 0.0
    for j, dr in enumerate(d5):
        want = R.draws(seed, j, F, 3, N, hyps[j % 3]["lenscale_sq"], hyps[j % 3]["noise"], kernel)
        assert dr["phase"].tobytes() == want["phase"].tobytes()
        for name in ("omega", "weight", "eps"):
            u = float(R.ulps(dr[name], want[name]).max())
            worst = max(worst, u)
            assert u <= (12.0 if (kernel == "ardmatern52" and name == "omega") else 4.0), (j, name, u)
    print("draws %s: worst %.2f ulp" % (kernel, worst))
    ctx.ts_nominate(hyps, 3, n_features=F, seed=seed)
    for j, dr in enumerate(device_draws(ctx, 3)):
        assert all(dr[k].tobytes() == d5[j][k].tobytes() for k in dr)
    ctx.ts_nominate(hyps[:1], 3, n_features=F, seed=seed)
    for j, dr in enumerate(device_draws(ctx, 3)):
        assert dr["phase"].tobytes() == d5[j]["phase"].tobytes() and dr["weight"].tobytes() == d5[j]["weight"].tobytes()
    d1 = ctx.ts_last_draws(0)
    assert d1["omega"].tobytes() == d5[0]["omega"].tobytes() and d1["eps"].tobytes() == d5[0]["eps"].tobytes()
    ctx.ts_nominate(hyps, 3, n_features=F, seed=seed + 1)
    assert ctx.ts_last_draws(0)["weight"].tobytes() != d5[0]["weight"].tobytes()
    ctx.gp_set_kernel("ardse")


# ---- 3. (and 5.) the paths and the nominees against the reference ------------------------------------------------------------
#        N    M     d   kernel         S  q
CASES = [(5, 7, 3, "ardse", 1, 1), (5, 7, 6, "ardmatern52", 3, 5), (37, 1000, 3, "ardse", 1, 5), (37, 1000, 6, "ardmatern52", 3, 5),
         (128, 1000, 6, "ardse", 3, 16), (129, 4099, 6, "ardmatern52", 1, 16), (129, 1000, 33, "ardmatern52", 1, 1),
         (200, 1000, 33, "ardse", 3, 5), (200, 4099, 3, "ardse", 1, 16), (128, 4099, 3, "ardmatern52", 3, 1)]


@pytest.mark.parametrize("N,M,d,kernel,S,q", CASES)
def test_paths_and_nominees_against_the_reference(ctx, orc, N, M, d, kernel, S, q):
    """b7_ts_last_paths against paths_ref fed with b7_ts_last_draws, make_problem's inputs (noise = 1e-4 amp), F = 256: within
    1e-5 max(1, |ref|); every nominee within twice that of the best row still free, rows distinct, path_min the path's own value.
    MI355X: scaled error 3.5e-15 (N = 5) ... 1.7e-10 (N = 128, d = 6, ARD-SE, S = 3, q = 16), the posterior mean's own range; every
    nominee the reference's best free row itself (slack 0)."""
    X, y, Xc, hyp = make_problem(None, orc, d, N, M, _objective)
    hyps = hyper_samples(hyp, S)
    stage(ctx, X, y, Xc, kernel)
    vals, idx, rep = ctx.ts_nominate(hyps, q, n_features=256, seed=77, want_report=True)
    P = ctx.ts_last_paths()
    ref = R.paths_ref(X, y, Xc, hyps, kernel, device_draws(ctx, q), jitter=rep["jitter"])
    err = scaled_err(P, ref)
    slack = check_nominees(ref, idx)
    print("paths N=%d M=%d d=%d %s S=%d q=%d: scaled error %.3g; nominees within %.3g of the best free row; jitter %s"
          % (N, M, d, kernel, S, q, err, slack, rep["jitter"].tolist()))
    assert P.shape == (M, q) and err <= BAR
    assert all(vals[j].tobytes() == P[idx[j] - 1, j].tobytes() for j in range(q))
    ctx.gp_set_kernel("ardse")


# ---- 4. the identity on the device -----------------------------------------------------------------------------------------
def test_path_identity_on_the_device(ctx, small):
    """paths(X_obs) + eps + noise alpha = y with everything from the device: the paths at the observed rows (the grid IS X_obs), eps
    from b7_ts_last_draws, alpha from a b7_gp_fit of the pseudo-responses y - b7_rff_compute(X, ...) - eps.  Bound: the backward
    error of two stable solves, 64 N 2^-53 ||K||_inf max |alpha|.  MI355X: residual 2.5e-13 ... 5.0e-13 against a bound of 1.2e-9 ... 1.7e-9
    (max |alpha| 234 ... 333)."""
    X, y, _, hyp = small
    N, F, q = len(X), 256, 5
    stage(ctx, X, y, X)
    ctx.ts_nominate([hyp], q, n_features=F, seed=3)
    P, dr = ctx.ts_last_paths(), device_draws(ctx, q)
    W = np.sqrt(2.0 * hyp["amp"] / F) * np.stack([d_["weight"] for d_ in dr], axis=1)
    phiw = ctx.rff_compute(X, dr[0]["omega"], dr[0]["phase"], W)
    for j in range(q):
        ctx.gp_fit(X, (y[:, 0] - phiw[:, j] - dr[j]["eps"]).reshape(-1, 1), hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        alpha = ctx.gp_download(N)[1][:, 0]
        res = float(np.abs(P[:, j] + dr[j]["eps"] + hyp["noise"] * alpha - y[:, 0]).max())
        bound = 64.0 * N * 2.0 ** -53 * (N * hyp["amp"] + hyp["noise"]) * float(np.abs(alpha).max())
        print("identity path %d: residual %.3g (bound %.3g, max |alpha| %.3g)" % (j, res, bound, np.abs(alpha).max()))
        assert res <= bound


# ---- 5. the nominees ----------------------------------------------------------------------------------------------------------
def test_nominees_share_minimisers_and_stay_distinct(ctx, small):
    """Seed 3 (chosen on the CPU reference): paths 0 and 4 share row 49, paths 1 and 2 row 317 as their unconstrained arg-min, so
    the exclusion rule decides two of the five nominees.  Also: path_min bit for bit with the paths, the same call twice the same
    bits, the grid untouched, and q = M = 7 a permutation of all rows."""
    X, y, Xc, hyp = small
    stage(ctx, X, y, Xc)
    before = ctx.grid_download()
    vals, idx = ctx.ts_nominate([hyp], 5, n_features=256, seed=3)
    P = ctx.ts_last_paths()
    ref = R.paths_ref(X, y, Xc, hyp, "ardse", device_draws(ctx, 5))
    free = ref.argmin(axis=0)
    print("unconstrained arg-mins of the reference:", free.tolist(), "nominees:", (idx - 1).tolist())
    assert len(set(free.tolist())) <= 3, "the seed was chosen so that paths share their minimiser"
    check_nominees(ref, idx)
    assert len(set(idx.tolist())) == 5 and (idx - 1).tolist() == R.nominees_ref(P)
    assert all(vals[j].tobytes() == P[idx[j] - 1, j].tobytes() for j in range(5))
    vals2, idx2 = ctx.ts_nominate([hyp], 5, n_features=256, seed=3)
    assert vals2.tobytes() == vals.tobytes() and np.array_equal(idx, idx2) and ctx.ts_last_paths().tobytes() == P.tobytes()
    assert np.array_equal(ctx.grid_download(), before)
    ctx.grid_upload(Xc[:7])
    _, idx7 = ctx.ts_nominate([hyp], 7, n_features=256, seed=3)
    assert sorted(idx7.tolist()) == list(range(1, 8))


# ---- 6. jitter ----------------------------------------------------------------------------------------------------------------
def test_jitter_schedule(ctx, small):
    """Duplicated observation rows with zero noise: the plain factorisation fails, the utils.math.chol schedule takes over, the call
    still nominates; the paths match the reference built with that jitter on K's diagonal (eps keeps the sample's own noise: 0).
    MI355X: info [39, 38], jitter 1.1e-8 for both samples, scaled error 3.7e-9."""
    X, y, Xc, hyp = small
    Xd, yd = np.concatenate([X, X[:7]]), np.concatenate([y, y[:7]])
    hard = [dict(h, noise=0.0) for h in hyper_samples(hyp, 2)]
    stage(ctx, Xd, yd, Xc)
    vals, idx, rep = ctx.ts_nominate(hard, 4, n_features=256, seed=5, want_report=True)
    assert (rep["info"] != 0).all() and (rep["jitter"] > 0).all()
    dr = device_draws(ctx, 4)
    assert all(not d_["eps"].any() for d_ in dr)
    P = ctx.ts_last_paths()
    ref = R.paths_ref(Xd, yd, Xc, hard, "ardse", dr, jitter=rep["jitter"])
    err = scaled_err(P, ref)
    print("jitter %s info %s: scaled error %.3g" % (rep["jitter"].tolist(), rep["info"].tolist(), err))
    assert err <= BAR
    check_nominees(ref, idx)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(small):
    import bot7_amd
    X, y, Xc, hyp = small
    hyps = hyper_samples(hyp, 2)
    sp = {"score": "ei", "fmin": [float(y.min())]}
    c = bot7_amd.Context(0)
    try:
        def refused(code, what, call):
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                call()
            assert e.value.code == code and what in str(e.value), str(e.value)

        refused(-4, "no successful b7_ts_nominate", lambda: c.ts_last_paths())
        refused(-4, "no successful b7_ts_nominate", lambda: c.ts_last_draws(0))
        c.grid_upload(Xc[:9])
        import ctypes as C
        arr, keep = c._pack_hyps(hyps, 3)
        out = np.zeros(2)
        optr = out.ctypes.data_as(C.c_void_p)
        assert c._L.b7_ts_nominate(c._h, 2, arr, 2, 64, 0, optr, optr, None, None) == -4   # (the wrapper asks for the data's d first)
        assert b"no resident data" in c._L.b7_last_error(c._h)
        c2 = bot7_amd.Context(0)
        try:
            c2.gp_set_data(X, y)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                c2.ts_nominate(hyps, 2)
            assert e.value.code == -4 and "no candidate grid" in str(e.value)
        finally:
            c2.close()
        c.gp_set_data(X, y)
        usual = c.eval_nominate(hyps, **sp)
        for q, what in ((0, "q = 0"), (17, "q = 17"), (10, "exceeds the grid's 9 rows")):
            refused(-1, what, lambda: c.ts_nominate(hyps, q))
        for F in (8, 4112, 100):
            refused(-1, "F = %d" % F, lambda: c.ts_nominate(hyps, 2, n_features=F))
        refused(-1, "S = 0", lambda: c.ts_nominate([], 2))
        assert c._L.b7_ts_nominate(c._h, 2, arr, 2, 64, 0, None, optr, None, None) == -1
        assert b"NULL" in c._L.b7_last_error(c._h)
        assert c._L.b7_ts_nominate(c._h, 2, None, 2, 64, 0, optr, optr, None, None) == -1
        assert c.eval_nominate(hyps, **sp) == usual
        c.gp_set_data(X, np.hstack([y, y + 1.0]))
        refused(-5, "2 response columns", lambda: c.ts_nominate(hyps, 2))
        c.gp_set_data(X, y)
        assert c.eval_nominate(hyps, **sp) == usual
        # a successful call leaves the accumulator and later nominations alone, and the fit slot empty
        vals, idx = c.ts_nominate(hyps, 3, n_features=64, seed=1)
        refused(-4, "no GP fit", lambda: c.gp_predict())
        assert c.eval_nominate(hyps, **sp) == usual
        refused(-1, "path 3", lambda: c.ts_last_draws(3))
        g = bot7_amd.Group([0, 0])
        try:
            g.grid_upload(Xc[:9])
            g.gp_set_data(X, y)
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                g.members[0].ts_nominate(hyps, 2)
            assert e.value.code == -4 and "group" in str(e.value)
            assert g.eval_nominate(hyps, **sp) == usual
        finally:
            g.close()
    finally:
        c.close()


def test_world_of_two_is_refused(ctx, small, tmp_path):
    """Two ranks on one GPU over the shared-memory RCCL double (tests/stub): b7_ts_nominate answers B7_ERR_UNSUPPORTED, naming the
    communicator, on both, and the b7_eval_nominate that follows gives the single-context nomination of the union."""
    from test_sharded_loop import _diag_lib, _stub_lib
    env = dict(os.environ, B7_RCCL_LIB=_stub_lib(), BOT7HIP_LIB=_diag_lib(), PYTHONPATH=ROOT)
    ident = ("b7ts_%d" % os.getpid()).encode().hex()
    outs = [str(tmp_path / ("r%d.json" % r)) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_ts_worker.py"), str(r), "2", ident, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    for p in procs:
        try:
            _, e = p.communicate(timeout=180)
        except subprocess.TimeoutExpired:
            for k in procs:
                k.kill()
            raise
        assert p.returncode == 0, e[-3000:]
    X, y, Xc, hyp = small
    hyps = hyper_samples(hyp, 2)
    stage(ctx, X, y, Xc)
    want = ctx.eval_nominate(hyps, score="ei", fmin=[float(y.min())])
    for o in outs:
        res = json.load(open(o))
        assert res["code"] == -5 and "communicator of 2 ranks" in res["message"] and (res["value"], res["index"]) == want


# ---- 8. the trial loop -------------------------------------------------------------------------------------------------------
class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def _bot(ctx, batch, seed=4):
    import bot7_amd
    from harness import benchmarks, bots
    grid = bot7_amd.grids.sobol({"size": 2000, "dims": 6, "mins": np.zeros(6), "maxes": np.ones(6)}, context=ctx)()
    cfg = {"bot": {"verbose": 0, "budget": 12, "nInitial": 5, "nSamples": 3, "seed": seed, "batch": batch},
           "grid": {"type": "sobol", "size": 2000, "dims": 6}, "score": {"type": "thompson_sampling", "nFeatures": 256}}
    model = bot7_amd.models.gp_regressor({}, context=ctx)
    return bots.bayesopt(benchmarks.hartmann6, [_H("x%d" % k) for k in range(6)], cfg, cache={"candidates": grid, "model": model})


@pytest.mark.parametrize("batch", [1, 4])
def test_trial_loop(ctx, batch):
    """harness bayesopt on hartmann6 (2000 Sobol candidates, nInitial 5, budget 12, nSamples 3): runs, is deterministic under a
    fixed bot seed, never nominates a row twice, and every model-based nominee re-derived from ts_last_paths / paths_ref passes
    the nominee check.  No optimisation-quality claim.  MI355X: every nominee the reference's best free row (slack 0)."""
    runs = []
    for rep in range(2):
        bot = _bot(ctx, batch)
        inner, seen, worst = bot._ts_nominate, [], 0.0

        def traced(q, cand, inner=inner, bot=bot, seen=seen):
            X, y, Xc = bot.observed.copy(), bot.responses.copy(), np.asarray(cand).copy()
            captured = {}
            orig = bot.score.nominate
            bot.score.nominate = lambda c, hyps, q_, seed: captured.update(hyps=hyps) or orig(c, hyps, q_, seed)
            idx = inner(q, cand)
            bot.score.nominate = orig
            P = ctx.ts_last_paths()
            ref = R.paths_ref(X, y, Xc, captured["hyps"], "ardse", device_draws(ctx, q))
            assert scaled_err(P, ref) <= BAR
            seen.append(check_nominees(ref, np.asarray(idx)))
            return idx
        bot._ts_nominate = traced
        with pytest.raises(NotImplementedError):
            bot.score.add_to(ctx)
        rows = [bot.run_trial()[0] for _ in range(12)]
        assert len(seen) == 12 - 5
        obs = bot.observed
        assert obs.shape == (12 * batch, 6) and len({r.tobytes() for r in obs}) == len(obs)
        assert np.asarray(bot.candidates).shape == (2000 - 12 * batch, 6)
        assert np.array_equal(ctx.grid_download(), np.asarray(bot.candidates))
        with pytest.raises(NotImplementedError):
            bot.eval(want_scores=True)
        runs.append(np.array(rows))
        print("trial loop batch=%d: nominees within %.3g of the best free row; best response %.4f" % (batch, max(seen), bot.responses.min()))
    assert runs[0].tobytes() == runs[1].tobytes()


# ---- 9. nothing else moved ----------------------------------------------------------------------------------------------------
PARENT_BITS = {"fantasize_sha256": "0c0c5598cb5e3b2346b8680e61e78bdb09d182f5cfbf4b53c1b13dd8da77497d", "ei_value_hex": "0x1.e5808485565e3p-2",
               "ei_index": 49}


def pinned_outputs(c, orc):
    """b7_gp_fantasize (P = 8, 16 draws, seed 2024) and an EI b7_eval_nominate (three hyper samples) at N = 37, d = 3, M = 1000."""
    X, y, Xc, hyp = make_problem(None, orc, 3, 37, 1000, _objective)
    stage(c, X, y, Xc)
    c.gp_fit(X, y, hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
    Yf = c.gp_fantasize(Xc[:8], 16, seed=2024)
    Yf = Yf[0] if isinstance(Yf, tuple) else Yf
    c.gp_set_data(X, y)
    v, i = c.eval_nominate(hyper_samples(hyp, 3), score="ei", fmin=[float(y.min())])
    return {"fantasize_sha256": hashlib.sha256(np.ascontiguousarray(Yf).tobytes()).hexdigest(), "ei_value_hex": float(v).hex(), "ei_index": int(i)}


def test_nothing_else_moved(ctx, orc):
    """The generator moved from extras.hip into counter_rng.h: b7_gp_fantasize's draws and an EI nomination give the bits the parent
    commit gave on an MI355X (recorded from a build of the parent)."""
    got = pinned_outputs(ctx, orc)
    print("pinned outputs:", got)
    assert got == PARENT_BITS
