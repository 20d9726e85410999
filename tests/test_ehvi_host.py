"""Two-objective nomination, host side (no GPU): the float64 restatement of the marginal EHVI against 50 digits, the closed form
against a Monte-Carlo mean of brute-force hypervolume improvements, the factorised marginal against the explicit double loop, the
two host-only exports through the C ABI, the declarations of the new entry points (header, Lua cdef, Python SYMBOLS), the score
class, and the bot's bookkeeping on a stand-in context."""
import os
import re
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib

import _ehvi_ref as R
import _exact as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_eval_posterior", "b7_posterior_get", "b7_pareto_front2", "b7_hypervolume2", "b7_ehvi_compute", "b7_ehvi_nominate")
NAN = np.nan


def test_restatement_against_50_digits():
    """ehvi_numpy against ehvi_mp on the kernel tests' case set (rows thinned to keep the 50-digit side short): row classes
    exactly; values within 1e-6 of the row's scale Psi1(r1) Psi2(r2) -- the positive-term form loses about z^4 eps / 2 of a Psi's
    own value where z = (a - mu) / sigma is far below -1 (the rounding of z^2 / 2 inside exp, times the 1 / z^2 that the
    subtraction leaves), 3e-10 at z = -37.5 in each objective, beyond which Psi is 0 -- and within 64 eps of it on the rows where no
    Psi has z below -4; the smallest normal double is added to either bar, for the rows whose scale is none.  Prints the worst figures."""
    worst_all, worst_mild = 0.0, 0.0
    for M, P, S1, S2 in R.KERNEL_CASES:
        mu1, var1, mu2, var2 = R.make_rows(M, S1, S2)
        keep = np.arange(M)[:: max(1, M // 24)]
        mu1, var1, mu2, var2 = mu1[:, keep], var1[:, keep], mu2[:, keep], var2[:, keep]
        front = R.make_front(P)
        got = R.ehvi_numpy(mu1, var1, mu2, var2, front, R.REF)
        hi, lo = R.ehvi_mp(mu1, var1, mu2, var2, front, R.REF)
        assert np.array_equal(np.isnan(got), np.isnan(hi))
        ok = ~np.isnan(hi)
        assert ok.sum() >= len(keep) - 3 and (got[ok] >= 0.0).all() and np.isfinite(got[ok]).all()
        scale = R.empty_scale_mp(mu1, var1, mu2, var2, R.REF)
        assert (hi[ok] <= scale[ok] * (1 + 1e-15)).all()            # the empty-front EHVI bounds every EHVI of the row
        err, sc = R.err_vs_mp(got, hi, lo)[ok], scale[ok]
        with np.errstate(all="ignore"):
            zmin = np.minimum(((R.REF[0] - 1.0 - mu1) / np.sqrt(var1)).min(axis=0), ((R.REF[1] - 1.0 - mu2) / np.sqrt(var2)).min(axis=0))[ok]
        mild = zmin > -4.0                                           # even the lowest strip edge (>= ref - extent) is no deep tail
        assert (err <= 1e-6 * sc + E.TINY).all() and (err[mild] <= 64 * E.EPS * sc[mild] + E.TINY).all()
        big = sc >= 1e-290                                           # (make_rows leaves no scale between 0 and this)
        worst_all = max(worst_all, (err[big] / sc[big]).max() if big.any() else 0.0)
        worst_mild = max(worst_mild, (err[big & mild] / sc[big & mild]).max() if (big & mild).any() else 0.0)
    print("ehvi_numpy against 50 digits: worst error %.3g of the row's scale; %.3g eps on rows without a deep tail" % (worst_all, worst_mild / E.EPS))


def test_row_classes_of_the_restatement():
    front, ref = np.array([[0.2, 0.8], [0.5, 0.3]]), np.array([1.0, 1.0])
    # var == 0 everywhere: Psi(a) = max(a - mu, 0) and the EHVI is the improvement of the point (mu1, mu2) itself
    pts = np.array([[0.1, 0.1], [0.3, 0.5], [0.6, 0.9], [0.2, 0.8], [2.0, 0.0]])
    got = R.ehvi_numpy(pts[None, :, 0], np.zeros((1, 5)), pts[None, :, 1], np.zeros((1, 5)), front, ref)
    want = R.hv_improvement(front, ref, pts)
    assert np.allclose(got, want, rtol=0, atol=4 * E.EPS) and got[3] == 0.0 and got[4] == 0.0 and got[0] > 0.0
    # P = 0: Psi1(r1) Psi2(r2)
    got0 = R.ehvi_numpy(pts[None, :, 0], np.zeros((1, 5)), pts[None, :, 1], np.zeros((1, 5)), np.zeros((0, 2)), ref)
    assert np.array_equal(got0, np.maximum(1.0 - pts[:, 0], 0.0) * np.maximum(1.0 - pts[:, 1], 0.0))
    # NaN classes; a division that overflows (sigma tiny) stays finite
    mu1 = np.array([[0.3, NAN, 0.3, 0.3, 0.3, -1e300]])
    var1 = np.array([[0.1, 0.1, NAN, -1.0, 0.1, 1e-320]])
    mu2, var2 = np.full((1, 6), 0.4), np.array([[0.1, 0.1, 0.1, 0.1, -0.0, 0.1]])
    got = R.ehvi_numpy(mu1, var1, mu2, var2, front, ref)
    assert list(np.isnan(got)) == [False, True, True, True, False, False] and np.isfinite(got[[0, 4, 5]]).all() and (got[[0, 4, 5]] >= 0).all()


def test_closed_form_against_monte_carlo():
    """ehvi_mp against the seeded Monte-Carlo mean of the brute-force hypervolume improvement, 2e5 draws, within 4 standard errors
    of that mean: this checks the formula, not the library."""
    rng = np.random.default_rng(20160229)
    cases = [(np.array([[0.2, 0.8], [0.5, 0.3]]), np.array([1.0, 1.0]), (0.4, 0.3), (0.5, 0.2)),
             (R.make_front(5), R.REF, (0.6, 0.5), (0.2, 0.6)),
             (np.zeros((0, 2)), np.array([1.0, 2.0]), (0.8, 0.4), (1.5, 1.0)),
             (R.make_front(9, seed=3), R.REF, (1.3, 0.7), (-0.2, 0.4))]
    for front, ref, (m1, s1), (m2, s2) in cases:
        y = np.stack([m1 + s1 * rng.standard_normal(200000), m2 + s2 * rng.standard_normal(200000)], axis=1)
        hvi = R.hv_improvement(front, ref, y)
        assert (hvi >= -1e-12).all()
        mean, se = hvi.mean(), hvi.std(ddof=1) / np.sqrt(len(hvi))
        want = float(R.ehvi_mp_values([[m1]], [[s1 * s1]], [[m2]], [[s2 * s2]], front, ref)[0])
        print("P = %d: closed form %.6g, Monte Carlo %.6g +- %.2g (%.2f standard errors)" % (len(front), want, mean, se, abs(mean - want) / se))
        assert abs(mean - want) <= 4.0 * se


def test_factorised_marginal_equals_the_double_loop():
    mu1, var1, mu2, var2 = R.make_rows(24, 4, 3, seed=5)
    for P in (0, 1, 7):
        front = R.make_front(P, seed=1)
        fact = R.ehvi_mp_values(mu1, var1, mu2, var2, front, R.REF)
        for j in range(6, 24, 3):
            dbl = R.ehvi_mp_double(mu1[:, j], var1[:, j], mu2[:, j], var2[:, j], front, R.REF)
            with mpmath.workdps(50):
                assert abs(fact[j] - dbl) <= mpmath.mpf("1e-40") * abs(dbl), (P, j)


def _front_through_the_abi(Y, ref):
    front, rows = _lib.pareto_front2(Y, ref)
    wf, wr = R.canonical_front(Y, ref)
    assert front.shape == wf.shape and front.tobytes() == wf.tobytes() and list(rows) == list(wr)
    assert R.is_canonical(front, ref)
    assert _lib.hypervolume2(front, ref) == R.hypervolume(front, ref)
    return front, rows


def test_pareto_front_and_hypervolume_through_the_c_abi():
    ref = np.array([1.0, 2.0])
    front, rows = _front_through_the_abi(np.zeros((0, 2)), ref)                       # n = 0
    assert front.shape == (0, 2) and _lib.hypervolume2(front, ref) == 0.0
    front, rows = _front_through_the_abi([[0.25, 0.5]], ref)                           # one row
    assert list(rows) == [1] and _lib.hypervolume2(front, ref) == 0.75 * 1.5
    front, rows = _front_through_the_abi([[0.5, 1.5], [0.1, 0.2], [0.1, 0.3], [0.9, 0.2]], ref)   # all dominated by row 2
    assert list(rows) == [2]
    front, rows = _front_through_the_abi([[0.4, 0.4], [0.2, 0.9], [0.4, 0.4], [0.2, 0.9]], ref)   # duplicates: the lowest row stays
    assert list(rows) == [2, 1]
    front, rows = _front_through_the_abi([[NAN, 0.1], [0.3, NAN], [0.5, 0.5], [-np.inf, 0.1], [0.1, np.inf]], ref)   # NaN / inf rows
    assert list(rows) == [3]
    # on and outside the walls: a_k < r1 and b_k < r2, strictly
    front, rows = _front_through_the_abi([[1.0, 0.1], [0.1, 2.0], [np.nextafter(1.0, 0), 0.2], [0.2, np.nextafter(2.0, 0)], [1.5, 0.0], [0.0, 2.5]], ref)
    assert list(rows) == [4, 3]
    rng = np.random.default_rng(8)
    Y = np.round(rng.random((300, 2)) * 40) / 40 * np.array([1.2, 2.4])               # 300 rows on a lattice: ties in either objective
    front, rows = _front_through_the_abi(Y, ref)
    assert 3 <= len(front) <= 40
    assert abs(_lib.hypervolume2(front, ref) - R.dominated_area(Y[None], ref)[0]) <= 64 * E.EPS * ref.prod()
    # every observed row inside the box is dominated by, or is, a front point; no front point dominates another
    for y in Y:
        if y[0] < ref[0] and y[1] < ref[1]:
            assert ((front[:, 0] <= y[0]) & (front[:, 1] <= y[1])).any()
    # P beyond the cap
    k = np.arange(_lib.EHVI_PMAX + 1, dtype=np.float64)
    big = np.stack([k / 1000.0, 1.0 - k / 1000.0], axis=1)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        _lib.pareto_front2(big, ref)
    assert e.value.code == -1 and str(_lib.EHVI_PMAX + 1) in str(e.value)
    assert len(_lib.pareto_front2(big[:-1], ref)[0]) == _lib.EHVI_PMAX
    with pytest.raises(bot7_amd.Bot7HipError):
        _lib.pareto_front2(big[:3], [np.inf, 1.0])
    # b7_hypervolume2 refuses what is not canonical
    for bad in ([[0.5, 0.5], [0.2, 0.9]], [[0.2, 0.5], [0.5, 0.5]], [[0.2, 0.5], [0.2, 0.4]], [[0.2, 2.0]], [[NAN, 0.1]]):
        with pytest.raises(bot7_amd.Bot7HipError) as e:
            _lib.hypervolume2(bad, ref)
        assert e.value.code == -1 and "canonical" in str(e.value)


def test_header_cdef_and_symbols_agree_on_the_new_entries():
    decls = {re.search(r"\b(b7_[a-z0-9_]+)\s*\(", d).group(1): d for d in gen_lua_cdef.cdef_lines(HEADER)
             if re.match(r"^(?!typedef).*\bb7_[a-z0-9_]+\s*\(", d)}
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    block = lua.split(gen_lua_cdef.BEGIN_CDEF)[1].split(gen_lua_cdef.END_CDEF)[0].splitlines()
    L = _lib.load()
    for name in NEW:
        assert name in decls, "include/bot7hip.h does not declare %s" % name
        assert decls[name] in block, "lua/bot7hip_ffi.lua does not carry the header's %s" % name
        assert name in _lib.SYMBOLS and len(getattr(L, name).argtypes) == decls[name].count(",") + 1
        i = HEADER.index(name + "(b7_ctx" if name not in ("b7_pareto_front2", "b7_hypervolume2") else name + "(const")
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "no counterpart in the reference" in comment.lower(), name
    defs = gen_lua_cdef.defines(HEADER)
    assert defs["B7_ABI_VERSION"] == 1                      # additive: the version stays
    assert (defs["B7_EHVI_PMAX"], defs["B7_EHVI_SMAX"], defs["B7_EHVI_SREG"]) == (_lib.EHVI_PMAX, _lib.EHVI_SMAX, _lib.EHVI_SREG) == (R.PMAX, R.SMAX, R.SREG)
    i = HEADER.index("#define B7_EHVI_PMAX")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    for word in ("Emmerich", "more than two objectives", "correlated objectives", "log-space EHVI", "batches", "refinement", "constraints",
                 "sharded grids and groups", "Bayesian-linear head", "ParEGO"):
        assert word in comment, word


def test_score_class_registry_and_refusals():
    from bot7_amd import scores
    cls = scores.registry["expected_hypervolume_improvement"]
    assert cls is scores.expected_hypervolume_improvement and cls().title == "bot7.scores.expected_hypervolume_improvement"
    s = cls({"type": "expected_hypervolume_improvement"})
    with pytest.raises(NotImplementedError) as e:
        s.compute(np.zeros(3), np.ones(3))
    assert "two objectives" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        s.add_to(object())
    assert "ehvi_nominate" in str(e.value)

    class Rec(object):
        def ehvi_nominate(self, other, front, ref):
            self.got = (other, np.asarray(front).shape, list(ref))
            return 0.5, 7
    r, o = Rec(), Rec()
    assert s.nominate(r, o, np.zeros((2, 2)), [1.0, 2.0]) == (0.5, 7) and r.got == (o, (2, 2), [1.0, 2.0])
    for meth in ("eval_posterior", "posterior_get", "ehvi_compute", "ehvi_nominate"):
        assert callable(getattr(bot7_amd.Context, meth)), meth
    assert callable(_lib.pareto_front2) and callable(_lib.hypervolume2)


# ---- the bot's bookkeeping on a stand-in context ------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401  (the package re-exports the class under the module's name)
    return sys.modules["harness.bots.bayesopt"]


def _stand_in():
    """oracle.hostctx.OracleContext (the device's stand-in of the CPU tests) with the three calls of a two-objective trial on top:
    the kept posterior from the oracle's GP, the nomination from the float64 restatement."""
    from oracle.hostctx import OracleContext

    class StandIn(OracleContext):
        def __init__(self, name):
            super().__init__()
            self.name, self.device_id, self.post, self.log = name, 0, None, []

        def gp_set_data(self, X_obs, Y):
            self.post = None
            super().gp_set_data(X_obs, Y)

        def grid_upload(self, X):
            self.post = None
            self.log.append(("grid_upload", np.asarray(X).shape[0]))
            super().grid_upload(X)

        def grid_remove(self, idx1):
            self.post = None
            self.log.append(("grid_remove", idx1))
            return super().grid_remove(idx1)

        def eval_posterior(self, hyps):
            mus, vs = [], []
            for h in hyps:
                self.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
                mus.append(np.ravel(self.mu).copy())
                vs.append(np.maximum(np.ravel(self.var), 0.0))
            self.post = (np.stack(mus), np.stack(vs))
            self.log.append(("eval_posterior", len(hyps), self.X.shape[0], np.asarray(self.Y).copy()))

        def ehvi_nominate(self, other, front, ref):
            assert self.post is not None and other.post is not None and self.post[0].shape[1] == other.post[0].shape[1]
            self.acc = R.ehvi_numpy(self.post[0], self.post[1], other.post[0], other.post[1], front, ref)
            i = R.nominee_ref(self.acc)
            self.log.append(("ehvi_nominate", other.name, np.asarray(front).copy(), np.asarray(ref).copy()))
            return float(self.acc[i]), i + 1

    return StandIn


class _Model(object):
    def __init__(self, ctx):
        self.ctx, self.n, self.inits, self.seen = ctx, 0, [], []

    def class_(self):
        return "bot7.models.gp_regressor"

    def init(self, X, Y):
        self.inits.append(np.asarray(Y).copy())

    def sample_hypers(self, X, Y, *a):
        Y = np.asarray(Y)
        assert Y.shape == (len(X), 1)
        self.seen.append(Y.copy())
        self.n += 1
        amp = float(np.var(Y)) or 1.0
        return np.array([0.3 + 0.01 * self.n, 0.3, amp, 1e-4 * amp, float(np.mean(Y))])

    def parse_hypers(self, v):
        return {"lenscale_sq": np.asarray(v[:2]), "amp": float(v[2]), "noise": float(v[3]), "mean": float(v[4])}

    def stage(self, X, Y, grid):
        self.ctx.gp_set_data(X, np.asarray(Y).reshape(len(X), -1))
        if self.ctx.X is None or not np.array_equal(self.ctx.X, np.asarray(grid)):
            self.ctx.grid_upload(np.asarray(grid))


def _ocfg(ref=None, **bot):
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "objectives": {"ref": ref, "model": {"sample": True}}}, **bot),
            "grid": {"dims": 2}, "score": {"type": "expected_hypervolume_improvement"}}


def test_bot_bookkeeping_on_a_stand_in_context():
    from bot7_amd.grids.abstract import DeviceGrid
    from harness import benchmarks as B
    Bz, StandIn = _bot_module(), _stand_in()
    # the column split and the default reference point
    resp = np.array([[1.0, 4.0], [3.0, 2.0], [2.0, NAN], [2.0, 3.0]])
    Y1, Y2 = Bz.split_objectives(resp)
    assert Y1.shape == Y2.shape == (4, 1) and list(Y1[:, 0]) == [1.0, 3.0, 2.0, 2.0] and list(Y2[[0, 1, 3], 0]) == [4.0, 2.0, 3.0]
    assert Y1.flags["C_CONTIGUOUS"] and Y2.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        Bz.split_objectives(np.zeros((3, 3)))
    assert list(Bz.default_ref(resp)) == [3.0 + 0.1 * 2.0, 4.0 + 0.1 * 2.0]          # maximum + 10 % of the range; the NaN row sits out
    assert list(Bz.default_ref(np.array([[0.5, -3.0]]))) == [0.5 + 0.1, -3.0 + 0.3]   # no range: 10 % of max(|maximum|, 1)
    # the loop: 3 random + 3 model-based trials on two_spheres
    host = np.random.default_rng(3).random((40, 2))
    c1, c2 = StandIn("one"), StandIn("two")
    c1.grid_upload(host)
    m1, m2 = _Model(c1), _Model(c2)
    bot = Bz.bayesopt(B.two_spheres, [], _ocfg(), {"model": m1, "candidates": DeviceGrid(host, c1, c1.grid_version)})
    assert bot.config["bot"]["objectives"] == {"ref": None, "model": dict(Bz.bayesopt._model_defaults({"sample": True}, 2))}
    bot.objective2 = {"ctx": c2, "grid": None, "model": m2}
    for t in range(6):
        x, y = bot.run_trial()
        bot.update_best(x, y)
        bot.progress_report(t + 1, x, y)
        assert np.asarray(y).shape == (1, 2) and np.array_equal(y, B.two_spheres(x))
        if t < 3:
            assert not [e for e in c1.log + c2.log if e[0] in ("eval_posterior", "ehvi_nominate")]      # the initial trials touch no model
            continue
        last = bot.last_objectives
        n = t                                                                          # observations this nomination saw
        e1, e2 = [e for e in c1.log if e[0] == "eval_posterior"][-1], [e for e in c2.log if e[0] == "eval_posterior"][-1]
        assert e1[1:3] == (2, 40 - n) and e2[1:3] == (2, 40 - n)                        # both contexts, the same grid rows, nSamples each
        assert np.array_equal(e1[3][:, 0], bot.responses[:n, 0]) and np.array_equal(e2[3][:, 0], bot.responses[:n, 1])   # column 0 / column 1
        nom = [e for e in c1.log if e[0] == "ehvi_nominate"][-1]
        assert nom[1] == "two" and np.array_equal(nom[3], Bz.default_ref(bot.responses[:n])) and np.array_equal(nom[3], last["ref"])
        wf, wr = R.canonical_front(bot.responses[:n], last["ref"])
        assert np.array_equal(nom[2], wf) and list(last["rows"]) == list(wr)
        assert np.array_equal(c1.X, c2.X) and np.array_equal(c1.X, np.asarray(bot.candidates)) and c1.X.shape == (40 - n - 1, 2)
        assert c1.log[-1] == c2.log[-1] == ("grid_remove", last["index"])              # the stolen row leaves both grids
    assert m1.inits[0].shape == (3, 1) and np.array_equal(m1.inits[0][:, 0], bot.responses[:3, 0])
    assert np.array_equal(m2.inits[0][:, 0], bot.responses[:3, 1])
    assert m1.n == m2.n == 3 * 3                                                       # per trial the burn-in call and nSamples draws, each model
    assert [e[1] for e in c2.log if e[0] == "grid_upload"] == [37]                     # the second context's grid: uploaded once, then followed
    # under the nadir heuristic the box holds every observation but those on its walls' side: the maxima themselves stay inside
    assert bot.best["hv"] == _lib.hypervolume2(bot.best["front"], bot.best["ref"]) > 0.0 and len(bot.best["front"]) >= 1
    # P = 0 on the first model-based trial: a fixed reference point below every observation
    c1, c2 = StandIn("one"), StandIn("two")
    c1.grid_upload(host)
    bot = Bz.bayesopt(B.two_spheres, [], _ocfg(ref=[-1.0, -1.0]), {"model": _Model(c1), "candidates": DeviceGrid(host, c1, c1.grid_version)})
    bot.objective2 = {"ctx": c2, "grid": None, "model": _Model(c2)}
    for t in range(4):
        x, y = bot.run_trial()
        bot.update_best(x, y)
    assert bot.last_objectives["front"].shape == (0, 2) and [e for e in c1.log if e[0] == "ehvi_nominate"][-1][2].shape == (0, 2)
    assert bot.best["hv"] == 0.0 and list(bot.best["ref"]) == [-1.0, -1.0]
    assert bot.last_objectives["value"] == 0.0 or bot.last_objectives["value"] > 0.0    # Psi1(r1) Psi2(r2): finite, never NaN


def test_bot_refusals_by_name():
    Bz = _bot_module()
    base = Bz.bayesopt(None, [], _ocfg(), {"model": object(), "candidates": np.zeros((4, 2))}).config
    assert Bz.objectives_refusal(base) is None
    plain = Bz.bayesopt(None, [], {"bot": {"verbose": 0}, "grid": {"dims": 2}}, {"model": object(), "candidates": np.zeros((4, 2))}).config
    assert plain["bot"]["objectives"] is None and Bz.objectives_refusal(plain) is None    # the default: the reference's loop
    con = [{"threshold": 0.5, "model": {}}]
    cases = [(dict(base, bot=dict(base["bot"], batch=2)), {}, "batch"),
             (dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "refine"),
             (dict(base, bot=dict(base["bot"], constraints=con)), {}, "constraints"),
             (base, {"sharded": True}, "sharded"),
             (base, {"model_class": "bot7.models.dngo"}, "dngo"),
             (dict(base, score={"type": "expected_improvement"}), {}, "expected_improvement"),
             (dict(base, score={"type": "knowledge_gradient"}), {}, "knowledge_gradient"),
             (dict(base, bot=dict(base["bot"], objectives=None)), {}, "without config.bot.objectives")]
    for cfg, kw, word in cases:
        why = Bz.objectives_refusal(cfg, **kw)
        assert why and word in why and "config.bot.objectives" in why, (word, why)

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    for cfg, kw, word in cases[:3] + cases[5:6] + cases[7:]:
        bot = Bz.bayesopt(None, [], cfg, {"model": M(), "candidates": np.zeros((4, 2))})
        with pytest.raises(NotImplementedError) as e:
            bot.run_trial()
        assert word in str(e.value)
        assert bot.nTrials == 0                                  # refused before anything moved


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new ones: their calls name declared functions with the declared
    number of arguments, the score class exists, and nominate_objectives makes the Python mirror's calls in the mirror's order."""
    import test_lua_shims as L
    sc = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "scores_hip.lua")).read())
    assert "torch.class('bot7.scores.expected_hypervolume_improvement_hip', 'bot7.scores.abstract')" in sc
    assert "S.expected_hypervolume_improvement = EHVI" in sc
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos, called = L.prototypes(), dict(L.calls(bt))
    for name in ("b7_eval_posterior", "b7_pareto_front2", "b7_ehvi_nominate"):
        assert called[name] == protos[name], name
    i = bt.index("function bot:nominate_objectives(")
    body = bt[i:bt.index("\nend", i)]
    order = [body.index(w) for w in ("b7_pareto_front2(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P)",
                                     "b7_eval_posterior(hip.ctx, S, hyps, jit, info)", "follow_steal(o2, self.objectives_idx, candidates)",
                                     "b7_eval_posterior(hip.ctx, S, hyps2, nil, nil)", "b7_ehvi_nominate(hip.ctx, o2.ctx, front, P[0], hip.data(ref), v, i)")]
    assert order == sorted(order)
    assert "self.nTrials <= self.config.bot.nInitial" in body and "R:narrow(2, 1, 1)" in body and "R:narrow(2, 2, 1)" in body
    assert "kernel = hip.KERNEL_ARDSE}" in body and "b7_create(ctxp, hip.device)" in body and "self.objectives_idx = tonumber(i[0])" in body
    for word in ("batch", "refine", "constraints", "group", "gp_hip"):          # the refusals, by name
        assert word in body, word
    assert "if self.config.bot.objectives then return self:nominate_objectives(candidates) end" in bt
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
