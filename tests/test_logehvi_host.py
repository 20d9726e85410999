"""Log-space EHVI, host side (no GPU): the float64 restatements of both log scores against 50 digits, their row classes and
bit-for-bit identities, the fixtures on which the linear scores are exactly 0, the declarations of the four entry points (header, Lua
cdef, Python SYMBOLS), the score class, the bot's refusals, and a bot trial on a stand-in context whose every linear score is 0."""
import os
import re
import sys

import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib

import _ehvi3_ref as R3
import _ehvi_ref as R2
import _logehvi_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_logehvi_compute", "b7_logehvi_nominate", "b7_logehvi3_compute", "b7_logehvi3_nominate")
LOG_EHVI = "log_expected_hypervolume_improvement"
NAN = np.nan


def _thin(M, n=12):
    """The special rows and a spread of the others: the 50-digit side stays short."""
    return np.unique(np.concatenate([np.arange(min(M, 10)), np.arange(M)[:: max(1, M // n)]]))


@pytest.mark.parametrize("P", [0, 1, 2, 33, 256])
def test_two_objective_restatement_against_50_digits(P):
    """logehvi_numpy against log(ehvi_mp_values) within HOST_BAR of max(1, |ref|), on rows with z down to -1e4 and every special class,
    against fronts whose first two points are one ulp apart.  Measured: 8.5e-16 at the worst."""
    M, S1, S2 = (48, 3, 2) if P <= 33 else (20, 2, 1)
    mu1, var1, mu2, var2 = R.make_rows_log(M, S1, S2, seed=P)
    keep = _thin(M) if P == 256 else np.arange(M)
    mu1, var1, mu2, var2 = mu1[:, keep], var1[:, keep], mu2[:, keep], var2[:, keep]
    front = R2.make_front(P)
    got = R.logehvi_numpy(mu1, var1, mu2, var2, front, R2.REF)
    err = R.scaled_errors(got, R.logehvi_mp(mu1, var1, mu2, var2, front, R2.REF))
    lin = R2.ehvi_numpy(mu1, var1, mu2, var2, front, R2.REF)
    print("logehvi_numpy P=%d: worst scaled error %.3g over %d rows; %d of them have a linear EHVI of exactly 0" % (P, err.max(), len(keep), int((lin == 0.0).sum())))
    assert err.max() <= R.HOST_BAR
    assert (lin == 0.0).sum() >= len(keep) // 4                # the rows this score exists for are in the set


@pytest.mark.parametrize("P", [6, 33, 256])
def test_three_objective_restatement_against_50_digits(P):
    """logehvi3_numpy against log(ehvi3_mp_both[0]) within HOST_BAR; P = 6 brings in the shared coordinates.  Measured: 1.2e-15."""
    M, S = (30, (3, 2, 1)) if P <= 33 else (16, (2, 1, 1))
    mu, var = R.make_rows3_log(M, S, seed=P)
    keep = _thin(M, 4) if P == 256 else np.arange(M)
    mu, var = [m[:, keep] for m in mu], [v[:, keep] for v in var]
    front = R3.make_front3(P)
    got = R.logehvi3_numpy(mu, var, front, R3.REF3)
    err = R.scaled_errors(got, R.logehvi3_mp(mu, var, front, R3.REF3))
    lin = R3.ehvi3_numpy(mu, var, front, R3.REF3)
    print("logehvi3_numpy P=%d: worst scaled error %.3g over %d rows; %d of them have a linear EHVI of exactly 0" % (P, err.max(), len(keep), int((lin == 0.0).sum())))
    assert err.max() <= R.HOST_BAR
    assert (lin == 0.0).sum() >= len(keep) // 4


def test_row_classes_of_the_restatements():
    front, ref = np.array([[0.2, 0.8], [0.5, 0.3]]), np.array([1.0, 1.0])
    # var == 0 everywhere: the log of the improvement of the point itself; a dominated point and one outside the box: -inf
    pts = np.array([[0.1, 0.1], [0.3, 0.5], [0.6, 0.9], [0.2, 0.8], [2.0, 0.0]])
    z = np.zeros((1, 5))
    got = R.logehvi_numpy(pts[None, :, 0], z, pts[None, :, 1], z, front, ref)
    want = R2.hv_improvement(front, ref, pts)
    assert got[3] == -np.inf and got[4] == -np.inf and np.isfinite(got[:2]).all()
    assert np.abs(got[:2] - np.log(want[:2])).max() <= 1e-14
    # NaN exactly where the linear score is NaN; everything else never NaN, never +inf
    mu1 = np.array([[0.3, NAN, 0.3, 0.3, 0.3, -1e300, 1e300]])
    var1 = np.array([[0.1, 0.1, NAN, -1.0, 0.1, 1e-320, 1e-300]])
    mu2, var2 = np.full((1, 7), 0.4), np.array([[0.1, 0.1, 0.1, 0.1, -0.0, 0.1, 0.1]])
    got = R.logehvi_numpy(mu1, var1, mu2, var2, front, ref)
    lin = R2.ehvi_numpy(mu1, var1, mu2, var2, front, ref)
    assert np.array_equal(np.isnan(got), np.isnan(lin)) and list(np.isnan(got)) == [False, True, True, True, False, False, False]
    assert not (got[~np.isnan(got)] == np.inf).any() and got[6] == -np.inf and np.isfinite(got[[0, 4, 5]]).all()
    # three objectives: the same classes
    f3, r3 = R3.make_front3(3), R3.REF3
    mu, var = R.make_rows3_log(16, (2, 1, 2))
    got3, lin3 = R.logehvi3_numpy(mu, var, f3, r3), R3.ehvi3_numpy(mu, var, f3, r3)
    assert np.array_equal(np.isnan(got3), np.isnan(lin3)) and list(np.flatnonzero(np.isnan(got3))) == [3, 4, 5, 8, 9]
    assert not (got3[~np.isnan(got3)] == np.inf).any()
    # the deterministic limit: all var == 0 -> log of the hypervolume improvement, -inf for a dominated point
    p3 = np.array([[0.2, 0.2, 0.2], [0.9, 0.9, 0.9], [0.4, 0.5, 0.3]])
    z3 = np.zeros((1, 3))
    det = R.logehvi3_numpy([p3[None, :, m] for m in range(3)], [z3] * 3, f3, r3)
    hvi = R3.hv_improvement3(f3, r3, p3)
    assert det[1] == -np.inf and hvi[1] == 0.0 and np.abs(det[[0, 2]] - np.log(hvi[[0, 2]])).max() <= 1e-13


def test_identities_of_the_restatements_bit_for_bit():
    """P = 0, S = 1 each: the log score is logei(mu1, var1, r1) + logei(mu2, var2, r2) (logei_np, a variance of -0.0 read as 0), and
    with a third objective (l1 + l2) + l3: a difference against -inf, a log-sum-exp of one term and the subtraction of log 1 change no bit."""
    mu1, var1, mu2, var2 = R.make_rows_log(64, 1, 1, seed=9)
    ok = ~R2._bad(mu1, var1, mu2, var2)
    got = R.logehvi_numpy(mu1, var1, mu2, var2, np.zeros((0, 2)), R2.REF)
    want = R._log_psi_np(R2.REF[0], mu1[0], var1[0]) + R._log_psi_np(R2.REF[1], mu2[0], var2[0])
    assert got[ok].tobytes() == want[ok].tobytes() and np.isnan(got[~ok]).all()
    mu, var = R.make_rows3_log(64, (1, 1, 1), seed=9)
    ok = ~R3._bad3(mu, var)
    got = R.logehvi3_numpy(mu, var, np.zeros((0, 3)), R3.REF3)
    l = [R._log_psi_np(R3.REF3[m], mu[m][0], var[m][0]) for m in range(3)]
    want = (l[0] + l[1]) + l[2]
    assert got[ok].tobytes() == want[ok].tobytes() and np.isnan(got[~ok]).all()
    # ldiff and the log-sum-exp on their own
    u = np.array([-3.0, -1e7, 0.5, -np.inf, 2.0, 2.0])
    l_ = np.array([-np.inf, -np.inf, -np.inf, -np.inf, 2.0, 3.0])
    d = R.ldiff_np(u, l_)
    assert d[:4].tobytes() == u[:4].tobytes() and d[4] == -np.inf and d[5] == -np.inf
    acc = R.Lse(3)
    assert (acc.value() == -np.inf).all()                                   # the empty sum
    acc.add(np.array([-np.inf, -5e7, 1.25]))
    acc.add(np.array([-np.inf, -np.inf, -np.inf]))                          # -inf terms are neutral
    assert acc.value().tobytes() == np.array([-np.inf, -5e7, 1.25]).tobytes()   # a single term comes back exactly


def test_far_fixtures_every_linear_score_is_zero_and_the_log_score_ranks():
    """The fixtures of the GPU tests' "it ranks where the linear score cannot": every linear score exactly 0 (its arg-max is row 1),
    the 50-digit arg-max of the log score another row with a gap of at least 1e-6 |value| to the runner-up, and the restatement
    finds it."""
    mu1, var1, mu2, var2, front, ref = R.far_rows()
    assert (R2.ehvi_numpy(mu1, var1, mu2, var2, front, ref) == 0.0).all()
    best, gap = R.argmax_mp(R.logehvi_mp(mu1, var1, mu2, var2, front, ref))
    got = R.logehvi_numpy(mu1, var1, mu2, var2, front, ref)
    print("far rows, two objectives: 50-digit arg-max row %d, gap %.3g, value %.6g" % (best + 1, gap, got[best]))
    assert best != 0 and gap >= 1e-6 and R2.nominee_ref(got) == best
    mu, var, front, ref = R.far_rows3()
    assert (R3.ehvi3_numpy(mu, var, front, ref) == 0.0).all()
    best, gap = R.argmax_mp(R.logehvi3_mp(mu, var, front, ref))
    got = R.logehvi3_numpy(mu, var, front, ref)
    print("far rows, three objectives: 50-digit arg-max row %d, gap %.3g, value %.6g" % (best + 1, gap, got[best]))
    assert best != 0 and gap >= 1e-6 and R3.nominee_ref(got) == best


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
        twin = name.replace("b7_log", "b7_")
        assert decls[name].replace(name, twin) == decls[twin], name          # the linear twin's signature
        i = HEADER.index(name + "(")
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "no counterpart in the reference" in comment.lower(), name
    assert gen_lua_cdef.defines(HEADER)["B7_ABI_VERSION"] == 1                # additive: the version stays
    for define, where in (("#define B7_EHVI_PMAX", "b7_logehvi_"), ("#define B7_EHVI3_PMAX", "b7_logehvi3_")):
        i = HEADER.index(define)
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "log-space EHVI" in comment and where in comment              # the not-built lists say where it now lives
    for src in ("ehvi.hip", "ehvi3.hip", "ehvi_math.h"):
        assert "a\n// log-space EHVI," not in open(os.path.join(ROOT, "bot7_amd", "csrc", src)).read()


def test_score_class_registry():
    from bot7_amd import scores
    cls = scores.registry[LOG_EHVI]
    assert cls is scores.log_expected_hypervolume_improvement and cls().title == "bot7.scores." + LOG_EHVI
    s = cls({"type": LOG_EHVI})
    with pytest.raises(NotImplementedError) as e:
        s.compute(np.zeros(3), np.ones(3))
    assert "logehvi_compute" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        s.add_to(object())
    assert "logehvi_nominate" in str(e.value)

    class Rec(object):
        def logehvi_nominate(self, other, front, ref):
            self.got = ("two", other, np.asarray(front).shape, list(ref))
            return -80.5, 7

        def logehvi3_nominate(self, other2, other3, front, ref):
            self.got = ("three", other2, other3, np.asarray(front).shape, list(ref))
            return -90.25, 9
    r, o2, o3 = Rec(), Rec(), Rec()
    assert s.nominate(r, o2, np.zeros((2, 2)), [1.0, 2.0]) == (-80.5, 7) and r.got == ("two", o2, (2, 2), [1.0, 2.0])
    assert s.nominate(r, (o2, o3), np.zeros((2, 3)), [1.0, 2.0, 3.0]) == (-90.25, 9) and r.got == ("three", o2, o3, (2, 3), [1.0, 2.0, 3.0])
    with pytest.raises(NotImplementedError) as e:
        s.nominate(r, (o2, o3, o3), np.zeros((2, 4)), [1.0, 2.0, 3.0, 4.0])
    assert "4 objectives" in str(e.value)
    for meth in ("logehvi_compute", "logehvi_nominate", "logehvi3_compute", "logehvi3_nominate"):
        assert callable(getattr(bot7_amd.Context, meth)), meth


# ---- the bot ------------------------------------------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401
    return sys.modules["harness.bots.bayesopt"]


def _ocfg(kind, ref=None, three=False, **bot):
    obj = {"ref": ref, "models": [{"sample": True}, {"sample": True}]} if three else {"ref": ref, "model": {"sample": True}}
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "objectives": obj}, **bot), "grid": {"dims": 2}, "score": {"type": kind}}


def test_bot_refusals_by_name():
    """Everything refused with the linear type is refused with the log type, in the same words; the log type is accepted where
    EHVI is, for {"ref", "model"} and {"ref", "models"}; without config.bot.objectives it is refused as EHVI is."""
    Bz = _bot_module()
    con = [{"threshold": 0.5, "model": {}}]
    for three in (False, True):
        mk = lambda kind: Bz.bayesopt(None, [], _ocfg(kind, three=three), {"model": object(), "candidates": np.zeros((4, 2))}).config
        base, lin = mk(LOG_EHVI), mk(Bz.EHVI)
        assert Bz.objectives_refusal(base) is None and Bz.objectives_refusal(lin) is None
        cases = [(dict(bot=dict(batch=2)), {}, "batch"), (dict(bot=dict(refine={"starts": 2})), {}, "refine"),
                 (dict(bot=dict(constraints=con)), {}, "constraints"), ({}, {"sharded": True}, "sharded"),
                 ({}, {"model_class": "bot7.models.dngo"}, "dngo")]
        if three:
            cases.append((dict(bot=dict(trust_region={"length_init": 0.5})), {}, "trust_region"))
        for over, kw, word in cases:
            cfgs = [dict(c, bot=dict(c["bot"], **over.get("bot", {}))) for c in (base, lin)]
            why, why_lin = Bz.objectives_refusal(cfgs[0], **kw), Bz.objectives_refusal(cfgs[1], **kw)
            assert why and word in why and why == why_lin, (word, why, why_lin)
        why = Bz.objectives_refusal(dict(base, score={"type": "expected_improvement"}))
        assert why and "expected_improvement" in why and "config.bot.objectives" in why
    none = dict(base, bot=dict(base["bot"], objectives=None))
    why = Bz.objectives_refusal(none)
    assert why and "without config.bot.objectives" in why and why.startswith(LOG_EHVI)
    assert "trust_region" in Bz.trust_region_refusal(dict(none, bot=dict(none["bot"], trust_region={"length_init": 0.5})))

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"
    bot = Bz.bayesopt(None, [], none, {"model": M(), "candidates": np.zeros((4, 2))})
    with pytest.raises(NotImplementedError) as e:
        bot.run_trial()
    assert "without config.bot.objectives" in str(e.value) and bot.nTrials == 0


def test_bot_trial_where_every_linear_score_is_zero():
    """A stand-in context (test_ehvi_host's, with the log nomination from the float64 restatement) and a reference point far below
    every observation: P = 0 and every posterior is more than 37.5 sigma above it, so every linear score is exactly 0.  The EHVI
    bot takes row 1; the log bot takes the 50-digit arg-max of the log score, and reports the log value."""
    import test_ehvi_host as TH
    from bot7_amd.grids.abstract import DeviceGrid
    from harness import benchmarks as B
    Bz, Base = _bot_module(), TH._stand_in()

    class StandIn(Base):
        def ehvi_nominate(self, other, front, ref):
            self.seen = self.post + other.post                      # the grid_remove that follows forgets the posteriors
            return super().ehvi_nominate(other, front, ref)

        def logehvi_nominate(self, other, front, ref):
            self.seen = self.post + other.post
            self.acc = R.logehvi_numpy(self.post[0], self.post[1], other.post[0], other.post[1], front, ref)
            i = R2.nominee_ref(self.acc)
            self.log.append(("logehvi_nominate", other.name, np.asarray(front).copy(), np.asarray(ref).copy()))
            return float(self.acc[i]), i + 1

    host = np.random.default_rng(3).random((40, 2))
    picks = {}
    for kind in (Bz.EHVI, LOG_EHVI):
        c1, c2 = StandIn("one"), StandIn("two")
        c1.grid_upload(host)
        bot = Bz.bayesopt(B.two_spheres, [], _ocfg(kind, ref=[-100.0, -100.0]),
                          {"model": TH._Model(c1), "candidates": DeviceGrid(host, c1, c1.grid_version)})
        bot.objective2 = {"ctx": c2, "grid": None, "model": TH._Model(c2)}
        for t in range(4):
            x, y = bot.run_trial()
            bot.update_best(x, y)
        last = bot.last_objectives
        assert last["front"].shape == (0, 2)
        lin = R2.ehvi_numpy(*c1.seen, last["front"], last["ref"])
        assert (lin == 0.0).all()
        picks[kind] = last
        if kind == LOG_EHVI:
            ref_mp = R.logehvi_mp(*c1.seen, last["front"], last["ref"])
            best, gap = R.argmax_mp(ref_mp)
            print("log bot: nominee %d, 50-digit arg-max %d (gap %.3g), log value %.6g" % (last["index"], best + 1, gap, last["value"]))
            assert gap >= 1e-9 and last["index"] == best + 1 and last["index"] != 1
            assert abs(last["value"] - float(ref_mp[best])) <= R.HOST_BAR * abs(float(ref_mp[best])) and last["value"] < -700.0
            assert [e[0] for e in c1.log if "nominate" in e[0]] == ["logehvi_nominate"]
    assert picks[Bz.EHVI]["index"] == 1 and picks[Bz.EHVI]["value"] == 0.0


def test_lua_shim_static_checks():
    """The new shim lines: the score class, and the log calls beside the linear ones with the declared number of arguments."""
    import test_lua_shims as L
    sc = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "scores_hip.lua")).read())
    assert "torch.class('bot7.scores.log_expected_hypervolume_improvement_hip', 'bot7.scores.abstract')" in sc
    assert "S.log_expected_hypervolume_improvement = LogEHVI" in sc
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos, called = L.prototypes(), dict(L.calls(bt))
    for name in ("b7_logehvi_nominate", "b7_logehvi3_nominate"):
        assert called[name] == protos[name], name
    for fn, call in (("nominate_objectives", "b7_logehvi_nominate(hip.ctx, o2.ctx, front, P[0], hip.data(ref), v, i)"),
                     ("nominate_objectives3", "b7_logehvi3_nominate(hip.ctx, self.objectives23[1].ctx, self.objectives23[2].ctx, front, P[0], hip.data(ref), v, i)")):
        i = bt.index("function bot:%s(" % fn)
        body = bt[i:bt.index("\nend", i)]
        assert "local logkind = torch.type(self.score) == 'bot7.scores.log_expected_hypervolume_improvement_hip'" in body
        assert body.index("if logkind then") < body.index(call) < body.index(call.replace("b7_log", "b7_"))
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
