"""Log-space expected improvement, host side (no GPU): the float64 restatement of the device formula against 50-digit
arithmetic, the three declarations of the new entry points (header, Lua cdef, Python SYMBOLS), the score class and the Lua shim."""
import os
import re
import sys

import numpy as np

import bot7_amd
from bot7_amd import _lib

import _logei_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_score_logei", "b7_logei_compute")


def test_formula_against_50_digits_across_the_tail():
    """log EI = log sigma + log h(z) as score.hip evaluates it (z > -1: log(phi + z erfc(-z/sqrt2)/2); below: -z^2/2 - log(2 pi)/2 +
    log1p(-t sqrt(pi/2) erfcx(t/sqrt2))), in float64 with scipy, against mpmath on the exact values of the inputs: 3000 draws of
    z over [-1e6, 8] packed around -1, -8.6 and -38.6, sigma log-uniform in [1e-6, 1].  Bar 1e-14 in |err| / max(1, |ref|)
    (measured: 9.4e-16 on this formula).  The same rows through EI's own formula are 0 or noise below z ~ -8.6."""
    rng = np.random.default_rng(20231210)
    z = R.packed_z(rng, 3000)
    sigma = np.exp(rng.uniform(np.log(1e-6), 0.0, z.size))
    var = sigma * sigma
    mu = -(z * np.sqrt(var))            # fmin = 0, xi = 0: the device recomputes z from (mu, var), and so does the reference
    got = R.logei_np(mu, var, 0.0, 0.0)
    ref = R.logei_mp(mu, var, 0.0, 0.0)
    err = R.scaled_errors(got, ref)
    zz = -mu / np.sqrt(var)
    print("LogEI restatement: max scaled error %.3g at z = %.6g; z in [%.3g, %.3g]" % (err.max(), zz[err.argmax()], zz.min(), zz.max()))
    assert zz.min() < -9e5 and zz.max() > 7.0
    assert np.isfinite(got).all()
    assert err.max() <= R.HOST_BAR
    # with a trade-off: imprv = (fmin - mu) - xi
    got = R.logei_np(mu[:500], var[:500], 0.25, 0.5)
    assert R.scaled_errors(got, R.logei_mp(mu[:500], var[:500], 0.25, 0.5)).max() <= R.HOST_BAR


def test_far_tail_is_finite_ordered_and_exact():
    """z in [-1e12, -1e7]: r = t sqrt(pi/2) erfcx(t/sqrt2) is within an ulp of 1 there, and log1p(-r) taken from it is NaN wherever
    the three roundings of r land above 1 (shown first: that is why the formula has a tail).  The tail -2 log t + log1p(-3/t^2) is
    never NaN, strictly decreasing in t at fixed sigma, and meets the 50-digit value at the same bar as the rest (24 of the 50 digits
    go to the cancellation in phi + z Phi at t = 1e12).  Past t ~ 1.3e154, z^2/2 overflows: -inf, never NaN."""
    rng = np.random.default_rng(7)
    t = R.far_tail_t(rng, 2000)
    with np.errstate(all="ignore"):
        naive = np.log1p(-((t * R.SQRT_PI_2) * R.special.erfcx(t * R.SQRT1_2)))
    assert np.isnan(naive).any()                       # the hazard is real on this host's erfcx as well
    for sigma in (1.0, 1e-8):
        var = np.full(t.size, sigma * sigma)
        mu = t * sigma                                 # fmin = 0: z = -mu / sigma
        tt = mu / np.sqrt(var)
        assert tt.min() >= 9.9e6 and tt.max() <= 1.01e12
        got = R.logei_np(mu, var, 0.0, 0.0)
        assert np.isfinite(got).all()
        order = np.argsort(tt, kind="stable")
        assert (np.diff(got[order][np.diff(tt[order], prepend=0.0) > 0]) < 0).all()
        err = R.scaled_errors(got[::10], R.logei_mp(mu[::10], var[::10], 0.0, 0.0))
        print("LogEI restatement, far tail, sigma %g: max scaled error %.3g" % (sigma, err.max()))
        assert err.max() <= R.HOST_BAR
    # the two branches meet at t = 1e5 within the rounding of the -z^2/2 term (an ulp of 5e9 is 9.5e-7)
    edge = R.logei_np(np.array([np.nextafter(1e5, 0.0), 1e5]), np.ones(2), 0.0, 0.0)
    assert 0.0 <= edge[0] - edge[1] <= 4 * 9.5e-7
    out = R.logei_np(np.array([1e13, 1e100, 1e154, 1e155, 1e300]), np.ones(5), 0.0, 0.0)
    assert not np.isnan(out).any() and np.isfinite(out[:3]).all() and (out[3:] == -np.inf).all() and (np.diff(out[:3]) < 0).all()


def test_edge_cases_and_logaddexp_of_the_restatement():
    inf, nan = np.inf, np.nan
    #                 var == 0: imprv > 0, == 0, < 0;  var < 0;  var NaN;  mu NaN;  mu NaN at var == 0
    mu = np.array([-2.0, 0.0, 3.0, 0.0, 0.0, nan, nan])
    var = np.array([0.0, 0.0, 0.0, -1.0, nan, 1.0, 0.0])
    got = R.logei_np(mu, var, 0.0, 0.0)
    assert got[0] == np.log(2.0) and got[1] == -inf and got[2] == -inf and np.isnan(got[3:]).all()
    # z = +inf with sigma > 0 (the division overflows): log(imprv)
    assert R.logei_np(np.array([-1e300]), np.array([1e-300 ** 2 * 1e-20]), 0.0)[0] == np.log(1e300)
    a = np.array([-inf, -inf, 1.0, -800.0, nan, 2.0, inf, inf, inf])
    v = np.array([-inf, 3.0, 1.0, -10.0, 1.0, nan, inf, 5.0, -inf])
    out = R.logaddexp_np(a, v)
    assert out[0] == -inf and out[1] == 3.0 and out[2] == 1.0 + np.log1p(1.0) and out[3] == -10.0 and np.isnan(out[4:6]).all()
    assert (out[6:] == inf).all()                      # two samples with EI = +inf (var = +inf) marginalise to +inf, as linear EI does
    # the marginal is the log of the MEAN of EI, not the mean of the logs
    l1, l2 = R.logei_mp([1.0], [1e-4], 0.0), R.logei_mp([0.5], [1e-2], 0.0)
    want = float(R.logmeanexp_mp([l1, l2])[0])
    fold = R.logaddexp_np(R.logaddexp_np(-inf, float(l1[0])), float(l2[0])) - np.log(2.0)
    assert abs(fold - want) <= 1e-14 * abs(want) and abs(want - 0.5 * (float(l1[0]) + float(l2[0]))) > 1.0


def test_header_cdef_and_symbols_agree_on_the_new_entries():
    decls = {re.search(r"\b(b7_[a-z0-9_]+)\s*\(", d).group(1): d for d in gen_lua_cdef.cdef_lines(HEADER)
             if re.match(r"^(?!typedef).*\bb7_[a-z0-9_]+\s*\(", d)}
    lua = open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read()
    block = lua.split(gen_lua_cdef.BEGIN_CDEF)[1].split(gen_lua_cdef.END_CDEF)[0].splitlines()
    for name in NEW:
        assert name in decls, "include/bot7hip.h does not declare %s" % name
        assert decls[name] in block, "lua/bot7hip_ffi.lua does not carry the header's %s" % name
        assert name in _lib.SYMBOLS
    assert decls["b7_score_logei"] == decls["b7_score_ei"].replace("b7_score_ei", "b7_score_logei")
    assert decls["b7_logei_compute"] == decls["b7_ei_compute"].replace("b7_ei_compute", "b7_logei_compute")
    defs = gen_lua_cdef.defines(HEADER)
    assert defs["B7_SCORE_LOGEI"] == 3 == _lib.SCORE_LOGEI and defs["B7_SCORE_EI"] == 1 and defs["B7_SCORE_CB"] == 2
    assert defs["B7_ABI_VERSION"] == 1                      # additive: the version stays
    assert "M.SCORE_LOGEI = 3" in lua.split(gen_lua_cdef.BEGIN_CONST)[1].split(gen_lua_cdef.END_CONST)[0]
    # the declarations say where this comes from: not from the reference's scores/
    for name in NEW + ("B7_SCORE_LOGEI",):
        i = HEADER.index(name)
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "no counterpart" in comment.lower() and "Ament" in comment, name


def test_score_class_defaults_and_registry():
    from bot7_amd import scores
    assert scores.registry["log_expected_improvement"] is scores.log_expected_improvement
    lei, ei = scores.log_expected_improvement(), scores.expected_improvement()
    assert lei.config == ei.config == {"tradeoff": 0.0, "nFantasies": 100}
    assert scores.log_expected_improvement({"tradeoff": 0.5, "nFantasies": 7}).config == {"tradeoff": 0.5, "nFantasies": 7}
    assert lei.title == "bot7.scores.log_expected_improvement"
    Y = np.array([[3.0], [-1.5], [2.0]])
    spec = scores.log_expected_improvement({"tradeoff": 0.25}).device_spec(Y)
    assert spec["score"] == "logei" and list(spec["fmin"]) == [-1.5] and spec["tradeoff"] == 0.25
    s, fm = bot7_amd.Context._pack_spec("logei", [-1.5], 0.25, False, -1.0)
    assert (s.kind, s.tradeoff, s.fmin[0]) == (3, 0.25, -1.5)

    class Rec(object):
        def score_logei(self, fmin, tradeoff):
            self.got = (list(fmin), tradeoff)
    r = Rec()
    scores.log_expected_improvement({"tradeoff": 0.25}).add_to(r, Y)
    assert r.got == ([-1.5], 0.25)
    # the trial loop picks the score by config.score.type (a stub model and a given candidate set: no device is touched)
    from harness.bots.bayesopt import bayesopt
    cache = {"model": object(), "candidates": np.zeros((4, 2))}
    cfg = {"bot": {"verbose": 0}, "grid": {"dims": 2}, "score": {"type": "log_expected_improvement", "tradeoff": 0.5}}
    bot = bayesopt(None, [], cfg, cache)
    assert type(bot.score) is scores.log_expected_improvement and bot.score.config["tradeoff"] == 0.5
    assert type(bayesopt(None, [], {"bot": {"verbose": 0}, "grid": {"dims": 2}}, cache).score) is scores.expected_improvement


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new one: its calls name declared functions with the declared
    number of arguments, the class sits beside EI's with EI's defaults, and the fused bot maps it to B7_SCORE_LOGEI."""
    import test_lua_shims as L
    protos = L.prototypes()
    sc = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "scores_hip.lua")).read())
    seen = dict(L.calls(sc))
    assert seen["b7_score_logei"] == protos["b7_score_logei"] == 3
    assert "torch.class('bot7.scores.log_expected_improvement_hip', 'bot7.scores.abstract')" in sc
    body = sc[sc.index("bot7.scores.log_expected_improvement_hip"):]
    assert "config.tradeoff or 0.0" in body and "config.nFantasies or 100" in body and "S.log_expected_improvement = LEI" in body
    assert re.search(r"b7_score_reset\(hip\.ctx\)\)\s*hip\.check\(hip\.C\.b7_score_logei\(hip\.ctx, hip\.data\(fmins\)", body)
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    assert "'bot7.scores.log_expected_improvement_hip'" in bt and "hip.SCORE_LOGEI" in bt
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
