"""Three-objective nomination, host side (no GPU): the three host-only exports through the C ABI against their restatements and
against brute force over the coordinate grid (the box decomposition is an exact partition of the non-dominated region), the 50-digit
marginal against the explicit triple loop, the float64 restatement against 50 digits, the declarations of the new entry points
(header, Lua cdef, Python SYMBOLS), the score class, and the bot's bookkeeping on a stand-in context."""
import os
import re
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib

import _ehvi3_ref as R
import _exact as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_pareto_front3", "b7_nondominated_boxes3", "b7_hypervolume3", "b7_ehvi3_compute", "b7_ehvi3_nominate")
NAN = np.nan
REF = np.array([1.0, 2.0, 1.5])


def tie_laden(n, seed):
    """n rows rounded to quarters inside and around the box of REF: ties in every objective, duplicates, rows on the walls, NaN rows."""
    rng = np.random.default_rng(seed)
    Y = np.round(rng.random((n, 3)) * np.array([5.0, 9.0, 7.0])) / 4.0
    Y[rng.integers(0, n, max(1, n // 10))] = Y[rng.integers(0, n, max(1, n // 10))]      # duplicates
    Y[rng.integers(0, n, 2), rng.integers(0, 3, 2)] = NAN
    return Y


def _front_through_the_abi(Y, ref):
    front, rows = _lib.pareto_front3(Y, ref)
    wf, wr = R.canonical_front3(Y, ref)
    assert front.shape == wf.shape and front.tobytes() == wf.tobytes() and list(rows) == list(wr)
    assert R.is_canonical3(front, ref)
    return front, rows


def test_pareto_front3_through_the_c_abi():
    front, rows = _front_through_the_abi(np.zeros((0, 3)), REF)
    assert front.shape == (0, 3)
    front, rows = _front_through_the_abi([[0.25, 0.5, 0.75]], REF)
    assert list(rows) == [1]
    # dominated rows; equal rows: the lowest stays; a shared coordinate in ONE objective between non-dominated points is legal
    front, rows = _front_through_the_abi([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [0.5, 0.4, 0.9], [0.5, 0.9, 0.4]], REF)
    assert list(rows) == [5, 1, 4]
    front, rows = _front_through_the_abi([[NAN, 0.1, 0.1], [0.3, 0.3, NAN], [0.5, 0.5, 0.5], [-np.inf, 0.1, 0.1], [0.1, 0.1, np.inf]], REF)
    assert list(rows) == [3]
    # on and outside the walls: strictly inside in every objective
    front, rows = _front_through_the_abi([[1.0, 0.1, 0.1], [0.1, 2.0, 0.1], [0.1, 0.1, 1.5], [np.nextafter(1.0, 0), 0.2, 0.2], [0.0, 0.0, 3.0]], REF)
    assert list(rows) == [4]
    for seed in range(6):
        rng = np.random.default_rng(seed)
        front, _ = _front_through_the_abi(rng.random((60, 3)) * np.array([1.2, 2.4, 1.8]), REF)
        assert len(front) >= 3
        Y = tie_laden(80, seed)
        front, _ = _front_through_the_abi(Y, REF)
        for y in Y:       # every observed row inside the box is dominated by, or is, a front point
            if np.isfinite(y).all() and (y < REF).all():
                assert (front <= y).all(axis=1).any()
    # P beyond the cap: the count is written
    k = np.arange(_lib.EHVI3_PMAX + 1, dtype=np.float64)
    big = np.stack([k / 1000.0, 0.5 - k / 1000.0, np.full(len(k), 0.25)], axis=1)
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        _lib.pareto_front3(big, REF)
    assert e.value.code == -1 and str(_lib.EHVI3_PMAX + 1) in str(e.value)
    assert len(_lib.pareto_front3(big[:-1], REF)[0]) == _lib.EHVI3_PMAX
    with pytest.raises(bot7_amd.Bot7HipError):
        _lib.pareto_front3(big[:3], [np.inf, 1.0, 1.0])


def partition_counts(front, ref, boxes):
    """Over the coordinate grid of the front, extended by a cell (-inf, lowest coordinate] on every axis: how many boxes hold each
    cell, and which cells are dominated."""
    edges, dom = R.grid_cells(front, ref)
    lo = [np.concatenate([[-np.inf], e[:-1]]) for e in edges]
    hi = edges
    full = np.zeros(tuple(len(x) for x in lo), dtype=bool)
    full[1:, 1:, 1:] = dom
    count = np.zeros(full.shape, dtype=np.int64)
    for l1, u1, l2, u2, u3 in boxes:
        in1, in2, in3 = (lo[0] >= l1) & (hi[0] <= u1), (lo[1] >= l2) & (hi[1] <= u2), hi[2] <= u3
        count += (in1[:, None, None] & in2[None, :, None] & in3[None, None, :]).astype(np.int64)
    return count, full


def fronts_for_the_boxes():
    out = [("P=%d" % P, R.make_front3(P), R.REF3) for P in (0, 1, 2, 7, 33)]
    out += [("P=%d seed 1" % P, R.make_front3(P, seed=1), R.REF3) for P in (3, 12)]
    for seed in range(5):
        out.append(("ties %d" % seed, R.canonical_front3(tie_laden(90, 10 + seed), REF)[0], REF))
    for seed in range(3):     # eighths near a tilted plane: long fronts in which most coordinates are shared
        rng = np.random.default_rng(40 + seed)
        ab = rng.integers(0, 8, (60, 2)) / 8.0
        Y = np.concatenate([ab, (12 - 8 * ab.sum(axis=1, keepdims=True) + rng.integers(-1, 2, (60, 1))) / 8.0], axis=1)
        out.append(("ties on a plane %d" % seed, R.canonical_front3(Y, np.array([1.0, 1.0, 2.0]))[0], np.array([1.0, 1.0, 2.0])))
    rng = np.random.default_rng(4)
    for n in (5, 20):                                                  # general position: no coordinate shared
        out.append(("general %d" % n, R.canonical_front3(rng.random((n, 3)), np.array([1.0, 1.0, 1.0]))[0], np.array([1.0, 1.0, 1.0])))
    return out


def test_boxes_are_an_exact_partition_of_the_non_dominated_region():
    """Over the coordinate grid every non-dominated cell lies in exactly one box and no dominated cell in any; the library's boxes
    are the restatement's bit for bit; B <= 3P + 1, and 2P + 1 where no two points share a coordinate."""
    for label, front, ref in fronts_for_the_boxes():
        P = len(front)
        boxes = _lib.nondominated_boxes3(front, ref)
        assert boxes.tobytes() == R.boxes3(front, ref).tobytes(), label
        assert 1 <= len(boxes) <= 3 * P + 1 and len(boxes) <= 2 * P + 1, label
        if label.startswith("general"):
            assert len(boxes) == 2 * P + 1, label
        assert (boxes[:, 0] < boxes[:, 1]).all() and (boxes[:, 2] < boxes[:, 3]).all() and np.isfinite(boxes[:, [1, 3, 4]]).all(), label
        count, dom = partition_counts(front, ref, boxes)
        assert (count[dom] == 0).all() and (count[~dom] == 1).all(), label
    assert any(len(f) >= 6 and len(_lib.nondominated_boxes3(f, r)) < 2 * len(f) + 1 for lab, f, r in fronts_for_the_boxes() if lab.startswith("ties"))


def test_hypervolume3_against_brute_force():
    for label, front, ref in fronts_for_the_boxes():
        hv = _lib.hypervolume3(front, ref)
        assert hv == R.hypervolume3(front, ref), label
        want = R.hv_brute(front, ref)
        assert abs(hv - want) <= 64 * E.EPS * float(np.prod(ref)) * max(1, len(front)), label
        assert (hv > 0.0) == (len(front) > 0)
    # any point set (dominated rows, rows outside) through the front
    for seed in range(3):
        Y = tie_laden(70, 20 + seed)
        front, _ = _lib.pareto_front3(Y, REF)
        Yf = Y[np.isfinite(Y).all(axis=1)]
        assert abs(_lib.hypervolume3(front, REF) - R.hv_brute(Yf, REF)) <= 64 * E.EPS * float(REF.prod()) * len(front)


def test_box_sum_of_deterministic_points_is_the_hypervolume_improvement():
    """sum_b prod_m (u_bm - max(l_bm, y_m))+ against brute-force hypervolume differences."""
    rng = np.random.default_rng(7)
    for label, front, ref in fronts_for_the_boxes():
        boxes = _lib.nondominated_boxes3(front, ref)
        y = rng.uniform(-0.2, 1.1, (12, 3)) * ref
        if len(front):
            y[:3] = front[rng.integers(0, len(front), 3)] + rng.uniform(-0.05, 0.05, (3, 3))
            y[3] = front[0]
        want = R.hv_improvement3(front, ref, y)
        l = np.stack([boxes[:, 0], boxes[:, 2], np.full(len(boxes), -np.inf)], axis=1)
        u = np.stack([boxes[:, 1], boxes[:, 3], boxes[:, 4]], axis=1)
        got = np.maximum(u[None] - np.maximum(l[None], y[:, None, :]), 0.0).prod(axis=2).sum(axis=1)
        assert np.allclose(got, want, rtol=0, atol=64 * E.EPS * float(np.prod(ref)) * max(1, len(front))), label
        assert (got >= 0.0).all() and (len(front) == 0 or got[3] == 0.0)


def test_host_functions_refuse_what_is_not_canonical():
    ok = np.array([[0.5, 0.9, 0.4], [0.5, 0.5, 0.5], [0.5, 0.4, 0.9]])
    assert R.is_canonical3(ok, REF) and _lib.hypervolume3(ok, REF) > 0.0 and len(_lib.nondominated_boxes3(ok, REF)) >= 4
    bads = (ok[::-1],                                              # not sorted
            [[0.5, 0.5, 0.5], [0.6, 0.6, 0.6]],                    # dominated
            [[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]],                    # equal
            [[0.5, 2.0, 0.5]], [[0.5, 0.5, 1.5]], [[NAN, 0.1, 0.1]])
    for bad in bads:
        assert not R.is_canonical3(bad, REF)
        for fn in (_lib.hypervolume3, _lib.nondominated_boxes3):
            with pytest.raises(bot7_amd.Bot7HipError) as e:
                fn(bad, REF)
            assert e.value.code == -1 and "canonical" in str(e.value)
    with pytest.raises(bot7_amd.Bot7HipError):
        _lib.hypervolume3(ok, [1.0, np.inf, 1.0])


def test_marginal_against_the_triple_loop_and_the_restatement():
    """ehvi3_mp (slabs x strips over T tables) against the explicit S1 x S2 x S3 loop of single EHVIs at one row, to 1e-40; the
    float64 restatement (the library's boxes) against ehvi3_mp on thinned rows of the kernel tests' cases: row classes exactly, values
    within 1e-6 of the row's empty-front scale (the bound test_ehvi_host.py derives for Psi's deep tail)."""
    mu, var = R.make_rows3(24, (3, 2, 2), seed=5)
    for P in (0, 1, 7):
        front = R.make_front3(P, seed=1)
        fact = R.ehvi3_mp_both(mu, var, front, R.REF3)
        for j in (6, 11, 17):
            tri = R.ehvi3_mp_triple([m[:, j] for m in mu], [v[:, j] for v in var], front, R.REF3)
            with mpmath.workdps(50):
                assert abs(fact[j][0] - tri) <= mpmath.mpf("1e-40") * abs(tri), (P, j)
    worst = 0.0
    for M, P, S1, S2, S3 in R.KERNEL_CASES3:
        mu, var = R.make_rows3(M, (S1, S2, S3))
        keep = np.arange(M)[:: max(1, M // 12)]
        mu, var = [m[:, keep] for m in mu], [v[:, keep] for v in var]
        front = R.make_front3(P)
        got = R.ehvi3_numpy(mu, var, front, R.REF3)
        hi, lo, scale = R.ehvi3_mp(mu, var, front, R.REF3)
        assert np.array_equal(np.isnan(got), np.isnan(hi))
        ok = ~np.isnan(hi)
        assert (got[ok] >= 0.0).all() and np.isfinite(got[ok]).all() and (hi[ok] <= scale[ok] * (1 + 1e-15)).all()
        err = R.err_vs_mp(got, hi, lo)[ok]
        assert (err <= 1e-6 * scale[ok] + E.TINY).all()
        big = scale[ok] >= 1e-290
        worst = max(worst, (err[big] / scale[ok][big]).max() if big.any() else 0.0)
    print("ehvi3_numpy against 50 digits: worst error %.3g of the row's scale" % worst)


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
        i = HEADER.index(name + "(")
        comment = HEADER[HEADER.rindex("/*", 0, i):i]
        assert "no counterpart in the reference" in comment.lower(), name
    defs = gen_lua_cdef.defines(HEADER)
    assert defs["B7_ABI_VERSION"] == 1                      # additive: the version stays
    assert defs["B7_EHVI3_PMAX"] == _lib.EHVI3_PMAX == R.PMAX == 256 and "M.EHVI3_PMAX = 256" in lua
    i = HEADER.index("#define B7_EHVI3_PMAX")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    for word in ("No counterpart in the reference", "four or more objectives", "correlated objectives", "log-space EHVI", "batches", "refinement",
                 "constraints", "sharded grids and groups", "Bayesian-linear head", "trust regions"):
        assert word in comment, word
    # the two-objective comment says what is now true and keeps its words
    i = HEADER.index("#define B7_EHVI_PMAX")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    assert "more than two objectives" in comment and "b7_ehvi3_" in comment and "four and more" in comment
    src = open(os.path.join(ROOT, "bot7_amd", "csrc", "ehvi3.hip")).read()
    assert "No counterpart in the reference" in src and "four or more objectives" in src


def test_score_class_takes_two_other_contexts():
    from bot7_amd import scores
    s = scores.registry["expected_hypervolume_improvement"]({"type": "expected_hypervolume_improvement"})

    class Rec(object):
        def ehvi_nominate(self, other, front, ref):
            self.got = ("two", other, np.asarray(front).shape, list(ref))
            return 0.5, 7

        def ehvi3_nominate(self, other2, other3, front, ref):
            self.got = ("three", other2, other3, np.asarray(front).shape, list(ref))
            return 0.25, 9
    r, o2, o3 = Rec(), Rec(), Rec()
    assert s.nominate(r, (o2, o3), np.zeros((2, 3)), [1.0, 2.0, 3.0]) == (0.25, 9) and r.got == ("three", o2, o3, (2, 3), [1.0, 2.0, 3.0])
    assert s.nominate(r, o2, np.zeros((2, 2)), [1.0, 2.0]) == (0.5, 7) and r.got == ("two", o2, (2, 2), [1.0, 2.0])
    with pytest.raises(NotImplementedError) as e:
        s.nominate(r, (o2, o3, o3), np.zeros((2, 4)), [1.0, 2.0, 3.0, 4.0])
    assert "4 objectives" in str(e.value)
    for meth in ("ehvi3_compute", "ehvi3_nominate"):
        assert callable(getattr(bot7_amd.Context, meth)), meth
    assert callable(_lib.pareto_front3) and callable(_lib.nondominated_boxes3) and callable(_lib.hypervolume3)


# ---- the bot's bookkeeping on a stand-in context ------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401  (the package re-exports the class under the module's name)
    return sys.modules["harness.bots.bayesopt"]


def _stand_in():
    """oracle.hostctx.OracleContext (the device's stand-in of the CPU tests) with the calls of a three-objective trial on top: the
    kept posterior from the oracle's GP, the nomination from the float64 restatement."""
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

        def ehvi3_nominate(self, other2, other3, front, ref):
            posts = [self.post, other2.post, other3.post]
            assert all(p is not None and p[0].shape[1] == posts[0][0].shape[1] for p in posts)
            self.acc = R.ehvi3_numpy([p[0] for p in posts], [p[1] for p in posts], front, ref)
            i = R.nominee_ref(self.acc)
            self.log.append(("ehvi3_nominate", other2.name, other3.name, np.asarray(front).copy(), np.asarray(ref).copy()))
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


def _ocfg3(ref=None, **bot):
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "objectives": {"ref": ref, "models": [{"sample": True}, {}]}}, **bot),
            "grid": {"dims": 2}, "score": {"type": "expected_hypervolume_improvement"}}


def test_bot_bookkeeping_on_a_stand_in_context():
    from bot7_amd.grids.abstract import DeviceGrid
    from harness import benchmarks as B
    Bz, StandIn = _bot_module(), _stand_in()
    # three_spheres; the column split and the default reference point, per column
    x = np.array([[0.25, 0.25], [0.5, 0.5], [1.0, 0.0]])
    assert np.allclose(B.three_spheres(x), [[0.0, 0.125, 0.5], [0.125, 0.0, 0.125], [0.625, 0.5, 0.625]], rtol=0, atol=1e-15)
    assert B.registry["three_spheres"] is B.three_spheres
    resp = np.array([[1.0, 4.0, 0.0], [3.0, 2.0, 0.0], [2.0, NAN, 0.0], [2.0, 3.0, -1.0]])
    Ys = Bz.split_objectives3(resp)
    assert len(Ys) == 3 and all(Y.shape == (4, 1) and Y.flags["C_CONTIGUOUS"] for Y in Ys) and list(Ys[2][:, 0]) == [0.0, 0.0, 0.0, -1.0]
    with pytest.raises(ValueError):
        Bz.split_objectives3(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        Bz.split_objectives(np.zeros((3, 3)))                                            # the two-objective split still refuses three columns
    assert list(Bz.default_ref(resp)) == [3.0 + 0.1 * 2.0, 4.0 + 0.1 * 2.0, 0.0 + 0.1 * 1.0]
    assert list(Bz.default_ref(np.array([[1.0, 4.0], [3.0, 2.0], [2.0, NAN], [2.0, 3.0]]))) == [3.0 + 0.1 * 2.0, 4.0 + 0.1 * 2.0]
    # the loop: 3 random + 3 model-based trials on three_spheres
    host = np.random.default_rng(3).random((40, 2))
    c1, c2, c3 = StandIn("one"), StandIn("two"), StandIn("three")
    c1.grid_upload(host)
    models = [_Model(c1), _Model(c2), _Model(c3)]
    bot = Bz.bayesopt(B.three_spheres, [], _ocfg3(), {"model": models[0], "candidates": DeviceGrid(host, c1, c1.grid_version)})
    assert bot.config["bot"]["objectives"] == {"ref": None, "models": [dict(Bz.bayesopt._model_defaults({"sample": True}, 2)),
                                                                        dict(Bz.bayesopt._model_defaults({}, 2))]}
    bot.objectives23 = [{"ctx": c2, "grid": None, "model": models[1]}, {"ctx": c3, "grid": None, "model": models[2]}]
    hv = []
    for t in range(6):
        x, y = bot.run_trial()
        bot.update_best(x, y)
        bot.progress_report(t + 1, x, y)
        assert np.asarray(y).shape == (1, 3) and np.array_equal(y, B.three_spheres(x))
        ref = Bz.default_ref(bot.responses)
        wf, wr = R.canonical_front3(bot.responses, ref)
        assert np.array_equal(bot.best["front"], wf) and list(bot.best["rows"]) == list(wr) and np.array_equal(bot.best["ref"], ref)
        assert bot.best["hv"] == _lib.hypervolume3(wf, ref)
        hv.append(bot.best["hv"])
        if t < 3:
            assert not [e for c in (c1, c2, c3) for e in c.log if e[0] in ("eval_posterior", "ehvi3_nominate")]    # the initial trials touch no model
            continue
        last, n = bot.last_objectives, t                                               # n: observations this nomination saw
        for k, c in enumerate((c1, c2, c3)):
            e = [e for e in c.log if e[0] == "eval_posterior"][-1]
            assert e[1:3] == (2, 40 - n) and np.array_equal(e[3][:, 0], bot.responses[:n, k])      # column k, the same grid rows, nSamples
        nom = [e for e in c1.log if e[0] == "ehvi3_nominate"][-1]
        assert nom[1:3] == ("two", "three") and np.array_equal(nom[4], Bz.default_ref(bot.responses[:n])) and np.array_equal(nom[4], last["ref"])
        wf, wr = R.canonical_front3(bot.responses[:n], last["ref"])
        assert np.array_equal(nom[3], wf) and list(last["rows"]) == list(wr) and len(last["hyps"]) == 3
        for c in (c2, c3):
            assert np.array_equal(c1.X, c.X) and c.log[-1] == ("grid_remove", last["index"])     # the stolen row leaves all three grids
        assert np.array_equal(c1.X, np.asarray(bot.candidates)) and c1.X.shape == (40 - n - 1, 2) and c1.log[-1] == ("grid_remove", last["index"])
    for k, m in enumerate(models):
        assert m.inits[0].shape == (3, 1) and np.array_equal(m.inits[0][:, 0], bot.responses[:3, k]) and m.n == 3 * 3
    assert [e[1] for e in c2.log if e[0] == "grid_upload"] == [37] == [e[1] for e in c3.log if e[0] == "grid_upload"]
    assert hv[-1] > 0.0 and len(bot.best["front"]) >= 1
    # P = 0 on the first model-based trial: a fixed reference point below every observation
    c1, c2, c3 = StandIn("one"), StandIn("two"), StandIn("three")
    c1.grid_upload(host)
    bot = Bz.bayesopt(B.three_spheres, [], _ocfg3(ref=[-1.0, -1.0, -1.0]), {"model": _Model(c1), "candidates": DeviceGrid(host, c1, c1.grid_version)})
    bot.objectives23 = [{"ctx": c2, "grid": None, "model": _Model(c2)}, {"ctx": c3, "grid": None, "model": _Model(c3)}]
    for t in range(4):
        x, y = bot.run_trial()
        bot.update_best(x, y)
    assert bot.last_objectives["front"].shape == (0, 3) and bot.best["hv"] == 0.0 and list(bot.best["ref"]) == [-1.0, -1.0, -1.0]
    assert bot.last_objectives["value"] >= 0.0


def test_bot_refusals_by_name():
    Bz = _bot_module()
    cands = {"model": object(), "candidates": np.zeros((4, 2))}
    base = Bz.bayesopt(None, [], _ocfg3(), dict(cands)).config
    assert Bz.objectives_refusal(base) is None and Bz.objectives3_refusal(base) is None
    con = [{"threshold": 0.5, "model": {}}]
    obj4 = {"ref": None, "models": [{}, {}, {}]}
    cases = [(dict(base, bot=dict(base["bot"], batch=2)), {}, "batch"),
             (dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "refine"),
             (dict(base, bot=dict(base["bot"], constraints=con)), {}, "constraints"),
             (dict(base, bot=dict(base["bot"], trust_region={"perturb": 1.0})), {}, "trust_region"),
             (dict(base, score={"type": "expected_improvement"}), {}, "expected_improvement"),
             (dict(base, score={"type": "knowledge_gradient"}), {}, "knowledge_gradient"),
             (dict(base, bot=dict(base["bot"], objectives=obj4)), {}, "four or more objectives"),
             (base, {"sharded": True}, "sharded"),
             (base, {"model_class": "bot7.models.dngo"}, "dngo")]
    for cfg, kw, word in cases:
        why = Bz.objectives_refusal(cfg, **kw)
        assert why and word in why and "config.bot.objectives" in why, (word, why)
        assert "three" in why or word in ("constraints", "dngo", "expected_improvement", "knowledge_gradient", "four or more objectives")

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    for cfg, kw, word in cases[:5] + cases[6:7]:
        bot = Bz.bayesopt(None, [], cfg, {"model": M(), "candidates": np.zeros((4, 2))})
        with pytest.raises(NotImplementedError) as e:
            bot.run_trial()
        assert "config.bot" in str(e.value) and (word in str(e.value) or word == "trust_region")
        assert bot.nTrials == 0                                  # refused before anything moved


def test_the_two_objective_config_still_normalises_to_its_pinned_form():
    Bz = _bot_module()
    cfg = {"bot": {"verbose": 0, "nSamples": 2, "objectives": {"ref": (1, 2), "model": {"sample": True}}}, "grid": {"dims": 2},
           "score": {"type": "expected_hypervolume_improvement"}}
    bot = Bz.bayesopt(None, [], cfg, {"model": object(), "candidates": np.zeros((4, 2))})
    assert bot.config["bot"]["objectives"] == {"ref": [1.0, 2.0], "model": dict(Bz.bayesopt._model_defaults({"sample": True}, 2))}
    assert bot._objectives() and not bot._objectives3() and Bz.objectives_refusal(bot.config) is None
    bot3 = Bz.bayesopt(None, [], _ocfg3(ref=(1, 2, 3)), {"model": object(), "candidates": np.zeros((4, 2))})
    assert bot3.config["bot"]["objectives"]["ref"] == [1.0, 2.0, 3.0] and bot3._objectives3()
    plain = Bz.bayesopt(None, [], {"bot": {"verbose": 0}, "grid": {"dims": 2}}, {"model": object(), "candidates": np.zeros((4, 2))})
    assert plain.config["bot"]["objectives"] is None and not plain._objectives3()


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new one: its calls name declared functions with the declared number
    of arguments, nominate_objectives hands over to nominate_objectives3, which makes the Python mirror's calls in the mirror's order."""
    import test_lua_shims as L
    bt = L.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos, called = L.prototypes(), dict(L.calls(bt))
    for name in ("b7_eval_posterior", "b7_pareto_front2", "b7_ehvi_nominate", "b7_pareto_front3", "b7_ehvi3_nominate"):
        assert called[name] == protos[name], name
    i = bt.index("function bot:nominate_objectives(")
    assert "if obj.models then return self:nominate_objectives3(candidates) end" in bt[i:bt.index("\nend", i)]
    i = bt.index("function bot:nominate_objectives3(")
    body = bt[i:bt.index("\nend", i)]
    order = [body.index(w) for w in ("b7_pareto_front3(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P)",
                                     "b7_eval_posterior(hip.ctx, S, hyps, jit, info)", "follow_steal(o, self.objectives_idx, candidates)",
                                     "b7_eval_posterior(hip.ctx, S, hypsk, nil, nil)",
                                     "b7_ehvi3_nominate(hip.ctx, self.objectives23[1].ctx, self.objectives23[2].ctx, front, P[0], hip.data(ref), v, i)")]
    assert order == sorted(order)
    assert "self.nTrials <= self.config.bot.nInitial" in body and "R:narrow(2, 1, 1)" in body and "R:narrow(2, k + 1, 1)" in body
    assert "b7_create(ctxp, hip.device)" in body and "self.objectives_idx = tonumber(i[0])" in body and "hip.EHVI3_PMAX" in body
    for word in ("batch", "refine", "constraints", "trust_region", "group", "gp_hip", "four or more objectives"):          # the refusals, by name
        assert word in body, word
    L.test_lua_blocks_and_brackets_balance()
    L.test_cdef_block_is_the_header()
    L.test_every_ffi_call_matches_a_declared_prototype()
