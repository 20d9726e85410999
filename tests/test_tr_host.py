"""Trust-region nomination, host side (no GPU): b7_tr_box through the C ABI against 50 digits, b7_tr_init / b7_tr_update against
transition tables written out by hand, the statistics of the numpy restatement of the map, the declarations of the new entry points
(header, Lua cdef, Python SYMBOLS), the Lua shim's static checks, and the bot's bookkeeping on a stand-in context."""
import ctypes as C
import math
import os
import re
import sys

import mpmath
import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib
from bot7_amd.grids.abstract import DeviceGrid, ResidentGrid

import _tr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_lua_cdef  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "bot7hip.h")).read()
NEW = ("b7_grid_trust_region", "b7_tr_box", "b7_tr_init", "b7_tr_update")
NAN = np.nan


# ---- b7_tr_box ---------------------------------------------------------------------------------------------------------------------
def _box_case(d, S, seed):
    rng = np.random.default_rng(seed)
    ls = 10.0 ** rng.uniform(-4.0, 4.0, size=(S, d))          # lengthscales over eight decades
    mins = rng.uniform(-3.0, 1.0, size=d)
    maxes = mins + 10.0 ** rng.uniform(-1.0, 1.5, size=d)      # ranges that are not 1
    center = mins + (maxes - mins) * rng.uniform(0.05, 0.95, size=d)
    center = np.minimum(np.maximum(center, mins), maxes)
    return ls, center, mins, maxes


WORST = {"ratio": 0.0}


@pytest.mark.parametrize("d", [1, 2, 6, 32, 96])
@pytest.mark.parametrize("S", [1, 3, 10])
def test_tr_box_against_50_digits(d, S):
    for rep, length in enumerate((0.8, 2.0 ** -7, 1.6, 0.05)):
        ls, center, mins, maxes = _box_case(d, S, 1000 * d + 10 * S + rep)
        lo, hi = _lib.tr_box(list(ls), center, length, mins, maxes)
        mlo, mhi, _ = R.tr_box_mp(ls, center, length, mins, maxes)
        bar = R.tr_box_bar(ls, center, length, mins, maxes)
        for k in range(d):
            elo = float(abs(mpmath.mpf(float(lo[k])) - mlo[k]))
            ehi = float(abs(mpmath.mpf(float(hi[k])) - mhi[k]))
            WORST["ratio"] = max(WORST["ratio"], elo / bar[k], ehi / bar[k])
            assert elo <= bar[k] and ehi <= bar[k], (d, S, k, elo, ehi, bar[k])
            assert mins[k] <= lo[k] <= center[k] <= hi[k] <= maxes[k]
    print("tr_box: worst error / bar so far %.3f" % WORST["ratio"])


def test_tr_box_volume_clipping_and_cube():
    # nothing clips: prod (hi - lo) = length^d prod range
    for d, S in ((2, 1), (6, 3), (32, 10)):
        rng = np.random.default_rng(d)
        ls = 10.0 ** rng.uniform(-0.2, 0.2, size=(S, d))      # mild anisotropy and a small box: no wall is reached
        mins, maxes = rng.uniform(-2.0, 0.0, size=d), rng.uniform(1.0, 3.0, size=d)
        center = 0.5 * (mins + maxes)
        length = 0.25
        lo, hi = _lib.tr_box(list(ls), center, length, mins, maxes)
        assert np.all(lo > mins) and np.all(hi < maxes)
        got = float(np.sum(np.log(hi - lo)))
        want = d * math.log(length) + float(np.sum(np.log(maxes - mins)))
        assert abs(got - want) <= 64 * d * R.U * max(1.0, abs(want))         # d logs, d rounded differences, two sums of d terms
    # equal lengthscales on equal ranges: a cube of side length * range
    d = 6
    lo, hi = _lib.tr_box([np.full(d, 0.37), np.full(d, 0.37)], np.full(d, 0.25), 0.4, np.full(d, -1.0), np.full(d, 3.0))
    assert np.allclose(hi - lo, 0.4 * 4.0, rtol=8 * R.U, atol=0) and len(set((hi - lo).tolist())) == 1
    assert np.allclose(0.5 * (lo + hi), 0.25, rtol=0, atol=8 * R.U)
    # clipping at either wall: the clipped side IS the wall, the other side is untouched
    mins, maxes = np.zeros(2), np.ones(2)
    free_lo, free_hi = _lib.tr_box([np.ones(2)], [0.5, 0.5], 0.4, mins, maxes)
    lo, hi = _lib.tr_box([np.ones(2)], [0.05, 0.5], 0.4, mins, maxes)
    assert lo[0] == 0.0 and hi[0] == 0.05 + 0.2 and (lo[1], hi[1]) == (free_lo[1], free_hi[1])
    lo, hi = _lib.tr_box([np.ones(2)], [0.5, 0.95], 0.4, mins, maxes)
    assert hi[1] == 1.0 and lo[1] == 0.95 - 0.2 and (lo[0], hi[0]) == (free_lo[0], free_hi[0])
    lo, hi = _lib.tr_box([np.ones(2)], [0.0, 1.0], 0.4, mins, maxes)         # the center on a wall
    assert (lo[0], hi[1]) == (0.0, 1.0)


def test_tr_box_refusals():
    L = _lib.load()
    d = 3
    good = dict(ls=np.ones(d), center=np.full(d, 0.5), length=0.8, mins=np.zeros(d), maxes=np.ones(d))

    def call(S=1, d_=d, null=None, **kw):
        a = dict(good, **kw)
        arrs = {k: np.ascontiguousarray(a[k], dtype=np.float64) for k in ("ls", "center", "mins", "maxes")}
        hyp = (_lib.Hyp * max(S, 1))()
        for s in range(max(S, 1)):
            hyp[s].lenscale_sq = arrs["ls"].ctypes.data_as(C.POINTER(C.c_double))
        lo, hi = np.empty(d), np.empty(d)
        ptr = {k: v.ctypes.data_as(C.c_void_p) for k, v in arrs.items()}
        ptr.update(lo=lo.ctypes.data_as(C.c_void_p), hi=hi.ctypes.data_as(C.c_void_p), hyp=hyp)
        if null:
            ptr[null] = None
        return L.b7_tr_box(d_, S, ptr["hyp"], ptr["center"], float(a["length"]), ptr["mins"], ptr["maxes"], ptr["lo"], ptr["hi"])

    assert call() == 0
    bad = [dict(ls=[1.0, 0.0, 1.0]), dict(ls=[1.0, -2.0, 1.0]), dict(ls=[1.0, NAN, 1.0]), dict(ls=[1.0, np.inf, 1.0]),
           dict(maxes=[1.0, 0.0, 1.0]), dict(maxes=[1.0, -1.0, 1.0]), dict(length=0.0), dict(length=-0.5), dict(length=NAN),
           dict(S=0), dict(center=[0.5, 1.5, 0.5]), dict(center=[-0.1, 0.5, 0.5]), dict(d_=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for null in ("hyp", "center", "mins", "maxes", "lo", "hi"):
        assert call(null=null) == -1, null
    with pytest.raises(_lib.Bot7HipError) as e:
        _lib.tr_box([np.ones(3)], [0.5, 0.5, 0.5], -1.0, np.zeros(3), np.ones(3))
    assert e.value.code == -1 and "length > 0" in str(e.value)


# ---- b7_tr_init / b7_tr_update ---------------------------------------------------------------------------------------------------
def _run(st, seq):
    """Feed the rows of seq = [(responses, restart, length, succ, fail, best)] and check every transition."""
    for n, (y, restart, length, succ, fail, best) in enumerate(seq):
        got = st.update(y)
        assert got is restart, (n, "restart")
        assert st.length == length and (st.succ, st.fail) == (succ, fail), (n, st.as_dict())
        assert (math.isnan(st.best) and best is None) or st.best == best, (n, st.best)


def test_tr_update_transition_tables():
    # three successes double the length; the cap at length_max; the counters start over
    st = _lib.TrustRegionState(6, 1)                                        # defaults: 0.8, 2^-7, 1.6, 3, ceil(max(4, 6)) = 6
    got = st.as_dict()
    assert math.isnan(got.pop("best")) and got == dict(length=0.8, length_init=0.8, length_min=2.0 ** -7, length_max=1.6, succ=0,
                                                       fail=0, succ_tol=3, fail_tol=6, restarts=0)
    _run(st, [([5.0], False, 0.8, 1, 0, 5.0),          # the first response sets best and counts as a success
              ([4.0], False, 0.8, 2, 0, 4.0),
              ([3.0], False, 1.6, 0, 0, 3.0),          # the third: 0.8 -> 1.6
              ([2.0], False, 1.6, 1, 0, 2.0),
              ([1.0], False, 1.6, 2, 0, 1.0),
              ([0.5], False, 1.6, 0, 0, 0.5),          # min(3.2, 1.6): capped
              ([0.6], False, 1.6, 0, 1, 0.5),          # worse: a failure, best stays
              ([0.4], False, 1.6, 1, 0, 0.4)])         # a success zeroes the failures
    # fail_tol failures halve the length; a success in between starts the streak over
    st = _lib.TrustRegionState(2, 1, 1.0, 0.3, 4.0, 2, 3)
    _run(st, [([1.0], False, 1.0, 1, 0, 1.0),
              ([2.0], False, 1.0, 0, 1, 1.0),
              ([2.0], False, 1.0, 0, 2, 1.0),
              ([0.5], False, 1.0, 1, 0, 0.5),
              ([0.7], False, 1.0, 0, 1, 0.5),
              ([0.7], False, 1.0, 0, 2, 0.5),
              ([0.7], False, 0.5, 0, 0, 0.5),          # three in a row: 1.0 -> 0.5
              ([0.7], False, 0.5, 0, 1, 0.5),
              ([0.7], False, 0.5, 0, 2, 0.5),
              ([0.7], True, 1.0, 0, 0, None)])         # 0.25 < 0.3: restart; length_init again, best unset
    assert st.restarts == 1
    _run(st, [([9.0], False, 1.0, 1, 0, 9.0)])         # the first response after the restart counts as a success, whatever it is
    # the restart fires exactly when length < length_min: halving ONTO length_min does not restart
    st = _lib.TrustRegionState(2, 1, 1.0, 0.5, 1.0, 3, 1)
    _run(st, [([1.0], False, 1.0, 1, 0, 1.0),
              ([1.0], False, 0.5, 0, 0, 1.0),          # 0.5 == length_min: no restart
              ([1.0], True, 1.0, 0, 0, None)])         # 0.25 < 0.5
    assert st.restarts == 1


def test_tr_update_threshold_nan_and_batches():
    # the 1e-3 |best| threshold from both sides: best = 2 -> a success needs y < 2 - 0.002
    below, above = float(np.nextafter(2.0 - 1e-3 * 2.0, -np.inf)), 2.0 - 1e-3 * 2.0
    st = _lib.TrustRegionState(2, 1, 1.0, 0.01, 4.0, 100, 100)
    _run(st, [([2.0], False, 1.0, 1, 0, 2.0),
              ([above], False, 1.0, 0, 1, 2.0),        # not strictly below the threshold
              ([1.9999], False, 1.0, 0, 2, 2.0),       # better than best, but by less than 1e-3 |best|
              ([below], False, 1.0, 1, 0, below)])
    st = _lib.TrustRegionState(2, 1, 1.0, 0.01, 4.0, 100, 100)
    _run(st, [([-2.0], False, 1.0, 1, 0, -2.0),        # a negative best: the threshold uses |best|
              ([-2.001], False, 1.0, 0, 1, -2.0),
              ([-2.003], False, 1.0, 1, 0, -2.003),
              ([0.0 - 2.003], False, 1.0, 0, 1, -2.003)])
    st = _lib.TrustRegionState(2, 1, 1.0, 0.01, 4.0, 100, 100)
    _run(st, [([0.0], False, 1.0, 1, 0, 0.0),          # best = 0: any strictly smaller value succeeds
              ([0.0], False, 1.0, 0, 1, 0.0),
              ([-1e-300], False, 1.0, 1, 0, -1e-300)])
    # NaN is a failure, also as the first response; it never becomes best
    st = _lib.TrustRegionState(2, 1, 1.0, 0.01, 4.0, 100, 100)
    _run(st, [([NAN], False, 1.0, 0, 1, None),
              ([3.0], False, 1.0, 1, 0, 3.0),
              ([NAN], False, 1.0, 0, 1, 3.0)])
    # q > 1 takes the minimum (a NaN among the q sits out)
    st = _lib.TrustRegionState(2, 3, 1.0, 0.01, 4.0, 100, 100)
    _run(st, [([5.0, 4.0, 6.0], False, 1.0, 1, 0, 4.0),
              ([4.5, 4.2, 4.0], False, 1.0, 0, 1, 4.0),
              ([4.5, NAN, 3.0], False, 1.0, 1, 0, 3.0),
              ([NAN, NAN, NAN], False, 1.0, 0, 1, 3.0)])
    # the default fail_tol: ceil(max(4 / q, d / q))
    for (d, q), want in {(2, 1): 4, (6, 1): 6, (32, 1): 32, (32, 8): 4}.items():
        assert _lib.TrustRegionState(d, q).fail_tol == want == R.default_fail_tol(d, q)
    assert _lib.TrustRegionState(3, 5).fail_tol == 1 and _lib.TrustRegionState(33, 8).fail_tol == 5
    # refusals
    L = _lib.load()
    st = _lib.TrState()
    for args in ((0, 1, 0.0, 0.0, 0.0, 0, 0), (2, 0, 0.0, 0.0, 0.0, 0, 0), (2, 1, NAN, 0.0, 0.0, 0, 0), (2, 1, 2.0, 0.0, 1.0, 0, 0),
                 (2, 1, 0.1, 0.5, 1.0, 0, 0), (2, 1, np.inf, 0.0, 0.0, 0, 0)):
        assert L.b7_tr_init(C.byref(st), *args) == -1, args
    assert L.b7_tr_init(None, 2, 1, 0.0, 0.0, 0.0, 0, 0) == -1
    assert L.b7_tr_init(C.byref(st), 2, 1, 0.0, 0.0, 0.0, 0, 0) == 0
    y = np.array([1.0])
    assert L.b7_tr_update(C.byref(st), None, 1, None) == -1 and L.b7_tr_update(None, y.ctypes.data_as(C.c_void_p), 1, None) == -1
    assert L.b7_tr_update(C.byref(st), y.ctypes.data_as(C.c_void_p), 0, None) == -1
    assert L.b7_tr_update(C.byref(st), y.ctypes.data_as(C.c_void_p), 1, None) == 0 and st.best == 1.0     # restart_out is nullable


def test_replay_class_follows_the_library():
    rng = np.random.default_rng(11)
    for q in (1, 4):
        a, b = _lib.TrustRegionState(5, q, 0.4, 0.11, 0.8, 2, 2), R.TrReplay(5, q, 0.4, 0.11, 0.8, 2, 2)
        for _ in range(60):
            y = rng.normal(size=q) + 3.0
            assert a.update(y) is b.update(y) and a.length == b.length and (a.succ, a.fail, a.restarts) == (b.succ, b.fail, b.restarts)
        assert a.restarts >= 1


# ---- the restatement of the map ------------------------------------------------------------------------------------------------------
def test_restatement_mask_statistics():
    """Fixed seeds, 10^5 rows.  The interval is 5 standard deviations of the binomial: a fair generator leaves it with probability
    5.7e-7 per check; the restatement passes, which is what is checked here."""
    n = 100000
    g = np.arange(n, dtype=np.int64) + 12345
    for seed, d, prob in ((1, 6, 0.625), (2, 32, 20.0 / 32.0), (3, 3, 0.1), (2 ** 63 + 5, 10, 0.5)):
        moved, f = R.tr_mask(seed, g, d, prob)
        free = np.ones((n, d), dtype=bool)
        free[np.arange(n), f] = False                                  # the non-forced columns
        share = moved[free].mean()
        sd = math.sqrt(prob * (1.0 - prob) / (n * (d - 1)))
        assert abs(share - prob) <= 5.0 * sd, (seed, d, prob, share, sd)
        assert moved[np.arange(n), f].all()                            # the forced column is always perturbed
        counts = np.bincount(f, minlength=d)
        sdc = math.sqrt(n * (1.0 / d) * (1.0 - 1.0 / d))
        assert counts.sum() == n and np.all(np.abs(counts - n / d) <= 5.0 * sdc), (seed, d, counts)
    for d in (1, 6, 39):
        moved0, f = R.tr_mask(7, g, d, 0.0)
        assert np.array_equal(moved0.sum(axis=1), np.ones(n, dtype=np.int64)) and moved0[np.arange(n), f].all()   # exactly one column
        assert R.tr_mask(7, g, d, 1.0)[0].all()                        # all of them


def test_restatement_map_properties():
    rng = np.random.default_rng(0)
    M, d = 500, 6
    base = rng.random((M, d))
    lo, hi = np.array([-1.0, 0.0, 0.25, 0.5, 2.0, -3.0]), np.array([1.0, 0.0, 0.75, 0.5000001, 2.5, -1.0])   # column 1: zero width
    center = np.array([0.3, 0.0, 0.25, 0.5, 2.25, -2.0])                                                 # column 2: touches lo
    shift = rng.random(d)
    X, moved = R.tr_map(base, center, lo, hi, 0.625, shift, seed=9, row_offset=77)
    assert np.all(X >= lo) and np.all(X <= hi)
    assert np.array_equal(X[~moved].view(np.uint64), np.broadcast_to(center, (M, d))[~moved].view(np.uint64))
    # slices with their row_offset are the slices of the whole
    a, _ = R.tr_map(base[:123], center, lo, hi, 0.625, shift, seed=9, row_offset=77)
    b, _ = R.tr_map(base[123:], center, lo, hi, 0.625, shift, seed=9, row_offset=77 + 123)
    assert np.array_equal(np.concatenate([a, b]), X)
    # without a rotation a perturbed entry is base * span + lo
    Y, mv = R.tr_map(base, center, lo, hi, 1.0, None, seed=9)
    assert mv.all() and np.array_equal(Y, np.minimum(np.maximum(base * (hi - lo) + lo, lo), hi))


# ---- declarations ----------------------------------------------------------------------------------------------------------------
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
    struct = [d for d in gen_lua_cdef.cdef_lines(HEADER) if d.endswith("b7_tr_state;")]
    assert len(struct) == 1 and struct[0] in block
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", struct[0].split("{")[1].split("}")[0])
    assert tuple(fields) == _lib.TrustRegionState.FIELDS == tuple(n for n, _ in _lib.TrState._fields_)
    assert gen_lua_cdef.defines(HEADER)["B7_ABI_VERSION"] == 1              # additive: the version stays
    i = HEADER.index("int b7_grid_trust_region(")
    comment = HEADER[HEADER.rindex("/*", 0, i):i]
    for word in ("Eriksson", "EVERY row", "no counterpart in the reference", "row_offset", "Cranley-Patterson", "additive"):
        assert word in comment, word
    rng_h = open(os.path.join(ROOT, "bot7_amd", "csrc", "counter_rng.h")).read()
    assert "b7_grid_trust_region" in rng_h and "key(seed, 1)   counter g " in rng_h      # the layout table names the new user
    for meth in ("grid_trust_region",):
        assert callable(getattr(bot7_amd.Context, meth)), meth
    assert callable(_lib.tr_box)


def test_lua_shim_static_checks():
    """What tests/test_lua_shims.py checks of every shim, for the new entries: the calls name declared functions with the declared
    number of arguments, and nominate_trust_region makes the Python mirror's calls in the mirror's order."""
    import test_lua_shims as Ls
    bt = Ls.strip_lua_comments(open(os.path.join(ROOT, "lua", "bots_bayesopt_hip.lua")).read())
    protos, called = Ls.prototypes(), dict(Ls.calls(bt))
    for name in NEW:
        assert called[name] == protos[name], name
    i = bt.index("function bot:nominate_trust_region(")
    body = bt[i:bt.index("\nend", i)]
    order = [body.index(w) for w in ("b7_tr_init(", "tr_base_grid(self, rec, mins, maxes)", "sample_hyps(model, X_win, Y_win, S, keep)", "b7_tr_box(",
                                     "tr_base_grid(self, rec, nil, nil)", "b7_grid_trust_region(", "local grid = hip.resident_only(M, d)",
                                     "self:nominate_batch(q, grid)")]
    assert order == sorted(order), order
    assert body.rstrip().endswith("return tr_rows(idx, d), rec")
    assert "b7_grid_sobol(hip.ctx, M, d, 1, hip.data(mins), hip.data(maxes), nil)" in bt and "b7_grid_download(hip.ctx, idx[k] - 1, 1," in bt
    assert "self.tr_since < cfg.bot.nInitial" in body and "model.sample_hypers, model.parse_hypers = nil, nil" in body
    for word in ("refine", "constraints", "objectives", "group", "gp_hip", "sobol"):       # the refusals, by name
        assert word in body, word
    j = bt.index("function bot:run_trial_trust_region(")
    body2 = bt[j:bt.index("\nend", j)]
    assert "b7_tr_update(" in body2 and "self.tr_start" in body2 and "self:nominate_trust_region()" in body2
    assert "if self.config.bot.trust_region then return self:run_trial_trust_region() end" in bt
    ff = Ls.strip_lua_comments(open(os.path.join(ROOT, "lua", "bot7hip_ffi.lua")).read())
    assert "function M.resident_only(" in ff
    Ls.test_lua_blocks_and_brackets_balance()
    Ls.test_cdef_block_is_the_header()
    Ls.test_every_ffi_call_matches_a_declared_prototype()


# ---- the resident-only handle --------------------------------------------------------------------------------------------------------
class _Ctx(object):
    """What a ResidentGrid needs of a context."""

    def __init__(self, X):
        self.X, self.grid_version, self.downloads = np.array(X, dtype=np.float64), 3, []

    def grid_shape(self):
        return self.X.shape

    def grid_download(self, row0=0, rows=None):
        self.downloads.append((row0, rows))
        return self.X[row0:row0 + rows].copy()


def test_resident_grid_handle():
    X = np.arange(20.0).reshape(5, 4)
    ctx = _Ctx(X)
    g = ResidentGrid(ctx, ctx.grid_version, X.shape)
    assert g.shape == (5, 4) and len(g) == 5
    assert np.array_equal(g.row(2), X[1]) and np.array_equal(g.rows([5, 1, 5]), X[[4, 0, 4]])
    assert ctx.downloads == [(1, 1), (4, 1), (0, 1), (4, 1)]                # just those rows cross
    with pytest.raises(TypeError) as e:
        np.asarray(g)
    assert "lives on the device" in str(e.value)
    with pytest.raises(IndexError):
        g.rows([6])
    with pytest.raises(IndexError):
        g.rows([0])
    ctx.grid_version += 1                                                   # the grid changed: the handle is stale
    with pytest.raises(RuntimeError):
        g.rows([1])
    # the model takes it for the resident grid exactly when context, row count and version match
    from bot7_amd.models.gp_regressor import gp_regressor
    m = gp_regressor.__new__(gp_regressor)
    m._ctx = ctx
    assert not m._is_resident(g)
    g2 = ResidentGrid(ctx, ctx.grid_version, X.shape)
    assert m._is_resident(g2) and not m._is_resident(ResidentGrid(ctx, ctx.grid_version, (4, 4)))
    assert not m._is_resident(ResidentGrid(_Ctx(X), ctx.grid_version, X.shape)) and not m._is_resident(X)
    assert m._is_resident(DeviceGrid(X, ctx, ctx.grid_version))             # what it took before, it still takes


# ---- the bot's bookkeeping on a stand-in context -------------------------------------------------------------------------------------
def _bot_module():
    import harness.bots  # noqa: F401  (the package re-exports the class under the module's name)
    return sys.modules["harness.bots.bayesopt"]


def _stand_in():
    """oracle.hostctx.OracleContext (the device's stand-in of the CPU tests) with the calls of a trust-region trial on top: the
    generators without a download, the map from the numpy restatement, and nominations that record what they were handed."""
    from oracle.hostctx import OracleContext

    class StandIn(OracleContext):
        def __init__(self):
            super().__init__()
            self.device_id, self.grid_version, self.log, self.fit_token = 0, 0, [], 0

        def _set(self, X):
            self.X = np.array(X, dtype=np.float64)
            self.grid_version += 1

        def grid_sobol(self, size, dims, skip=1, mins=None, maxes=None, download=True):
            assert not download
            u = np.random.default_rng(1000 + skip).random((size, dims))       # (any fixed base points do for the bookkeeping)
            self._set(u if mins is None else u * (np.asarray(maxes) - np.asarray(mins)) + np.asarray(mins))
            self.log.append(("grid_sobol", size, dims, skip, mins is not None))

        def grid_random(self, size, dims, seed=0, row_offset=0, mins=None, maxes=None, download=True):
            assert not download
            u = np.random.default_rng(seed % (2 ** 32)).random((size, dims))
            self._set(u if mins is None else u * (np.asarray(maxes) - np.asarray(mins)) + np.asarray(mins))
            self.log.append(("grid_random", size, dims, seed, mins is not None))

        def grid_upload(self, X):
            self.log.append(("grid_upload", np.asarray(X).shape[0]))
            self._set(X)

        def grid_download(self, row0=0, rows=None):
            self.log.append(("grid_download", row0, rows))
            return self.X[row0:row0 + rows].copy()

        def grid_trust_region(self, center, lo, hi, prob, shift=None, seed=0, row_offset=0):
            assert self.X.min() >= 0.0 and self.X.max() < 1.0                   # base points: the generator got no mins / maxes
            X, _ = R.tr_map(self.X, center, lo, hi, prob, shift, seed, row_offset)
            self._set(X)
            self.log.append(("grid_trust_region", np.array(center), np.array(lo), np.array(hi), prob, None if shift is None else np.array(shift), seed))

        def _pick(self, q):
            return [1 + (7 * k + len(self.log)) % self.X.shape[0] for k in range(q)]

        def eval_nominate(self, hyps, **spec):
            self.log.append(("eval_nominate", len(hyps), self.X.shape[0], np.asarray(self.Y).copy(), [h["lenscale_sq"][0] for h in hyps]))
            return 0.0, self._pick(1)[0]

        def eval_nominate_batch(self, hyps, q, **spec):
            self.log.append(("eval_nominate_batch", len(hyps), self.X.shape[0], np.asarray(self.Y).copy(), q))
            return [0.0] * q, self._pick(q)

        def ts_nominate(self, hyps, q, n_features=1024, seed=0):
            self.log.append(("ts_nominate", len(hyps), self.X.shape[0], np.asarray(self.Y).copy(), q))
            return [0.0] * q, self._pick(q)

    return StandIn


class _Model(object):
    """A model whose hyper samples count the sampler's calls, and whose stage records the grid handle it was given."""

    def __init__(self, ctx, d):
        self.ctx, self.d, self.n, self.inits, self.staged = ctx, d, 0, [], []

    def class_(self):
        return "bot7.models.gp_regressor"

    def init(self, X, Y):
        self.inits.append((np.asarray(X).copy(), np.asarray(Y).copy()))

    def sample_hypers(self, X, Y, *a):
        Y = np.asarray(Y)
        assert Y.shape == (len(X), 1)
        self.n += 1
        return np.concatenate([np.full(self.d, 0.3 + 0.01 * self.n), [1.0, 1e-4, float(np.mean(Y))]])

    def parse_hypers(self, v):
        return {"lenscale_sq": np.asarray(v[:self.d]), "amp": float(v[self.d]), "noise": float(v[self.d + 1]), "mean": float(v[self.d + 2])}

    def stage(self, X, Y, grid):
        self.staged.append(grid)
        assert isinstance(grid, ResidentGrid) and grid.ctx is self.ctx and grid.version == self.ctx.grid_version   # nothing to upload
        self.ctx.gp_set_data(np.asarray(X), np.asarray(Y).reshape(len(X), -1))


def _tcfg(score="expected_improvement", base="random", d=3, **bot):
    tr = {"length_init": 0.4, "length_min": 0.19, "failure_tolerance": 2, "success_tolerance": 2}
    return {"bot": dict({"verbose": 0, "nInitial": 3, "nSamples": 2, "seed": 5, "trust_region": tr}, **bot),
            "grid": {"dims": d, "size": 50, "type": base, "mins": np.full(d, -2.0), "maxes": np.full(d, 3.0)},
            "score": {"type": score}}


class _TS(object):
    config = {"nFeatures": 64}

    def nominate(self, ctx, hyps, q, seed):
        return ctx.ts_nominate(hyps, q, n_features=64, seed=seed)[1]


def _decreasing_then_flat():
    """An objective by call count: improving for a while, then flat, so that halvings and a restart certainly occur."""
    state = {"n": 0}

    def f(x):
        state["n"] += 1
        return 10.0 - state["n"] if state["n"] <= 5 else 100.0
    return f


@pytest.mark.parametrize("score,q,base", [("expected_improvement", 1, "random"), ("expected_improvement", 3, "sobol"),
                                          ("thompson_sampling", 1, "sobol"), ("thompson_sampling", 2, "random")])
def test_bot_bookkeeping_on_a_stand_in_context(score, q, base):
    Bz, StandIn = _bot_module(), _stand_in()
    d = 3
    ctx = StandIn()
    model = _Model(ctx, d)
    cache = {"model": model}
    if score == "thompson_sampling":
        cache["score"] = _TS()
    bot = Bz.bayesopt(_decreasing_then_flat(), [], _tcfg(score, base, d, batch=q), cache)
    assert bot.candidates is None                                            # no grid is generated up front
    tr = bot.config["bot"]["trust_region"]
    assert tr["perturb"] == 1.0 and tr["base"] == base and tr["length_max"] is None     # min(1, 20 / d); the library's defaults
    replay = R.TrReplay(d, q, 0.4, 0.19, None, 2, 2)
    start, since, restarts = 0, 0, 0
    for t in range(14):
        n_before, log_before, calls_before = 0 if bot.observed is None else bot.observed.shape[0], len(ctx.log), model.n
        x, y = bot.run_trial()
        bot.update_best(x, y)
        rec, new = bot.tr_trace[-1], ctx.log[log_before:]
        assert len(bot.tr_trace) == t + 1 and bot.nTrials == t + 1
        assert bot.observed.shape == (n_before + q, d) and bot.responses.shape == (n_before + q, 1)          # the record is global
        assert np.array_equal(rec["x"], bot.observed[n_before:]) and np.array_equal(rec["y"], bot.responses[n_before:])
        assert rec["length_before"] == replay.length
        for key in ("trial", "kind", "base", "index", "length_before", "length_after", "center", "lo", "hi", "shift", "map_seed",
                    "prob", "restart", "x", "y"):
            assert key in rec, key                                            # the trace is complete
        if since < 3:                                                          # an initial trial: random rows of a global base grid
            assert rec["kind"] == "initial" and model.n == calls_before and not [e for e in new if "nominate" in e[0]]
            assert new[0][0] == "grid_" + base and new[0][-1] is True         # mapped to mins / maxes by the generator
            assert [e[0] for e in new[1:]] == ["grid_download"] * q and len(set(rec["index"])) == q
            assert np.all(rec["x"] >= -2.0) and np.all(rec["x"] <= 3.0)
        else:
            assert rec["kind"] == "model" and model.n == calls_before + 3     # the burn-in call and nSamples draws, ONCE
            assert [e[0] for e in new[:2]] == ["grid_" + base, "grid_trust_region"] and new[0][-1] is False
            assert (base == "sobol") == (rec["shift"] is not None) and (base == "random") == ("base_seed" in rec)
            nom = new[2]
            want = {("expected_improvement", 1): "eval_nominate", ("expected_improvement", 3): "eval_nominate_batch"}.get((score, q), "ts_nominate")
            assert nom[0] == want and nom[1:3] == (2, 50)
            assert np.array_equal(nom[3][:, 0], bot.responses[start:n_before, 0])          # the model saw the window only
            assert isinstance(model.staged[-1], ResidentGrid)                 # the branch was handed the resident-only handle
            win_X, win_Y = bot.observed[start:n_before], bot.responses[start:n_before, 0]
            assert np.array_equal(rec["center"], win_X[int(np.argmin(win_Y))])           # the best row since the restart
            lo, hi = _lib.tr_box(rec["hyps"], rec["center"], rec["length_before"], np.full(d, -2.0), np.full(d, 3.0))
            assert np.array_equal(lo, rec["lo"]) and np.array_equal(hi, rec["hi"])
            assert np.array_equal(new[1][1], rec["center"]) and new[1][6] == rec["map_seed"] and new[1][4] == 1.0
            assert np.all(rec["x"] >= rec["lo"]) and np.all(rec["x"] <= rec["hi"])
            assert [e[0] for e in new[3:]] == ["grid_download"] * q
        since += 1
        if since == 3:
            assert np.array_equal(model.inits[-1][0], bot.observed[start:]) and len(model.inits) == restarts + 1   # init on the window
        restart = replay.update(bot.responses[n_before:, 0])
        assert rec["restart"] is restart and rec["length_after"] == replay.length == bot.tr_state.length
        if restart:
            start, since, restarts = bot.observed.shape[0], 0, restarts + 1
        assert (bot.tr_start, bot.tr_since) == (start, since)
    assert restarts >= 1 and bot.tr_state.restarts == restarts               # the window moved at least once
    assert not [e for e in ctx.log if e[0] == "grid_upload"]                 # no grid ever crossed to the device
    assert float(np.ravel(bot.best["y"])[0]) == bot.responses.min()          # best stays the run's


def test_bot_refusals_by_name_and_the_default_path():
    Bz = _bot_module()
    base = Bz.bayesopt(None, [], _tcfg(), {"model": object()}).config
    assert Bz.trust_region_refusal(base) is None
    plain = Bz.bayesopt(None, [], {"bot": {"verbose": 0}, "grid": {"dims": 2}}, {"model": object(), "candidates": np.zeros((4, 2))})
    assert plain.config["bot"]["trust_region"] is None and Bz.trust_region_refusal(plain.config) is None and not plain._trust_region()
    con = [{"threshold": 0.5, "model": {}}]
    wide = dict(base, grid=dict(base["grid"], dims=40, type="sobol"), bot=dict(base["bot"], trust_region=dict(base["bot"]["trust_region"], base="sobol")))
    cases = [(dict(base, bot=dict(base["bot"], refine={"starts": 2})), {}, "refine"),
             (dict(base, bot=dict(base["bot"], constraints=con)), {}, "constraints"),
             (dict(base, bot=dict(base["bot"], objectives={"ref": None, "model": {}})), {}, "objectives"),
             (dict(base, score={"type": "expected_hypervolume_improvement"}), {}, "expected_hypervolume_improvement"),
             (base, {"sharded": True}, "sharded"),
             (base, {"sharded": True}, "group"),
             (base, {"model_class": "bot7.models.dngo"}, "dngo"),
             (wide, {}, "sobol"),
             (dict(base, bot=dict(base["bot"], trust_region=dict(base["bot"]["trust_region"], base="halton"))), {}, "halton"),
             (dict(base, bot=dict(base["bot"], batch=17)), {}, "batch")]
    for cfg, kw, word in cases:
        why = Bz.trust_region_refusal(cfg, **kw)
        assert why and word in why and "config.bot.trust_region" in why, (word, why)

    class M(object):
        ctx = None

        def class_(self):
            return "bot7.models.gp_regressor"

    for cfg, kw, word in cases[:4] + cases[7:]:
        bot = Bz.bayesopt(None, [], cfg, {"model": M()})
        with pytest.raises(NotImplementedError) as e:
            bot.run_trial()
        assert word in str(e.value) and bot.nTrials == 0                    # refused before anything moved
    # trust_region = None leaves run_trial on the parent's path: the trust-region trial is never entered
    called = []
    plain._run_trial_trust_region = lambda: called.append(1)
    plain.objective = lambda x: 1.0
    plain.run_trial()
    assert not called and plain.nTrials == 1 and plain.candidates.shape == (3, 2) and plain.tr_trace == []
