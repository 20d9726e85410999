"""csrc/argbest.h on planted values: the five orderings through the shared part kernel and final kernel (diagnostic build:
b7dbg_argbest), and the workgroup reduction called in a loop (b7dbg_argbest_loop), against plain numpy restatements of each ordering.
Needs an MI355X: run with -m gpu.

Sizes: one row; one short of, exactly and one past a wave (63, 64, 65) and a workgroup (255, 256, 257); and 256 * 1024 + 3 rows, where
the pass has its 1024 workgroups and three threads take a second grid-stride trip.  Planted: copies of the extreme value in other
lanes, waves and workgroups and in the second trip; NaN at row 0, at the last row, and nothing but NaN; +-inf; 0 to 16 excluded rows
that begin with the winner, then every later winner (so every copy of the extreme), until nothing scorable is left.  Every answer is
compared bit for bit (row, and value with NaN == NaN)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = {0: "max, the first NaN wins", 1: "min, a NaN loses to every number", 2: "max, NaNs skipped", 3: "min, a NaN counts as +inf",
          4: "min, NaNs skipped"}
SMALL = (1, 63, 64, 65, 255, 256, 257)
LARGE = 256 * 1024 + 3
NONE = (-1, 0.0)


@pytest.fixture(scope="module")
def dctx():
    import bot7_amd
    c = bot7_amd.Context(0, lib="diag")
    c._L.b7dbg_argbest.restype = C.c_int
    c._L.b7dbg_argbest.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    c._L.b7dbg_argbest_loop.restype = C.c_int
    c._L.b7dbg_argbest_loop.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
    yield c
    c.close()


def ranked(order, v):
    """All rows that can be picked, best first: the ordering restated as one stable sort."""
    nan = np.isnan(v)
    rows = np.arange(v.size)
    if order == 0:   # NaNs first, in row order; then descending, equal values in row order
        rest = rows[~nan]
        return np.concatenate([rows[nan], rest[np.argsort(-v[rest], kind="stable")]])
    if order == 1:   # ascending, equal values in row order; NaNs last, in row order (numpy's own sort order)
        return np.argsort(v, kind="stable")
    if order == 2:
        rest = rows[~nan]
        return rest[np.argsort(-v[rest], kind="stable")]
    if order == 3:
        return np.argsort(np.where(nan, np.inf, v), kind="stable")
    rest = rows[~nan]
    return rest[np.argsort(v[rest], kind="stable")]


def best_ref(order, v, excl):
    """(row, value) of one pass with the rows `excl` left out, by a direct scan: no sort."""
    keep = np.ones(v.size, dtype=bool)
    keep[np.asarray(excl, dtype=np.int64)] = False
    rows = np.flatnonzero(keep)                 # the rows left, ascending: argmax / argmin name the first of equals
    nans, nums = rows[np.isnan(v[rows])], rows[~np.isnan(v[rows])]
    if order == 0:
        r = nans[0] if nans.size else nums[np.argmax(v[nums])] if nums.size else -1
    elif order == 1:
        r = nums[np.argmin(v[nums])] if nums.size else nans[0] if nans.size else -1
    elif order == 2:
        r = nums[np.argmax(v[nums])] if nums.size else -1
    elif order == 3:
        r = rows[np.argmin(np.where(np.isnan(v[rows]), np.inf, v[rows]))] if rows.size else -1
    else:
        r = nums[np.argmin(v[nums])] if nums.size else -1
    return (int(r), float(v[r])) if r >= 0 else NONE


def same(got, want):
    return got[0] == want[0] and (np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes() or (np.isnan(got[1]) and np.isnan(want[1])))


def dev_best(c, order, v, excl):
    e = np.asarray(excl, dtype=np.int64)
    val, row = C.c_double(-7.0), C.c_longlong(-7)
    rc = c._L.b7dbg_argbest(c._h, order, v.ctypes.data, v.size, e.ctypes.data if e.size else None, e.size, C.byref(val), C.byref(row))
    assert rc == 0
    return row.value, val.value


def spots(M):
    """Rows in different lanes, waves, workgroups and (at the large size) the second grid-stride trip; always the first and last."""
    cand = [0, 1, 37, 64, 70, 129, 255, 256, 300, 1000, 65536 + 5, 256 * 1024 - 1, 256 * 1024, M - 2, M - 1]
    return sorted({r for r in cand if 0 <= r < M})


def plantings(M):
    rng = np.random.default_rng(1000 + M)
    base = np.round(rng.standard_normal(M), 3)   # three decimals: plenty of exact ties among ordinary values too
    sp = spots(M)
    hi, lo = sp[0::2], sp[1::2]
    out = {}
    v = base.copy(); v[hi] = 9.5; v[lo] = -9.5
    out["copies of both extremes"] = v
    v = v.copy(); v[0] = np.nan
    out["NaN at row 0"] = v
    v = out["copies of both extremes"].copy(); v[M - 1] = np.nan
    out["NaN at the last row"] = v
    out["nothing but NaN"] = np.full(M, np.nan)
    v = base.copy(); v[hi] = np.inf; v[lo] = -np.inf
    out["+-inf"] = v
    v = v.copy(); v[sp[len(sp) // 2]] = np.nan; v[0] = np.nan
    out["+-inf and NaN"] = v
    return out


def exclusion_chain(order, v):
    """Up to 16 rows to exclude: the successive winners, then (nothing scorable left) the lowest rows not yet named."""
    chain = ranked(order, v)[:16].tolist()
    for r in range(v.size):
        if len(chain) >= 16:
            break
        if r not in chain:
            chain.append(r)
    return chain


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_pass_small(dctx, order):
    """Every small size, every planting, 0 .. min(16, M) exclusions."""
    n = 0
    for M in SMALL:
        for name, v in plantings(M).items():
            chain = exclusion_chain(order, v)
            rank = ranked(order, v)
            for k in range(len(chain) + 1):
                want = best_ref(order, v, chain[:k])
                assert want[0] == (int(rank[k]) if k < rank.size else -1), (ORDERS[order], M, name, k)   # the two restatements agree
                got = dev_best(dctx, order, v, chain[:k])
                assert same(got, want), (ORDERS[order], M, name, k, got, want)
                n += 1
    print("order %d (%s): %d passes" % (order, ORDERS[order], n))


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_one_pass_second_trip(dctx, order):
    """256 * 1024 + 3 rows: 1024 workgroups, the last three rows on a second trip; 0, 1, 5 and 16 exclusions."""
    for name, v in plantings(LARGE).items():
        chain = exclusion_chain(order, v)
        for k in (0, 1, 5, 16):
            want = best_ref(order, v, chain[:k])
            got = dev_best(dctx, order, v, chain[:k])
            assert same(got, want), (ORDERS[order], name, k, got, want)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_reduction_in_a_loop(dctx, order):
    """Sixteen successive picks by one workgroup that reduces sixteen times: the stable sort's first sixteen, then row -1 once every
    row is taken or cannot be scored."""
    for M in SMALL + (LARGE,):
        for name, v in plantings(M).items():
            rows, vals = np.full(16, -7, dtype=np.int64), np.full(16, -7.0)
            assert dctx._L.b7dbg_argbest_loop(dctx._h, order, v.ctypes.data, v.size, 16, vals.ctypes.data, rows.ctypes.data) == 0
            rank = ranked(order, v)[:16]
            want_rows = np.concatenate([rank, np.full(16 - rank.size, -1, dtype=np.int64)])
            want_vals = np.concatenate([v[rank], np.zeros(16 - rank.size)])
            assert rows.tolist() == want_rows.tolist(), (ORDERS[order], M, name, rows, want_rows)
            assert np.array_equal(vals, want_vals, equal_nan=True), (ORDERS[order], M, name)
