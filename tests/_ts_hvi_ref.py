"""References for multi-objective Thompson sampling (b7_ts_paths / b7_ts_hvi_nominate / b7_ts_hvi3_nominate / b7_hvi_compute;
bot7_amd/csrc/ts_hvi.hip).  All objectives are minimised.

  hvi2_numpy / hvi3_numpy   the kernels' formulas restated in numpy float64 in the kernels' operation order, one rounded operation per
                            operator: strips k ascending / boxes in b7_nondominated_boxes3's order, a running sum from 0; a row with an
                            entry that is not finite is NaN.
  hvi2_exact                the two-objective improvement in fractions.Fraction, from the region itself (the part of [y, ref] no
                            front point dominates, cut at the front's first coordinates) -> (hi, lo) float64 pairs.
  replay                    the pick rule from downloaded paths, the fallback included.
  special_rows              the rows of the kernel tests: on a front point, one ulp either side of a front coordinate, equal to ref,
                            beyond ref, dominating the whole front, NaN, +inf, -inf, then random rows around the box.
The fronts and the three-objective references are tests/_ehvi_ref.py's and tests/_ehvi3_ref.py's."""
from fractions import Fraction

import numpy as np

import _ehvi3_ref as R3
import _ehvi_ref as R2

U = 2.0 ** -53


def _pos(v):
    return np.where(v > 0.0, v, 0.0)


def hvi2_numpy(Y, front, ref):
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    av, bv = list(f[:, 0]) + [float(ref[0])], [float(ref[1])] + list(f[:, 1])
    y1, y2 = Y[:, 0], Y[:, 1]
    with np.errstate(all="ignore"):
        total, lo = np.zeros(len(Y)), -np.inf
        for a, b in zip(av, bv):
            w = _pos(a - np.where(lo > y1, lo, y1))
            h = _pos(b - y2)
            total = total + (w * h)
            lo = a
    total[~np.isfinite(Y).all(axis=1)] = np.nan
    return total


def hvi3_numpy(Y, front, ref, boxes=None):
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 3)
    bx = R3.boxes3(front, ref) if boxes is None else boxes
    y1, y2, y3 = Y[:, 0], Y[:, 1], Y[:, 2]
    with np.errstate(all="ignore"):
        total = np.zeros(len(Y))
        for l1, u1, l2, u2, u3 in np.asarray(bx, dtype=np.float64).reshape(-1, 5):
            w1 = _pos(u1 - np.where(l1 > y1, l1, y1))
            w2 = _pos(u2 - np.where(l2 > y2, l2, y2))
            w3 = _pos(u3 - y3)
            total = total + ((w1 * w2) * w3)
    total[~np.isfinite(Y).all(axis=1)] = np.nan
    return total


def hvi_numpy(Y, front, ref):
    return hvi2_numpy(Y, front, ref) if len(ref) == 2 else hvi3_numpy(Y, front, ref)


def hvi2_exact(Y, front, ref):
    """Per finite row of Y the area of {z: y <= z < ref, no front point <= z}, exactly.  The x axis is cut at every first coordinate
    of the front above y1; over a piece [e, e'] the region reaches from y2 up to the lowest second coordinate among the front points
    with a <= e (r2 where there is none).  Any point set will do: no canonical form is assumed."""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    r1, r2 = Fraction(float(ref[0])), Fraction(float(ref[1]))
    pts = [(Fraction(float(a)), Fraction(float(b))) for a, b in f]
    hi, lo = np.full(len(Y), np.nan), np.zeros(len(Y))
    for r, (p, q) in enumerate(Y):
        if not (np.isfinite(p) and np.isfinite(q)):
            continue
        y1, y2 = Fraction(float(p)), Fraction(float(q))
        area = Fraction(0)
        if y1 < r1 and y2 < r2:
            edges = sorted({y1, r1} | {a for a, _ in pts if y1 < a < r1})
            for e, e2 in zip(edges[:-1], edges[1:]):
                level = min([b for a, b in pts if a <= e] + [r2])
                if level > y2:
                    area += (e2 - e) * (level - y2)
        hi[r] = float(area)
        lo[r] = float(area - Fraction(hi[r]))
    return hi, lo


def canonical(points, ref):
    """b7_pareto_front2 / b7_pareto_front3 restated (tests/_ehvi_ref.canonical_front, tests/_ehvi3_ref.canonical_front3)."""
    m = len(ref)
    P = np.asarray(points, dtype=np.float64).reshape(-1, m)
    return (R2.canonical_front(P, ref) if m == 2 else R3.canonical_front3(P, ref))[0]


def ts_argmin(col, taken):
    """b7_ts_nominate's rule: the first minimum over the rows not taken, a NaN not winning (the first row left where all are NaN)."""
    free = np.ones(len(col), dtype=bool)
    free[list(taken)] = False
    ok = free & ~np.isnan(col)
    if not ok.any():
        return int(np.flatnonzero(free)[0])
    return int(np.flatnonzero(ok)[np.argmin(col[ok])])


def replay(paths, front, ref, score=hvi_numpy):
    """The pick rule from the m objectives' paths (M x q each) -> (hvi[q], rows[q] 0-based, y[q x m], fallback[q] bool).  Path j: the
    working front is the canonical front of (front, then the earlier picks' values under path j); the pick is the row of largest
    score among the rows not taken, ties to the lowest row, a NaN never winning; where no row scores above 0, the first minimum of
    objective (j mod m)'s path j over the rows not taken, and the value 0."""
    m, (M, q) = len(paths), paths[0].shape
    ref = np.asarray(ref, dtype=np.float64)
    front = np.asarray(front, dtype=np.float64).reshape(-1, m)
    rows, hv, ys, fb = [], np.zeros(q), np.zeros((q, m)), np.zeros(q, dtype=bool)
    for j in range(q):
        Yj = np.stack([p[:, j] for p in paths], axis=1)
        wf = canonical(np.concatenate([front, Yj[rows].reshape(-1, m)], axis=0), ref)
        s = score(Yj, wf, ref)
        s = np.where(np.isnan(s), -np.inf, s)
        s[rows] = -np.inf
        r = int(np.argmax(s))                  # the first of equal maxima
        if s[r] > 0.0:
            hv[j] = s[r]
        else:
            r, fb[j] = ts_argmin(paths[j % m][:, j], rows), True
        ys[j] = Yj[r]
        rows.append(r)
    return hv, np.asarray(rows, dtype=np.int64), ys, fb


def special_rows(front, ref, M1, seed=0):
    """M1 rows of m = len(ref) values: the special rows first (module docstring; those that need a front point are there for P >= 1),
    then random rows from half the box's extent below the front to a quarter beyond ref.  -> (Y, the number of special rows)."""
    ref = np.asarray(ref, dtype=np.float64)
    m = len(ref)
    f = np.asarray(front, dtype=np.float64).reshape(-1, m)
    rows = [ref.copy(), ref + 0.25, np.full(m, np.nan), np.full(m, np.inf), np.full(m, -np.inf)]
    rows.append((f.min(axis=0) if len(f) else ref) - 0.125)                      # dominates the whole front
    for k in sorted({0, len(f) // 2, len(f) - 1} - {-1}) if len(f) else ():
        rows.append(f[k].copy())                                                 # on a front point
        for c in range(m):
            for way in (-np.inf, np.inf):
                y = f[k].copy()
                y[c] = np.nextafter(y[c], way)
                rows.append(y)                                                   # one ulp either side of a front coordinate
    for c in range(m):                                                           # one entry not finite, the others ordinary
        for bad in (np.nan, np.inf, -np.inf):
            y = ref - 0.5
            y[c] = bad
            rows.append(y)
    n = len(rows)
    assert n <= M1
    rng = np.random.default_rng(4000 + seed + 7 * len(f) + m)
    rnd = rng.uniform(-0.5, 1.25, (M1 - n, m)) * ref
    return np.concatenate([np.asarray(rows), rnd], axis=0), n
