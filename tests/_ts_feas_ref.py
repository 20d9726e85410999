"""References for constrained Thompson sampling (b7_ts_feas_nominate / b7_ts_feas_compute; bot7_amd/csrc/ts_feas.hip).

The float64 restatement of the key, operation for operation (numpy rounds every operator once, like the kernel with contraction off):

    viol = ((0 + max(c_1 - t_1, 0)) + max(c_2 - t_2, 0)) + ..        k ascending, a running sum from 0
    class -1 where any of the 1 + C values is NaN (viol NaN, the row never wins)
    class  0 where viol == 0, key f;  class 1 otherwise, key viol

the order (class 0 before class 1, the smaller key, the lowest row), the plain sequential pick with exclusions, and the same key in
exact rational arithmetic."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def keys(f, cvals, thresholds):
    """f [M, q], cvals [C, M, q], thresholds [C] -> (viol [M, q] with NaN for class -1, cls [M, q] int, key [M, q])."""
    f = np.asarray(f, dtype=np.float64)
    thr = np.asarray(thresholds, dtype=np.float64).ravel()
    cv = np.asarray(cvals, dtype=np.float64).reshape((thr.size,) + f.shape)
    nan = np.isnan(f)
    viol = np.zeros_like(f)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(thr.size):
            nan = nan | np.isnan(cv[k])
            d = cv[k] - thr[k]
            viol = viol + np.where(d > 0.0, d, 0.0)
    viol = np.where(nan, np.nan, viol)
    cls = np.where(nan, -1, np.where(viol == 0.0, 0, 1)).astype(np.int64)
    key = np.where(cls == 0, f, viol)
    return viol, cls, key


def best_row(cls, key, taken=()):
    """The best row of one path (cls [M], key [M]) over the rows not in `taken` -> (row, cls, key), or (-1, -1, NaN) where no row
    scores: class 0 before class 1, the smaller key, the lowest row."""
    best = (-1, -1, np.nan)
    taken = set(int(t) for t in taken)
    for want in (0, 1):
        rows = np.flatnonzero(cls == want)
        rows = rows[[int(r) not in taken for r in rows]] if taken else rows
        if rows.size:
            k = key[rows]
            r = int(rows[int(np.argmin(k))])       # argmin: the first minimum, rows ascending
            return r, want, float(key[r])
    return best


def replay(f, cvals, thresholds):
    """The plain sequential rule -> dict(index [q] 1-based (0: no row), cls [q], key [q], y [q, 1 + C], unexcluded [q] 0-based best
    over all rows, reruns: how many paths' unexcluded best had been taken)."""
    f = np.asarray(f, dtype=np.float64)
    thr = np.asarray(thresholds, dtype=np.float64).ravel()
    cv = np.asarray(cvals, dtype=np.float64).reshape((thr.size,) + f.shape)
    _, cls, key = keys(f, cv, thr)
    M, q = f.shape
    taken, out = [], {"index": np.zeros(q, dtype=np.int64), "cls": np.zeros(q, dtype=np.int64), "key": np.zeros(q),
                      "y": np.full((q, 1 + thr.size), np.nan), "unexcluded": np.zeros(q, dtype=np.int64), "reruns": 0}
    for j in range(q):
        r0 = best_row(cls[:, j], key[:, j])[0]
        r, c, k = best_row(cls[:, j], key[:, j], taken)
        out["unexcluded"][j] = r0
        out["reruns"] += int(r0 >= 0 and r0 in taken)
        out["index"][j], out["cls"][j], out["key"][j] = r + 1, c, k
        if r >= 0:
            taken.append(r)
            out["y"][j, 0] = f[r, j]
            out["y"][j, 1:] = cv[:, r, j]
    return out


def viol_exact(c_row, thresholds):
    """The total violation of one (row, path) in rational arithmetic: c_row [C] finite doubles -> Fraction."""
    total = Fraction(0)
    for c, t in zip(c_row, thresholds):
        d = Fraction(float(c)) - Fraction(float(t))
        if d > 0:
            total += d
    return total
