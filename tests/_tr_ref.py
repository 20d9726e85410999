"""Restatements behind the trust-region tests (tests/test_tr_host.py, tests/test_gpu_tr.py).

  tr_map          the map of b7_grid_trust_region in numpy, integer-exact where the kernel is (uint64 splitmix64) and with the
                  kernel's rounded operations in the kernel's order where it is not: the GPU test compares BITS.
  tr_box_mp       b7_tr_box at 50 digits (mpmath), and tr_box_bar, the error a double evaluation may show, from its operation count.
  tr_replay       b7_tr_update's rules in plain Python (the tables of the host test are written out by hand; this replays a
                  bot's trace).

The generator is the library's counter-based one (csrc/counter_rng.h):
  splitmix64(z)            the published finaliser
  counter_key(seed, a)     splitmix64(splitmix64(seed) ^ a)
  counter_uniform(key, c)  (splitmix64(key + 0x9E3779B97F4A7C15 (2 c + 1)) >> 11) 2^-53
and the map's layout: key(seed, 0), counter g d + k: the mask's uniform of element (g, k); key(seed, 1), counter g: the uniform of
the forced column f(g) = min(d - 1, int(u d))."""
import math

import numpy as np

U64 = np.uint64
GOLD = U64(0x9E3779B97F4A7C15)
U = 2.0 ** -53   # the unit roundoff of a double


def splitmix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def counter_key(seed, stream):
    return splitmix64(splitmix64(U64(seed & (2 ** 64 - 1))) ^ U64(stream))


def counter_uniform(key, ctr):
    ctr = np.asarray(ctr, dtype=U64)
    with np.errstate(over="ignore"):
        a = splitmix64(key + GOLD * (U64(2) * ctr + U64(1)))
    return (a >> U64(11)).astype(np.float64) * U      # < 2^53: the conversion is exact


def forced_column(seed, g, d):
    """f(g) for the global row numbers g."""
    u = counter_uniform(counter_key(seed, 1), g)
    return np.minimum(d - 1, (u * float(d)).astype(np.int64))


def mask_draw(seed, g, d):
    """The mask's uniforms of rows g: len(g) x d."""
    g = np.asarray(g, dtype=U64)
    with np.errstate(over="ignore"):
        ctr = g[:, None] * U64(d) + np.arange(d, dtype=U64)[None, :]
    return counter_uniform(counter_key(seed, 0), ctr)


def tr_mask(seed, g, d, prob):
    """Which elements of rows g are perturbed -> (moved len(g) x d of bool, f len(g))."""
    f = forced_column(seed, g, d)
    moved = mask_draw(seed, g, d) < prob
    moved[np.arange(len(f)), f] = True
    return moved, f


def tr_map(base, center, lo, hi, prob, shift=None, seed=0, row_offset=0):
    """b7_grid_trust_region on the base points `base` (M x d, in [0, 1)) -> (X, moved)."""
    base = np.asarray(base, dtype=np.float64)
    M, d = base.shape
    center, lo, hi = (np.asarray(v, dtype=np.float64) for v in (center, lo, hi))
    moved, _ = tr_mask(seed, np.arange(M, dtype=np.int64) + row_offset, d, prob)
    t = base
    if shift is not None:
        t = base + np.asarray(shift, dtype=np.float64)[None, :]       # one rounded addition
        t = np.where(t >= 1.0, t - 1.0, t)                             # (exact)
    span = hi + (-lo)
    x = t * span[None, :]                                              # two rounded operations, never fused
    x = x + lo[None, :]
    x = np.where(x < lo[None, :], lo[None, :], x)
    x = np.where(x > hi[None, :], hi[None, :], x)
    return np.where(moved, x, np.broadcast_to(center, (M, d))), moved


# ---- b7_tr_box ---------------------------------------------------------------------------------------------------------------------
def tr_box_mp(lenscale_sq, center, length, mins, maxes, digits=50):
    """b7_tr_box at `digits` digits from the doubles given -> (lo, hi, half) as lists of mpf."""
    import mpmath
    with mpmath.workdps(digits):
        ls = [[mpmath.mpf(float(v)) for v in row] for row in np.atleast_2d(lenscale_sq)]
        S, d = len(ls), len(ls[0])
        rng = [mpmath.mpf(float(maxes[k])) - mpmath.mpf(float(mins[k])) for k in range(d)]
        logr = [sum(mpmath.log(ls[s][k]) / 2 for s in range(S)) / S - mpmath.log(rng[k]) for k in range(d)]
        mean = sum(logr) / d
        half = [mpmath.exp(logr[k] - mean) * mpmath.mpf(float(length)) * rng[k] / 2 for k in range(d)]
        lo = [max(mpmath.mpf(float(mins[k])), mpmath.mpf(float(center[k])) - half[k]) for k in range(d)]
        hi = [min(mpmath.mpf(float(maxes[k])), mpmath.mpf(float(center[k])) + half[k]) for k in range(d)]
        return lo, hi, half


def tr_box_bar(lenscale_sq, center, length, mins, maxes):
    """The absolute error a double evaluation of lo_k / hi_k may show, per column, from the operation count.  With u = 2^-53, a
    rounded operation's relative error at most u and log / exp within one unit in the last place (relative error at most 2u):
      t_sk = log(ls_sk) / 2                    |err| <= 2u |t_sk|                               (the halving is exact)
      a_k  = sum_s t_sk  (S - 1 additions)      |err| <= (S + 1) u A_k,  A_k = sum_s |t_sk|
      a_k / S                                    one more u;  log(range_k): range_k itself is a rounded difference (u), so
                                                 |err| <= u + 2u |log range_k|;  the subtraction: u |log r_k|
      => E_k = ((S + 2) u A_k) / S + u + 2u |log range_k| + u |log r_k|
      mean = (sum_j log r_j) / d                 |err| <= ((d - 1) u sum_j |log r_j| + sum_j E_j) / d + u |mean|  =: E_m
      z_k = log r_k - mean                       |err| <= E_k + E_m + u |z_k| =: D_k
      w_k = exp(z_k)                             relative error <= expm1(D_k) + 2u
      half_k = w_k length range_k / 2            two rounded products and range_k's own rounding: 3u   (the halving is exact)
      center_k -/+ half_k                        u |result|
    so |lo_k - exact| <= half_k (expm1(D_k) + 5u) (1 + 8u) + u |lo_k|.  A clipped side is exact."""
    ls = np.atleast_2d(np.asarray(lenscale_sq, dtype=np.float64))
    S, d = ls.shape
    mins, maxes, center = (np.asarray(v, dtype=np.float64) for v in (mins, maxes, center))
    rng = maxes - mins
    t = 0.5 * np.log(ls)
    A = np.abs(t).sum(axis=0)
    logr = t.sum(axis=0) / S - np.log(rng)
    E = (S + 2) * U * A / S + U + 2 * U * np.abs(np.log(rng)) + U * np.abs(logr)
    mean = logr.sum() / d
    Em = ((d - 1) * U * np.abs(logr).sum() + E.sum()) / d + U * abs(mean)
    z = logr - mean
    D = E + Em + U * np.abs(z)
    half = np.exp(z) * length * rng / 2.0
    side = np.maximum(np.abs(center - half), np.abs(center + half))
    return half * (np.expm1(D) + 5 * U) * (1 + 8 * U) + U * side


# ---- b7_tr_update ------------------------------------------------------------------------------------------------------------------
def default_fail_tol(d, q):
    return int(math.ceil(max(4.0 / q, float(d) / q)))


class TrReplay(object):
    """b7_tr_init / b7_tr_update in plain Python (the defaults are Eriksson et al.'s)."""

    def __init__(self, d, q=1, length_init=None, length_min=None, length_max=None, succ_tol=None, fail_tol=None):
        self.length_init = length_init if length_init and length_init > 0 else 0.8
        self.length_min = length_min if length_min and length_min > 0 else 2.0 ** -7
        self.length_max = length_max if length_max and length_max > 0 else 1.6
        self.succ_tol = succ_tol if succ_tol and succ_tol > 0 else 3
        self.fail_tol = fail_tol if fail_tol and fail_tol > 0 else default_fail_tol(d, q)
        self.restarts = 0
        self._reset()

    def _reset(self):
        self.length, self.best, self.succ, self.fail = self.length_init, None, 0, 0

    def update(self, y):
        vals = [float(v) for v in np.ravel(y) if not math.isnan(float(v))]
        ok = bool(vals) and (self.best is None or min(vals) < self.best - 1e-3 * abs(self.best))
        if ok:
            self.best, self.succ, self.fail = min(vals), self.succ + 1, 0
        else:
            self.succ, self.fail = 0, self.fail + 1
        if self.succ >= self.succ_tol:
            self.length, self.succ, self.fail = min(2.0 * self.length, self.length_max), 0, 0
        elif self.fail >= self.fail_tol:
            self.length, self.succ, self.fail = self.length / 2.0, 0, 0
        if self.length < self.length_min:
            self.restarts += 1
            self._reset()
            return True
        return False
