"""References for the two-objective expected hypervolume improvement (b7_ehvi_compute / b7_ehvi_nominate / b7_pareto_front2 /
b7_hypervolume2; bot7_amd/csrc/ehvi.hip).  Both objectives are minimised.

  ehvi_mp          the marginal  sum_k A_k B_k  in mpmath at 50 digits, per row -> (hi, lo) float64 pairs: the yardstick.
  ehvi_mp_double   the same marginal as the explicit S1 x S2 double loop of single EHVIs, at 50 digits (one row).
  ehvi_numpy       the library's form restated in numpy float64, one rounded operation per operator: the "how well can float64 do"
                   term of the bar.
  empty_scale_mp   Psi1(r1) Psi2(r2) marginalised, at 50 digits: the EHVI against an empty front, which bounds every EHVI of the row.
  canonical_front  b7_pareto_front2 restated; hypervolume: b7_hypervolume2 restated; dominated_area: a sweep over ANY point sets
                   (no canonical form assumed), and hv_improvement: that area with and without one extra point.
  fronts / rows    the case set of the kernel tests.

Front (a_k, b_k), k = 1..P: a strictly ascending, b strictly descending, inside the box of ref = (r1, r2).  a_0 = -inf, a_P+1 = r1,
b_0 = r2.  Psi(a; mu, sigma) = E[(a - y)+] = (a - mu) Phi(z) + sigma phi(z), z = (a - mu) / sigma."""
import math

import mpmath
import numpy as np

EPS = 2.0 ** -52
PMAX, SMAX, SREG = 256, 32, 10      # B7_EHVI_PMAX, B7_EHVI_SMAX, B7_EHVI_SREG
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
def _psi_mp(a, m, v, rs2):
    """a, m, v mpf (v >= 0); rs2 = 1/sqrt(2) at the working precision."""
    d = a - m
    if v == 0:
        return d if d > 0 else mpmath.mpf(0)
    s = mpmath.sqrt(v)
    z = d / s
    return d * (mpmath.erfc(-z * rs2) / 2) + s * (mpmath.exp(-z * z / 2) / mpmath.sqrt(2 * mpmath.pi))


def _bad(mu1, var1, mu2, var2):
    """Rows whose score is NaN: any mu or var NaN, or any var < 0, in either objective."""
    bad = np.zeros(np.asarray(mu1).shape[1], dtype=bool)
    for m, v in ((mu1, var1), (mu2, var2)):
        m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
        bad |= (np.isnan(m) | ~(v >= 0.0)).any(axis=0)
    return bad


def _strips(front, ref):
    """(a_1 .. a_P, r1), (r2, b_1 .. b_P): the upper edges of the P + 1 strips in each objective, as floats."""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    return list(f[:, 0]) + [float(ref[0])], [float(ref[1])] + list(f[:, 1])


def ehvi_mp_values(mu1, var1, mu2, var2, front, ref, dps=50):
    """Per row the mpf value of sum_k A_k B_k (None for a NaN-class row)."""
    mu1, var1, mu2, var2 = (np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (mu1, var1, mu2, var2))
    av, bv = _strips(front, ref)
    bad = _bad(mu1, var1, mu2, var2)
    out = []
    with mpmath.workdps(dps):
        rs2 = 1 / mpmath.sqrt(2)
        av, bv = [mpmath.mpf(x) for x in av], [mpmath.mpf(x) for x in bv]
        S1, S2 = mu1.shape[0], mu2.shape[0]
        for j in range(mu1.shape[1]):
            if bad[j]:
                out.append(None)
                continue
            p1 = [(mpmath.mpf(float(mu1[s, j])), mpmath.mpf(float(var1[s, j]))) for s in range(S1)]
            p2 = [(mpmath.mpf(float(mu2[t, j])), mpmath.mpf(float(var2[t, j]))) for t in range(S2)]
            prev = [mpmath.mpf(0)] * S1
            total = mpmath.mpf(0)
            for a, b in zip(av, bv):
                cur = [_psi_mp(a, m, v, rs2) for m, v in p1]
                A = sum((c - p for c, p in zip(cur, prev)), mpmath.mpf(0)) / S1      # Psi is monotone in a: no clamp at 50 digits
                B = sum((_psi_mp(b, m, v, rs2) for m, v in p2), mpmath.mpf(0)) / S2
                total += A * B
                prev = cur
            out.append(total)
    return out


def to_pairs(values, dps=50):
    """mpf values (None: NaN) -> (hi, lo) float64 arrays, hi + lo the value to ~1e-32 relative."""
    hi, lo = np.empty(len(values)), np.zeros(len(values))
    with mpmath.workdps(dps):
        for r, v in enumerate(values):
            if v is None:
                hi[r] = np.nan
                continue
            hi[r] = float(v)
            lo[r] = float(v - mpmath.mpf(hi[r]))
    return hi, lo


def ehvi_mp(mu1, var1, mu2, var2, front, ref):
    return to_pairs(ehvi_mp_values(mu1, var1, mu2, var2, front, ref))


def empty_scale_mp(mu1, var1, mu2, var2, ref):
    """Psi1(r1) Psi2(r2) marginalised, per row, as float64 (rounded from 50 digits; 0 for a NaN-class row)."""
    vals = ehvi_mp_values(mu1, var1, mu2, var2, np.zeros((0, 2)), ref)
    return np.array([0.0 if v is None else float(v) for v in vals])


def ehvi_mp_double(mu1, var1, mu2, var2, front, ref, dps=50):
    """One row (1-d arrays over the samples): (1 / (S1 S2)) sum_s sum_t EHVI_st, every single EHVI summed over its own strips."""
    av, bv = _strips(front, ref)
    with mpmath.workdps(dps):
        rs2 = 1 / mpmath.sqrt(2)
        av, bv = [mpmath.mpf(x) for x in av], [mpmath.mpf(x) for x in bv]
        total = mpmath.mpf(0)
        for m1, v1 in zip(mu1, var1):
            for m2, v2 in zip(mu2, var2):
                m1m, v1m, m2m, v2m = (mpmath.mpf(float(x)) for x in (m1, v1, m2, v2))
                prev, e = mpmath.mpf(0), mpmath.mpf(0)
                for a, b in zip(av, bv):
                    cur = _psi_mp(a, m1m, v1m, rs2)
                    e += (cur - prev) * _psi_mp(b, m2m, v2m, rs2)
                    prev = cur
                total += e
        return total / (len(mu1) * len(mu2))


def err_vs_mp(got, hi, lo):
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


# ---- the library's form in float64 ----------------------------------------------------------------------------------------------
def _psi_np(a, m, sd):
    """d = a - m, t = |d / sd|, f = max(phi(t) - t erfc(t / sqrt2) / 2, 0), 0 beyond t = 37.5; Psi = sd f (d <= 0), d + sd f (d > 0);
    sd == 0: max(d, 0)."""
    with np.errstate(all="ignore"):
        d = a - m
        t = np.abs(d / sd)
        pdf = np.exp((t * t) * -0.5) * 0.39894228040143267794
        q = _erfc(t * 0.70710678118654752440) * 0.5
        f = pdf - (t * q)
        f = np.where((f > 0.0) & (t <= 37.5), f, 0.0)             # beyond 37.5 both terms are below the smallest normal double
        g = sd * f
        return np.where(sd == 0.0, np.where(d > 0.0, d, 0.0), np.where(d > 0.0, d + g, g))


def ehvi_numpy(mu1, var1, mu2, var2, front, ref):
    """k ascending, s / t ascending within it, each sum divided once by its sample count, Psi(a_k; s) kept from strip to strip."""
    mu1, var1, mu2, var2 = (np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (mu1, var1, mu2, var2))
    av, bv = _strips(front, ref)
    S1, S2, M = mu1.shape[0], mu2.shape[0], mu1.shape[1]
    with np.errstate(all="ignore"):
        sd1, sd2 = np.sqrt(var1), np.sqrt(var2)
        prev = np.zeros((S1, M))
        score = np.zeros(M)
        for a, b in zip(av, bv):
            A, B = np.zeros(M), np.zeros(M)
            for s in range(S1):
                p = _psi_np(a, mu1[s], sd1[s])
                dd = p - prev[s]
                A = A + np.where(dd > 0.0, dd, 0.0)
                prev[s] = p
            for t in range(S2):
                B = B + _psi_np(b, mu2[t], sd2[t])
            score = score + ((A / float(S1)) * (B / float(S2)))
    score[_bad(mu1, var1, mu2, var2)] = np.nan
    return score


def nominee_ref(marginal):
    """b7_eval_nominate's rule: the first NaN, else the maximum, ties to the lowest index (0-based)."""
    nan = np.flatnonzero(np.isnan(marginal))
    return int(nan[0]) if len(nan) else int(np.argmax(marginal))


# ---- fronts and areas -----------------------------------------------------------------------------------------------------------
def canonical_front(Y, ref):
    """b7_pareto_front2 restated: rows with a non-finite entry or not strictly inside the box dropped, then a scan in the order
    (first objective, second objective, row): a row stays iff it lowers the running minimum of the second objective.
    -> (front P x 2, rows1 P: 1-based source rows)."""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    inside = [i for i in range(len(Y)) if np.isfinite(Y[i]).all() and Y[i, 0] < ref[0] and Y[i, 1] < ref[1]]
    inside.sort(key=lambda i: (Y[i, 0], Y[i, 1], i))
    keep, low = [], np.inf
    for i in inside:
        if Y[i, 1] < low:
            keep.append(i)
            low = Y[i, 1]
    return Y[keep].reshape(-1, 2).copy(), np.asarray(keep, dtype=np.int64) + 1


def is_canonical(front, ref):
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    return bool(np.isfinite(ref).all() and np.isfinite(f).all() and (f[:, 0] < ref[0]).all() and (f[:, 1] < ref[1]).all()
                and (np.diff(f[:, 0]) > 0).all() and (np.diff(f[:, 1]) < 0).all())


def hypervolume(front, ref):
    """b7_hypervolume2 restated: sum_k (a_k+1 - a_k)(r2 - b_k), k ascending, float64."""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    hv = 0.0
    for k in range(len(f)):
        nxt = f[k + 1, 0] if k + 1 < len(f) else float(ref[0])
        hv = hv + ((nxt - f[k, 0]) * (float(ref[1]) - f[k, 1]))
    return hv


def dominated_area(points, ref):
    """The area dominated inside the box by ANY point sets: points n x m x 2 (n sets of m points) -> n areas.  Every point is clipped
    onto the box (outside it, it then dominates nothing inside), the set sorted by the first objective, and the strip between two
    neighbours is as high as the best second objective seen so far reaches below r2."""
    P = np.array(points, dtype=np.float64)
    P = P[None] if P.ndim == 2 else P
    P[..., 0], P[..., 1] = np.minimum(P[..., 0], ref[0]), np.minimum(P[..., 1], ref[1])
    order = np.argsort(P[..., 0], axis=1, kind="stable")
    a, b = np.take_along_axis(P[..., 0], order, 1), np.take_along_axis(P[..., 1], order, 1)
    low = np.minimum.accumulate(b, axis=1)
    nxt = np.concatenate([a[:, 1:], np.full((len(a), 1), float(ref[0]))], axis=1)
    return ((nxt - a) * (ref[1] - low)).sum(axis=1)


def hv_improvement(front, ref, y):
    """By brute force: the dominated area of front + {y} minus that of the front alone; y n x 2 -> n improvements."""
    f = np.asarray(front, dtype=np.float64).reshape(-1, 2)
    y = np.asarray(y, dtype=np.float64).reshape(-1, 2)
    base = dominated_area(f[None], ref)[0] if len(f) else 0.0
    sets = np.concatenate([np.broadcast_to(f[None], (len(y),) + f.shape), y[:, None, :]], axis=1)
    return dominated_area(sets, ref) - base


# ---- the case set ---------------------------------------------------------------------------------------------------------------
REF = np.array([1.125, 1.0625])


def make_front(P, seed=0):
    """P canonical points in the unit square under REF; for P >= 2 the first two are ONE ULP apart in the first objective."""
    rng = np.random.default_rng(1000 + seed + P)
    a = np.sort(rng.random(P))
    b = np.sort(rng.random(P))[::-1].copy()
    for k in range(1, P):                     # strict, whatever the draws
        a[k] = max(a[k], np.nextafter(a[k - 1], np.inf))
        b[k] = min(b[k], np.nextafter(b[k - 1], -np.inf))
    if P >= 2:
        a[1] = np.nextafter(a[0], np.inf)
    front = np.stack([a, b], axis=1).reshape(-1, 2)
    assert is_canonical(front, REF)
    return front


def make_rows(M, S1, S2, seed=0, ref=REF, extent=1.0):
    """Synthetic posteriors mu / var, S x M each, around a front of the given extent under ref.  Half the rows place Psi(r)'s z by
    target, uniform in [-40, 8] (mu from far beyond ref to far below the front), the other half draw mu uniformly around the box;
    sigma log-uniform in [1e-8, 1e2] x extent.  Samples scatter around the row's (mu, sigma).  With M >= 16 the first rows are the
    special classes: var == 0 in one sample (rows 0, 1), in all (row 2, one of them -0.0), NaN mu (3), NaN var (4), var < 0 (5), and
    their complement, an ordinary row beside a NaN one (6)."""
    rng = np.random.default_rng(77 + seed + 131 * M + 17 * S1 + S2)
    out = []
    for S, r in ((S1, ref[0]), (S2, ref[1])):
        sig = extent * 10.0 ** rng.uniform(-8.0, 2.0, M)
        zt = rng.uniform(-40.0, 8.0, M)
        mu = np.where(np.arange(M) % 2 == 0, r - zt * sig, rng.uniform(r - 3.0 * extent, r + 2.0 * extent, M))
        mus = mu[None, :] + 0.1 * sig[None, :] * rng.standard_normal((S, M))
        sds = sig[None, :] * np.exp(0.2 * rng.standard_normal((S, M)))
        out += [mus, sds * sds]
    mu1, var1, mu2, var2 = out
    # A row whose scale Psi1(r1) Psi2(r2) would be a subnormal or nearly subnormal double (below 1e-290: 16 eps of it is no double
    # any more, and a bar made of it cannot tell one subnormal rounding from another) moves out to z = -60 in objective 1, where
    # float64 gives exactly 0 on every side; the deep tails with a scale a double still carries stay
    scale = ehvi_numpy(mu1, var1, mu2, var2, np.zeros((0, 2)), ref)
    for j in np.flatnonzero((scale > 0.0) & (scale < 1e-290)):
        mu1[:, j] = ref[0] + 60.0 * np.sqrt(var1[:, j]).max()
    if M >= 16:
        var1[0, 0] = 0.0
        var2[S2 - 1, 1] = 0.0
        var1[:, 2], var2[:, 2] = 0.0, 0.0
        var2[0, 2] = -0.0
        mu1[S1 - 1, 3] = np.nan
        var2[0, 4] = np.nan
        var1[0, 5] = -1e-300
    return mu1, var1, mu2, var2


# (M, P, S1, S2): M = 1000 is no multiple of the 64-lane workgroup and spans 16 of them; P covers 0, 1, 2, 33 and the cap; the
# sample counts cover 1, the register-resident limit, the first count beyond it (one sample in LDS) and the cap (22 in LDS each).
# (65, 2, 1, SREG + 1): objective 1 entirely in registers and one sample of objective 2 in LDS (x1 = 0, x2 = 1), the one corner of the
# kernel's computed LDS offsets that the others do not reach; 65 rows span two workgroups and end inside the second.
KERNEL_CASES = [(1000, 2, 3, 2), (257, 0, 1, 1), (257, 1, SREG, SREG), (1, 2, 1, 1), (40, 33, 3, 2), (5, PMAX, SREG + 1, 1),
                (257, 2, SREG + 1, 1), (70, 1, SMAX, SMAX), (65, 2, 1, SREG + 1)]
