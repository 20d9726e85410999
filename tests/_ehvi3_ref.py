"""References for the three-objective expected hypervolume improvement (b7_ehvi3_compute / b7_ehvi3_nominate / b7_pareto_front3 /
b7_nondominated_boxes3 / b7_hypervolume3; bot7_amd/csrc/ehvi3.hip).  All objectives are minimised.

  ehvi3_mp          the marginal in mpmath at 50 digits, per row -> (hi, lo) float64 pairs: the yardstick.  It uses a decomposition of
                    its OWN, not the library's boxes: the slabs between consecutive distinct third coordinates, each times the
                    two-dimensional strip sum over the staircase of the points at or below the slab's floor (O(P^2) per row).
  ehvi3_mp_triple   the same marginal as the explicit S1 x S2 x S3 loop of single EHVIs, at 50 digits (one row).
  ehvi3_numpy       the library's form restated in numpy float64, one rounded operation per operator: the "how well can float64 do"
                    term of the bar.
  empty_scale_mp    T1(r1) T2(r2) T3(r3) at 50 digits: the EHVI against an empty front, which bounds every EHVI of the row.
  canonical_front3 / boxes3 / hypervolume3   the three host functions restated; is_canonical3.
  hv_brute          the volume ANY point set dominates inside the box, as a union of cells of the coordinate grid; hv_improvement3.
  make_front3 / make_rows3 / KERNEL_CASES3   the case set of the kernel tests.

T_m(c) = (1/S_m) sum_s Psi(c; mu_ms, sigma_ms), Psi(a; mu, sigma) = E[(a - y)+]; T_m(-inf) = 0."""
import mpmath
import numpy as np

import _ehvi_ref as R2

EPS = R2.EPS
PMAX, SMAX = 256, R2.SMAX          # B7_EHVI3_PMAX, B7_EHVI_SMAX
REF3 = np.array([1.125, 1.0625, 1.03125])
nominee_ref, err_vs_mp, to_pairs = R2.nominee_ref, R2.err_vs_mp, R2.to_pairs


def _bad3(mu, var):
    """Rows whose score is NaN: any mu or var NaN, or any var < 0, in any objective."""
    bad = np.zeros(np.atleast_2d(mu[0]).shape[1], dtype=bool)
    for m, v in zip(mu, var):
        m, v = np.atleast_2d(np.asarray(m, dtype=np.float64)), np.atleast_2d(np.asarray(v, dtype=np.float64))
        bad |= (np.isnan(m) | ~(v >= 0.0)).any(axis=0)
    return bad


def _f3(front):
    return np.asarray(front, dtype=np.float64).reshape(-1, 3)


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
def _staircase(pts):
    """(a, b) pairs, any order -> the staircase: a ascending, b strictly descending."""
    st, low = [], None
    for a, b in sorted(pts):
        if low is None or b < low:
            st.append((a, b))
            low = b
    return st


def _slab_sum(front, ref, T1, T2, T3, zero):
    """sum over the slabs of the third objective of [T3(top) - T3(floor)] x the two-dimensional strip sum
    sum_k [T1(a_k+1) - T1(a_k)] T2(b_k) over the staircase of the points with c <= floor; T1 / T2 / T3 map a float cut to a value."""
    f = _f3(front)
    zs = sorted(set(f[:, 2]))
    total = T1(float(ref[0])) * T2(float(ref[1])) * T3(zs[0] if zs else float(ref[2]))     # below every point: nothing is dominated
    for i, z in enumerate(zs):
        top = zs[i + 1] if i + 1 < len(zs) else float(ref[2])
        st = _staircase([(p[0], p[1]) for p in f if p[2] <= z])
        edges = [a for a, _ in st] + [float(ref[0])]
        levels = [float(ref[1])] + [b for _, b in st]
        area, prev = zero, zero
        for a, b in zip(edges, levels):
            cur = T1(a)
            area += (cur - prev) * T2(b)
            prev = cur
        total += area * (T3(top) - T3(z))
    return total


def ehvi3_mp_both(mu, var, front, ref, dps=50):
    """Per row (the mpf marginal, the mpf empty-front scale); (None, None) for a NaN-class row."""
    mu = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in mu]
    var = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in var]
    bad = _bad3(mu, var)
    out = []
    with mpmath.workdps(dps):
        rs2, zero = 1 / mpmath.sqrt(2), mpmath.mpf(0)
        for j in range(mu[0].shape[1]):
            if bad[j]:
                out.append((None, None))
                continue

            def table(m):
                ps = [(mpmath.mpf(float(mu[m][s, j])), mpmath.mpf(float(var[m][s, j]))) for s in range(mu[m].shape[0])]
                memo = {}

                def T(c):
                    if c not in memo:
                        memo[c] = sum((R2._psi_mp(mpmath.mpf(c), mm, vv, rs2) for mm, vv in ps), zero) / len(ps)
                    return memo[c]
                return T
            T1, T2, T3 = table(0), table(1), table(2)
            out.append((_slab_sum(front, ref, T1, T2, T3, zero), T1(float(ref[0])) * T2(float(ref[1])) * T3(float(ref[2]))))
    return out


def ehvi3_mp(mu, var, front, ref):
    """-> (hi, lo, scale): the marginal as float64 pairs, the empty-front scale as float64 (0 for a NaN-class row)."""
    both = ehvi3_mp_both(mu, var, front, ref)
    hi, lo = to_pairs([b[0] for b in both])
    return hi, lo, np.array([0.0 if b[1] is None else float(b[1]) for b in both])


def empty_scale_mp(mu, var, ref):
    return ehvi3_mp(mu, var, np.zeros((0, 3)), ref)[2]


def ehvi3_mp_triple(mu, var, front, ref, dps=50):
    """One row (mu[m], var[m] 1-d over the samples): (1 / (S1 S2 S3)) sum_s sum_t sum_u EHVI_stu, every single EHVI by the slab sum."""
    with mpmath.workdps(dps):
        rs2, zero = 1 / mpmath.sqrt(2), mpmath.mpf(0)
        total = zero
        for m1, v1 in zip(mu[0], var[0]):
            for m2, v2 in zip(mu[1], var[1]):
                for m3, v3 in zip(mu[2], var[2]):
                    Ts = [(lambda c, mm=mpmath.mpf(float(mm)), vv=mpmath.mpf(float(vv)): R2._psi_mp(mpmath.mpf(c), mm, vv, rs2))
                          for mm, vv in ((m1, v1), (m2, v2), (m3, v3))]
                    total += _slab_sum(front, ref, Ts[0], Ts[1], Ts[2], zero)
        return total / (len(mu[0]) * len(mu[1]) * len(mu[2]))


# ---- the three host functions restated ----------------------------------------------------------------------------------------------
def canonical_front3(Y, ref):
    """b7_pareto_front3 restated: rows with a non-finite entry or not strictly inside the box dropped; the rest in the order (third,
    first, second, row); a row stays iff no row kept before it is <= it in every objective.  -> (front P x 3, rows1 P)."""
    Y = _f3(Y)
    inside = [i for i in range(len(Y)) if np.isfinite(Y[i]).all() and (Y[i] < ref).all()]
    inside.sort(key=lambda i: (Y[i, 2], Y[i, 0], Y[i, 1], i))
    keep = []
    for i in inside:
        if not any((Y[q] <= Y[i]).all() for q in keep):
            keep.append(i)
    return Y[keep].reshape(-1, 3).copy(), np.asarray(keep, dtype=np.int64) + 1


def is_canonical3(front, ref):
    f = _f3(front)
    if not (np.isfinite(ref).all() and np.isfinite(f).all() and (f < np.asarray(ref)).all()):
        return False
    keys = [(p[2], p[0], p[1]) for p in f]
    if any(not a < b for a, b in zip(keys, keys[1:])):
        return False
    return not any((f[q] <= f[k]).all() for k in range(len(f)) for q in range(len(f)) if q != k)


def boxes3(front, ref):
    """b7_nondominated_boxes3 restated -> B x 5: l1, u1, l2, u2, u3."""
    f, out, st = _f3(front), [], []
    for a, b, c in f:
        i = 0
        while i < len(st) and st[i][0] <= a:
            i += 1
        level = float(ref[1]) if i == 0 else st[i - 1][1]
        if not level > b:
            continue
        x, j = a, i
        while True:
            nx = st[j][0] if j < len(st) else float(ref[0])
            out.append([x, nx, b, level, c])
            if j == len(st):
                break
            level = st[j][1]
            if not level > b:
                break
            x, j = nx, j + 1
        st = sorted([p for p in st if not (p[0] >= a and p[1] >= b)] + [(a, b)])
    for k in range(len(st) + 1):
        out.append([-np.inf if k == 0 else st[k - 1][0], st[k][0] if k < len(st) else float(ref[0]), -np.inf,
                    float(ref[1]) if k == 0 else st[k - 1][1], float(ref[2])])
    return np.asarray(out, dtype=np.float64).reshape(-1, 5)


def hypervolume3(front, ref):
    """b7_hypervolume3 restated: slabs between distinct third coordinates, each the staircase area of the points at or below its
    floor (sum_k (a_k+1 - a_k)(r2 - b_k), k ascending) times its height, float64."""
    f, hv, k, pts = _f3(front), 0.0, 0, []
    while k < len(f):
        z = f[k, 2]
        while k < len(f) and f[k, 2] == z:
            pts.append((f[k, 0], f[k, 1]))
            k += 1
        znext = f[k, 2] if k < len(f) else float(ref[2])
        st, area = _staircase(pts), 0.0
        for i, (a, b) in enumerate(st):
            nxt = st[i + 1][0] if i + 1 < len(st) else float(ref[0])
            area = area + ((nxt - a) * (float(ref[1]) - b))
        hv = hv + (area * (znext - z))
    return hv


# ---- brute force ----------------------------------------------------------------------------------------------------------------
def grid_cells(points, ref):
    """The coordinate grid of ANY point set under ref: per axis the sorted distinct coordinates below r_m, then r_m.  -> (edges[3],
    dominated: bool array over the cells [e_i, e_i+1] of the three axes -- a cell is dominated iff a point is <= its lower corner)."""
    p = _f3(points)
    p = p[(p < np.asarray(ref)).all(axis=1)] if len(p) else p
    edges = [np.array(sorted(set(p[:, m])) + [float(ref[m])]) for m in range(3)]
    lo = [e[:-1] for e in edges]
    dom = np.zeros(tuple(len(x) for x in lo), dtype=bool)
    for q in p:
        dom |= (lo[0][:, None, None] >= q[0]) & (lo[1][None, :, None] >= q[1]) & (lo[2][None, None, :] >= q[2])
    return edges, dom


def hv_brute(points, ref):
    """The volume dominated inside the box by ANY point set, as the sum of the dominated cells of the coordinate grid.  A point with
    a coordinate at or beyond r_m dominates nothing inside the box and is left out."""
    p = np.minimum(_f3(points), np.asarray(ref, dtype=np.float64))
    p = p[(p < np.asarray(ref)).all(axis=1)] if len(p) else p      # a point on a wall dominates a set of volume 0
    if not len(p):
        return 0.0
    edges, dom = grid_cells(p, ref)
    w = [np.diff(e) for e in edges]
    return float((dom * (w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :])).sum())


def hv_improvement3(front, ref, y):
    """By brute force: hv_brute of front + {y} minus that of the front alone; y n x 3 -> n improvements."""
    f, y = _f3(front), _f3(y)
    base = hv_brute(f, ref)
    return np.array([hv_brute(np.concatenate([f, q[None]], axis=0), ref) - base for q in y])


def hv_improvement3_exact(front, ref, y):
    """hv_brute's union of cells in RATIONAL arithmetic: per row of y the volume of the cells of the coordinate grid of front + {y}
    that y dominates and no front point does, exactly, as (hi, lo) float64 pairs."""
    from fractions import Fraction
    f, y = _f3(front), _f3(y)
    hi, lo = np.zeros(len(y)), np.zeros(len(y))
    for r, q in enumerate(y):
        if not (q < np.asarray(ref)).all():
            continue
        edges, dom = grid_cells(np.concatenate([f, q[None]], axis=0), ref)
        lows = [e[:-1] for e in edges]
        mine = (lows[0][:, None, None] >= q[0]) & (lows[1][None, :, None] >= q[1]) & (lows[2][None, None, :] >= q[2])
        theirs = np.zeros(dom.shape, dtype=bool)
        for p in f:
            theirs |= (lows[0][:, None, None] >= p[0]) & (lows[1][None, :, None] >= p[1]) & (lows[2][None, None, :] >= p[2])
        w = [[Fraction(float(b)) - Fraction(float(a)) for a, b in zip(e[:-1], e[1:])] for e in edges]
        v = sum((w[0][i] * w[1][j] * w[2][k] for i, j, k in zip(*np.nonzero(mine & ~theirs))), Fraction(0))
        hi[r] = float(v)
        lo[r] = float(v - Fraction(hi[r]))
    return hi, lo


# ---- the library's form in float64 ----------------------------------------------------------------------------------------------
def ehvi3_numpy(mu, var, front, ref):
    """T_m per distinct cut, s ascending, each sum divided once by its sample count; the boxes in the decomposition's order, per box
    ((d1 * d2) * T3(u3)) with d = max(T(u) - T(l), 0) added to the running sum."""
    mu = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in mu]
    var = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in var]
    M = mu[0].shape[1]
    bx = boxes3(front, ref)
    with np.errstate(all="ignore"):
        tabs = []
        for m, cols in enumerate(((0, 1), (2, 3), (4,))):
            sd, tab = np.sqrt(var[m]), {-np.inf: np.zeros(M)}
            for c in sorted(set(bx[:, cols].ravel()) - {-np.inf}):
                acc = np.zeros(M)
                for s in range(mu[m].shape[0]):
                    acc = acc + R2._psi_np(c, mu[m][s], sd[s])
                tab[c] = acc / float(mu[m].shape[0])
            tabs.append(tab)
        score = np.zeros(M)
        for l1, u1, l2, u2, u3 in bx:
            d1, d2 = tabs[0][u1] - tabs[0][l1], tabs[1][u2] - tabs[1][l2]
            d1, d2 = np.where(d1 > 0.0, d1, 0.0), np.where(d2 > 0.0, d2, 0.0)
            score = score + ((d1 * d2) * tabs[2][u3])
    score[_bad3(mu, var)] = np.nan
    return score


# ---- the case set ---------------------------------------------------------------------------------------------------------------
def make_front3(P, seed=0):
    """P canonical points on the tilted plane a + b + c = 1.5 inside the unit cube under REF3, hence mutually non-dominated.  For
    P >= 2 two of them are ONE ULP apart in the first objective, for P >= 4 two share a first coordinate exactly, for P >= 6 two
    share a third coordinate exactly; every tied pair differs by 0.01 .. 0.02 in the other two objectives, in opposite directions."""
    rng = np.random.default_rng(3000 + seed + P)
    ab = rng.uniform(0.3, 0.7, (P, 2))
    f = np.concatenate([ab, 1.5 - ab.sum(axis=1, keepdims=True)], axis=1)
    if P >= 2:
        f[1] = [np.nextafter(f[0, 0], np.inf), f[0, 1] - 0.01, f[0, 2] + 0.01]
    if P >= 4:
        f[3] = [f[2, 0], f[2, 1] + 0.02, f[2, 2] - 0.02]
    if P >= 6:
        f[5] = [f[4, 0] + 0.015, f[4, 1] - 0.015, f[4, 2]]
    front, rows = canonical_front3(f, REF3)
    assert len(front) == P and is_canonical3(front, REF3), "make_front3(%d, %d): the draws are not mutually non-dominated" % (P, seed)
    return front


def make_rows3(M, S, seed=0, ref=REF3, extent=1.0):
    """_ehvi_ref.make_rows with a third objective: (mu, var), three arrays S[m] x M each.  Half the rows place Psi(r)'s z by target,
    uniform in [-40, 8], the other half draw mu uniformly around the box; sigma log-uniform in [1e-8, 1e2] x extent; samples scatter
    around the row's (mu, sigma).  A row whose scale T1(r1) T2(r2) T3(r3) would lie between 0 and 1e-290 moves out to z = -60 in
    objective 1, where float64 gives exactly 0 on every side.  With M >= 16 the first rows are the special classes: var == 0 in one
    sample (rows 0, 1, 7), in all (row 2, one of them -0.0), NaN mu (3, 8), NaN var (4), var < 0 (5, 9); row 6 is an ordinary row
    beside them."""
    rng = np.random.default_rng(177 + seed + 131 * M + 17 * S[0] + 5 * S[1] + S[2])
    mu, var = [], []
    for Sm, r in zip(S, ref):
        sig = extent * 10.0 ** rng.uniform(-8.0, 2.0, M)
        zt = rng.uniform(-40.0, 8.0, M)
        m = np.where(np.arange(M) % 2 == 0, r - zt * sig, rng.uniform(r - 3.0 * extent, r + 2.0 * extent, M))
        mu.append(m[None, :] + 0.1 * sig[None, :] * rng.standard_normal((Sm, M)))
        sds = sig[None, :] * np.exp(0.2 * rng.standard_normal((Sm, M)))
        var.append(sds * sds)
    scale = ehvi3_numpy(mu, var, np.zeros((0, 3)), ref)
    for j in np.flatnonzero((scale > 0.0) & (scale < 1e-290)):
        mu[0][:, j] = ref[0] + 60.0 * np.sqrt(var[0][:, j]).max()
    if M >= 16:
        var[0][0, 0] = 0.0
        var[1][S[1] - 1, 1] = 0.0
        var[0][:, 2], var[1][:, 2], var[2][:, 2] = 0.0, 0.0, 0.0
        var[1][0, 2] = -0.0
        mu[0][S[0] - 1, 3] = np.nan
        var[1][0, 4] = np.nan
        var[0][0, 5] = -1e-300
        var[2][0, 7] = 0.0
        mu[2][0, 8] = np.nan
        var[2][S[2] - 1, 9] = -1.0
    return mu, var


# (M, P, S1, S2, S3): M = 1000 is no multiple of either kernel's workgroup and ends inside one; P covers 0, 1, 2, 3, 33 (five cut
# blocks per objective, the last a partial one) and the cap; the sample counts cover 1, mixed small counts, 10 and the cap.
KERNEL_CASES3 = [(1000, 3, 3, 2, 1), (257, 0, 1, 1, 1), (257, 1, 10, 10, 10), (1, 2, 1, 1, 1), (40, 33, 3, 2, 2), (5, PMAX, 2, 1, 1),
                 (70, 2, SMAX, SMAX, SMAX)]
