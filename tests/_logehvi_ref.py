"""References for the log-space expected hypervolume improvement, two and three objectives (b7_logehvi_* / b7_logehvi3_*;
bot7_amd/csrc/ehvi_math.h).  All objectives are minimised.

  logehvi_mp / logehvi3_mp   log of the 50-digit marginals of _ehvi_ref / _ehvi3_ref, per row, as mpf (None: a NaN-class row; a
                             marginal of exactly 0 -- every var == 0 and the point dominated -- is -inf): the yardstick.
  logehvi_numpy / logehvi3_numpy   the library's form restated in numpy float64 from _logei_ref.logei_np: log Psi = log EI with
                             fmin = the cut and xi = 0, ldiff, the running-max log-sum-exp, the same orders.
  scaled_errors              |got - ref| / max(1, |ref|) per row, exact classes (NaN, -inf) checked; BAR (the device) and HOST_BAR
                             (the restatement) are _logei_ref's.
  make_rows_log / make_rows3_log   _ehvi_ref.make_rows / _ehvi3_ref.make_rows3 WITHOUT the move of tiny-scale rows to z = -60 and
                             with z drawn from [-1e4, 8] in a third of the rows; the same special classes.
  far_rows / far_rows3       256 rows whose z is in [-200, -45] in objective 1 at every cut: every linear score is exactly 0."""
import mpmath
import numpy as np

import _ehvi3_ref as R3
import _ehvi_ref as R2
import _logei_ref as LE

BAR, HOST_BAR, DPS = LE.BAR, LE.HOST_BAR, LE.DPS
LN2 = 0.69314718055994530942


# ---- 50 digits ------------------------------------------------------------------------------------------------------------------
def _log_mp(values):
    with mpmath.workdps(DPS):
        return [None if v is None else (mpmath.log(v) if v > 0 else mpmath.mpf("-inf")) for v in values]


def logehvi_mp(mu1, var1, mu2, var2, front, ref):
    return _log_mp(R2.ehvi_mp_values(mu1, var1, mu2, var2, front, ref, dps=DPS))


def logehvi3_mp(mu, var, front, ref):
    return _log_mp([b[0] for b in R3.ehvi3_mp_both(mu, var, front, ref, dps=DPS)])


def scaled_errors(got, ref_mp):
    """Per row |got - ref| / max(1, |ref|), the difference taken in 50 digits.  The classes are exact: NaN where ref is None and
    nowhere else, -inf where ref is -inf and nowhere else, never +inf."""
    got = np.asarray(got, dtype=np.float64)
    assert len(got) == len(ref_mp)
    out = np.zeros(len(got))
    with mpmath.workdps(DPS):
        for j, (g, r) in enumerate(zip(got, ref_mp)):
            if r is None:
                assert np.isnan(g), "row %d: %r where the linear score is NaN" % (j, g)
            elif r == mpmath.mpf("-inf"):
                assert g == -np.inf, "row %d: %r where the marginal is exactly 0" % (j, g)
            else:
                assert np.isfinite(g), "row %d: %r against %s" % (j, g, mpmath.nstr(r, 17))
                out[j] = float(abs(mpmath.mpf(float(g)) - r) / max(mpmath.mpf(1), abs(r)))
    return out


def argmax_mp(ref_mp):
    """(0-based arg-max, relative gap to the runner-up) of a list of mpf without a None in it."""
    with mpmath.workdps(DPS):
        order = sorted(range(len(ref_mp)), key=lambda j: ref_mp[j], reverse=True)
        best, second = ref_mp[order[0]], ref_mp[order[1]]
        return order[0], float((best - second) / abs(best))


# ---- the library's form in float64 ----------------------------------------------------------------------------------------------
def ldiff_np(u, l):
    """log(e^u - e^l): l == -inf: u exactly; !(l < u): -inf; d = l - u: u + log(-expm1(d)) if d > -ln 2, else u + log1p(-exp(d))."""
    u, l = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(l, dtype=np.float64))
    with np.errstate(all="ignore"):
        d = l - u
        out = np.where(d > -LN2, u + np.log(-np.expm1(d)), u + np.log1p(-np.exp(d)))
        out = np.where(l < u, out, -np.inf)
        return np.where(l == -np.inf, u, out)


class Lse(object):
    """The running-max log-sum-exp over terms added in order: (m, acc) = (-inf, 0); a term of -inf is skipped; otherwise
    e = exp(-|t - m|) and (m, acc) = (t, acc e + 1) if t > m, else (m, acc + e).  value: -inf if m == -inf, else m + log(acc)."""

    def __init__(self, M):
        self.m, self.acc = np.full(M, -np.inf), np.zeros(M)

    def add(self, t):
        with np.errstate(all="ignore"):
            t = np.asarray(t, dtype=np.float64)
            skip, up = t == -np.inf, t > self.m
            e = np.exp(np.where(up, self.m - t, t - self.m))
            acc = np.where(up, (self.acc * e) + 1.0, self.acc + e)
            self.acc = np.where(skip, self.acc, acc)
            self.m = np.where(skip | ~up, self.m, t)

    def value(self):
        with np.errstate(all="ignore"):
            return np.where(self.m == -np.inf, -np.inf, self.m + np.log(self.acc))


def _log_psi_np(a, mu, var):
    """b7_logei(mu, var, fmin = a, xi = 0).  var + 0.0 turns -0.0 into +0.0 and changes nothing else: b7_logei tests sigma == 0 before
    it looks at z, where logei_np lets the sign of sqrt(-0.0) decide between log(imprv) and -inf."""
    return LE.logei_np(mu, np.asarray(var, dtype=np.float64) + 0.0, a, 0.0)


def logehvi_numpy(mu1, var1, mu2, var2, front, ref):
    """LSE_k[(LSE_s ldiff(logPsi(a_k+1; s), logPsi(a_k; s)) - log S1) + (LSE_t logPsi(b_k; t) - log S2)], k ascending, s / t
    ascending within it, logPsi(a_k; s) kept from strip to strip."""
    mu1, var1, mu2, var2 = (np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (mu1, var1, mu2, var2))
    av, bv = R2._strips(front, ref)
    S1, S2, M = mu1.shape[0], mu2.shape[0], mu1.shape[1]
    ln1, ln2 = np.log(float(S1)), np.log(float(S2))
    prev = np.full((S1, M), -np.inf)
    score = Lse(M)
    with np.errstate(all="ignore"):
        for a, b in zip(av, bv):
            A, B = Lse(M), Lse(M)
            for s in range(S1):
                p = _log_psi_np(a, mu1[s], var1[s])
                A.add(ldiff_np(p, prev[s]))
                prev[s] = p
            for t in range(S2):
                B.add(_log_psi_np(b, mu2[t], var2[t]))
            score.add((A.value() - ln1) + (B.value() - ln2))
    out = score.value()
    out[R2._bad(mu1, var1, mu2, var2)] = np.nan
    return out


def logehvi3_numpy(mu, var, front, ref):
    """LT_m per distinct cut (s ascending, minus log S_m; LT_m(-inf) = -inf); the boxes in the decomposition's order, per box
    (ldiff(LT1(u1), LT1(l1)) + ldiff(LT2(u2), LT2(l2))) + LT3(u3) folded into the running-max log-sum-exp."""
    mu = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in mu]
    var = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in var]
    M = mu[0].shape[1]
    bx = R3.boxes3(front, ref)
    with np.errstate(all="ignore"):
        tabs = []
        for m, cols in enumerate(((0, 1), (2, 3), (4,))):
            tab = {-np.inf: np.full(M, -np.inf)}
            for c in sorted(set(bx[:, cols].ravel()) - {-np.inf}):
                acc = Lse(M)
                for s in range(mu[m].shape[0]):
                    acc.add(_log_psi_np(c, mu[m][s], var[m][s]))
                tab[c] = acc.value() - np.log(float(mu[m].shape[0]))
            tabs.append(tab)
        score = Lse(M)
        for l1, u1, l2, u2, u3 in bx:
            score.add((ldiff_np(tabs[0][u1], tabs[0][l1]) + ldiff_np(tabs[1][u2], tabs[1][l2])) + tabs[2][u3])
    out = score.value()
    out[R3._bad3(mu, var)] = np.nan
    return out


# ---- the case sets --------------------------------------------------------------------------------------------------------------
def _column(rng, S, M, r, extent):
    """One objective's (mu, var) S x M: rows j % 3 == 0 place Psi(r)'s z uniformly in [-1e4, 8], j % 3 == 1 in [-40, 8], the rest draw
    mu uniformly around the box; sigma log-uniform in [1e-8, 1e2] x extent; samples scatter around the row's (mu, sigma)."""
    sig = extent * 10.0 ** rng.uniform(-8.0, 2.0, M)
    zt = np.where(np.arange(M) % 3 == 0, rng.uniform(-1e4, 8.0, M), rng.uniform(-40.0, 8.0, M))
    mu = np.where(np.arange(M) % 3 == 2, rng.uniform(r - 3.0 * extent, r + 2.0 * extent, M), r - zt * sig)
    mus = mu[None, :] + 0.1 * sig[None, :] * rng.standard_normal((S, M))
    sds = sig[None, :] * np.exp(0.2 * rng.standard_normal((S, M)))
    return mus, sds * sds


def make_rows_log(M, S1, S2, seed=0, ref=R2.REF, extent=1.0):
    """_ehvi_ref.make_rows for the log score: no row is moved out of the deep tail, and a third of the rows reach z = -1e4.  With
    M >= 16 the first rows are the special classes: var == 0 in one sample (rows 0, 1), in all (row 2, one of them -0.0), NaN mu (3),
    NaN var (4), var < 0 (5)."""
    rng = np.random.default_rng(277 + seed + 131 * M + 17 * S1 + S2)
    mu1, var1 = _column(rng, S1, M, ref[0], extent)
    mu2, var2 = _column(rng, S2, M, ref[1], extent)
    if M >= 16:
        var1[0, 0] = 0.0
        var2[S2 - 1, 1] = 0.0
        var1[:, 2], var2[:, 2] = 0.0, 0.0
        var2[0, 2] = -0.0
        mu1[S1 - 1, 3] = np.nan
        var2[0, 4] = np.nan
        var1[0, 5] = -1e-300
    return mu1, var1, mu2, var2


def make_rows3_log(M, S, seed=0, ref=R3.REF3, extent=1.0):
    """_ehvi3_ref.make_rows3 for the log score, as make_rows_log; the special classes are make_rows3's (rows 0 .. 9)."""
    rng = np.random.default_rng(377 + seed + 131 * M + 17 * S[0] + 5 * S[1] + S[2])
    mu, var = [], []
    for Sm, r in zip(S, ref):
        m, v = _column(rng, Sm, M, r, extent)
        mu.append(m)
        var.append(v)
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


# (M, P, S1, S2): _ehvi_ref.KERNEL_CASES without its (257, 2, 11, 1): M = 1000 spans sixteen workgroups and ends inside one; 11 samples
# put one sample in LDS, 32 put twenty-two (78 848 bytes of it: beyond the 64 KiB default); (65, 2, 1, 11) is _ehvi_ref's case with
# objective 1 in registers and one sample of objective 2 in LDS
KERNEL_CASES = [(1000, 2, 3, 2), (257, 0, 1, 1), (257, 1, 10, 10), (1, 2, 1, 1), (40, 33, 3, 2), (5, 256, 11, 1), (70, 1, 32, 32),
                (65, 2, 1, 11)]
KERNEL_CASES3 = R3.KERNEL_CASES3


def _far_column(rng, S, M, r, zlo=-170.0, zhi=-45.0):
    """z(r) uniform in [zlo, zhi], sigma in [0.05, 0.5]: over cuts in [0, r] with r <= 1.125 z stays in [-192.5, -45].  Row 0 sits at
    zlo, so that it is not the arg-max."""
    sig = rng.uniform(0.05, 0.5, M)
    z = rng.uniform(zlo, zhi, M)
    z[0] = zlo
    mus = (r - z * sig)[None, :] + 0.01 * sig[None, :] * rng.standard_normal((S, M))
    sds = sig[None, :] * np.exp(0.05 * rng.standard_normal((S, M)))
    return mus, sds * sds


def _near_column(rng, S, M, r):
    sig = rng.uniform(0.1, 0.5, M)
    mus = rng.uniform(r - 1.5, r + 0.5, M)[None, :] + 0.05 * sig[None, :] * rng.standard_normal((S, M))
    sds = sig[None, :] * np.exp(0.1 * rng.standard_normal((S, M)))
    return mus, sds * sds


def far_rows(M=256, S1=2, S2=2, seed=0):
    """(mu1, var1, mu2, var2, front, ref): objective 1 far beyond ref at every strip, objective 2 ordinary; a front of two points."""
    rng = np.random.default_rng(4000 + seed)
    mu1, var1 = _far_column(rng, S1, M, R2.REF[0])
    mu2, var2 = _near_column(rng, S2, M, R2.REF[1])
    return mu1, var1, mu2, var2, R2.make_front(2), R2.REF


def far_rows3(M=256, S=(2, 1, 1), seed=0):
    """(mu, var, front, ref): objective 1 far beyond ref at every box, objectives 2 and 3 ordinary; a front of three points."""
    rng = np.random.default_rng(5000 + seed)
    cols = [_far_column(rng, S[0], M, R3.REF3[0]), _near_column(rng, S[1], M, R3.REF3[1]), _near_column(rng, S[2], M, R3.REF3[2])]
    return [c[0] for c in cols], [c[1] for c in cols], R3.make_front3(3), R3.REF3
