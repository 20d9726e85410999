"""Host references for tests/test_gpu_pending.py (multi-column fits, pending-point fantasies, append chains): plain numpy,
long double and mpmath; no GPU.  Checked against each other by tests/test_pending_host.py.

  * derived componentwise bars (Higham's gamma_n, valid for any summation order) for alpha = Linv' (Linv r), the posterior mean
    K* alpha and the fantasy covariance K(Xp, Xp) - (K_p Linv')(K_p Linv')', each against the DEVICE's own factor in long double;
  * gp_cov_truth: posterior mean and full P x P covariance at 50 digits (the algebra of _exact.gp_truth), and lapack_cov, the same
    algebra in float64 LAPACK (the yardstick of _exact.gp_bar);
  * fantasy_normals: b7_gp_fantasize's counter layout z(k, s) = counter_normal(seed, k n + s); recover_factor: the factor behind
    a set of draws, L_est = (Y - mu) pinv(Z), with the bound Delta on what rounding can put into it;
  * append_step / append_chain: b7_gp_append restated in float64 numpy, acceptance rule included."""
import math

import mpmath
import numpy as np
from scipy.linalg import lapack, solve_triangular

import _exact as E
import _ts_ref as T

U = 2.0 ** -53
EPS = 2.0 ** -52
K_GAP = 3 * EPS                # tests/test_gpu_numerics.py: device K against host K on grid inputs, entry by entry
DRAW_ULP = 4.0                 # tests/test_gpu_ts.py: the device's counter_normal against _ts_ref.counter_normal (measured 3.00)
NEAR_SINGULAR_FACTOR = 8 * EPS  # tests/test_gpu_numerics.py: the worst recorded residual of the diagonal-block kernel
LD = np.longdouble


def npad(N):
    """context.hip:npad_of with its defaults: one 64-block up to N = 64, multiples of 128 above."""
    return 64 if N <= 64 else 128 * ((N + 127) // 128)


def grid_points(M, d, seed):
    """Candidates / pending points on the grid k 2^-10 of _exact.grid_data (exact squared scaled distances)."""
    return np.ldexp(np.random.default_rng(seed).integers(0, 1024, (M, d)).astype(np.float64), -10)


def multi_data(N, d, c, seed):
    """Observations on the grid (the X of _exact.grid_data's construction) with c response columns: one smooth signal plus
    independent noise per column.  Finite at N = 1 (grid_data's standardisation is not)."""
    rng = np.random.default_rng(seed)
    X = np.ldexp(rng.integers(0, 1024, (N, d)).astype(np.float64), -10)
    y = np.sin(3.0 * X.sum(1)) + 0.3 * np.cos(7.0 * X[:, 0])
    return X, y[:, None] + 0.1 * rng.normal(size=(N, c))


def kernel_fn(kernel="ardse"):
    if kernel == "ardse":
        from oracle import gp
        return gp.ardse
    import _matern_ref
    return _matern_ref.matern52


def host_K(X, h, kernel="ardse"):
    K = kernel_fn(kernel)(X, None, h["lenscale_sq"], h["amp"])
    K[np.diag_indices(len(X))] += h["noise"]
    return K


# ---- the hyper box (tests/test_gpu_numerics.py:_box / _hyps, restated) -------------------------------------------------------------
def box(X, Y):
    d, vy = X.shape[1], float(np.var(Y)) or 1.0
    lo = dict(ls=1e-3 * d, amp=1e-3 * vy, noise=1e-8 * vy, mean=float(np.min(Y)) - 3 * math.sqrt(vy))
    hi = dict(ls=1e3 * d, amp=1e3 * vy, noise=vy, mean=float(np.max(Y)) + 3 * math.sqrt(vy))
    return lo, hi


def box_hyps(X, Y, seed):
    """Two corners of the sampler's box -- bits 3 (lenscale_sq and amp high, noise low: the near-singular one) and 12 (lenscale_sq
    and amp low, noise and mean high) -- and one seeded interior point."""
    lo, hi = box(X, Y)
    d = X.shape[1]
    out = []
    for bits in (3, 12):
        pick = [hi if bits >> i & 1 else lo for i in range(4)]
        out.append({"lenscale_sq": np.full(d, pick[0]["ls"]), "amp": pick[1]["amp"], "noise": pick[2]["noise"],
                    "mean": pick[3]["mean"]})
    u = np.random.default_rng(seed).random(d + 3)
    g = {k: math.exp(math.log(lo[k]) + u[i] * (math.log(hi[k]) - math.log(lo[k]))) for i, k in enumerate(("amp", "noise"))}
    out.append({"lenscale_sq": np.exp(np.log(lo["ls"]) + u[2:2 + d] * (np.log(hi["ls"]) - np.log(lo["ls"]))), "amp": g["amp"],
                "noise": g["noise"], "mean": lo["mean"] + u[-1] * (hi["mean"] - lo["mean"])})
    return out


def k_corners(X, Y):
    """tests/test_gpu_numerics.py:_k_corners: the eight covariance corners, lenscale_sq at the powers of 4 just inside its bounds."""
    lo, hi = box(X, Y)
    d = X.shape[1]
    ls = (4.0 ** math.ceil(math.log(lo["ls"], 4)), 4.0 ** math.floor(math.log(hi["ls"], 4)))
    return [{"lenscale_sq": np.full(d, ls[i & 1]), "amp": (lo, hi)[i >> 1 & 1]["amp"], "noise": (lo, hi)[i >> 2 & 1]["noise"],
             "mean": lo["mean"]} for i in range(8)]


def interior_hyp(d, mean=0.0):
    """The well-conditioned point of section D: lenscale_sq = 0.25 d, amp 1, noise 1e-3.  Only at d = 1 is that a power of 4; at
    d = 2 and 6 the scaled distances round (a few eps of an argument below 2), which the factor's K_GAP term has to carry."""
    return {"lenscale_sq": np.full(d, 0.25 * d), "amp": 1.0, "noise": 1e-3, "mean": mean}


CHAINS = [(3, 64, 2), (65, 128, 6), (129, 256, 6), (257, 300, 1)]     # (n0, N, d): by appends alone from a fit at n0


def chain_hypers(X, Y):
    """Section D's nine hypers: the eight covariance corners, then the interior point."""
    return k_corners(X, Y) + [interior_hyp(X.shape[1])]


def grid_hyp(d, j=-1, amp=1.0, noise=1e-2, mean=0.0):
    """A well-conditioned hyper with lenscale_sq = 4^j in every coordinate (exact distances on the grid), noise = 1e-2 amp."""
    return {"lenscale_sq": np.full(d, 4.0 ** j), "amp": amp, "noise": noise * amp, "mean": mean}


# ---- derived bars against the device's own factor ----------------------------------------------------------------------------------
def alpha_ref_bar(Linv, r, Np):
    """alpha_ref = Linv' (Linv r) in long double and the componentwise bar 2 (Np + 2) u |Linv|' |Linv| |r|: each stage is a sum of
    at most Np products, gamma_(Np+1) <= (Np + 2) u relative to its magnitude sum in ANY order; the first stage's error passes
    through |Linv|', and the second adds its own on |Linv|' |t| <= |Linv|' |Linv| |r|."""
    Ll = np.tril(np.asarray(Linv, dtype=LD))
    rl = np.asarray(r, dtype=LD)
    ref = Ll.T @ (Ll @ rl)
    bar = 2 * (Np + 2) * U * (np.abs(Ll).T @ (np.abs(Ll) @ np.abs(rl)))
    return ref, bar.astype(np.float64)


def mean_ref_bar(Ks, alpha, mean, Np, k_gap=K_GAP):
    """mu_ref = mean + K* alpha in long double on the host's K*, and the bar (Np + 2) u S + k_gap S + u |mu_ref| with S = |K*| |alpha|:
    the dot product in any order, the documented distance between the device's K* and the host's (k_gap: a scalar, or an M x N
    array of per-entry relative gaps), and the final addition's rounding."""
    Kl, al = np.asarray(Ks, dtype=LD), np.asarray(alpha, dtype=LD)
    ref = LD(mean) + Kl @ al
    S = np.abs(Kl) @ np.abs(al)
    Sg = (np.abs(Kl) * np.asarray(k_gap, dtype=LD)) @ np.abs(al) if np.ndim(k_gap) else k_gap * S
    return ref, ((Np + 2) * U * S + Sg + U * np.abs(ref)).astype(np.float64)


def cov_ref_bar(Kp, Kpp, Linv, Np, diag_add=0.0):
    """cov_ref = K(Xp, Xp) - V V' (+ diag_add I), V = K_p Linv', in long double, and 4 (Np + 8) u (E E')_ij + 4 eps |K(Xp, Xp)|_ij
    with E = |K_p| |Linv|': V carries (Np + 2) u E from its own sum and 3 eps E from K_p's entries, so V V' is off by at most
    2 (Np + 8) u E E' from V and (Np + 2) u E E' from the second product (first order); K(Xp, Xp)'s entries carry K_GAP = 3 eps
    and the subtraction one rounding."""
    Kl, Ll = np.asarray(Kp, dtype=LD), np.tril(np.asarray(Linv, dtype=LD))
    V = Kl @ Ll.T
    ref = np.asarray(Kpp, dtype=LD) - V @ V.T
    ref[np.diag_indices(len(ref))] += LD(diag_add)
    Em = np.abs(Kl) @ np.abs(Ll).T
    bar = 4 * (Np + 8) * U * (Em @ Em.T) + 4 * EPS * np.abs(np.asarray(Kpp, dtype=LD))
    return ref, bar.astype(np.float64)


# ---- 50 digits ---------------------------------------------------------------------------------------------------------------------
def gp_cov_truth(X, Y, hyp, Xp, jitter=0.0, dps=50):
    """Posterior mean (P mpf values) and the full P x P latent posterior covariance (mpmath matrix) at the pending points Xp: the
    algebra of _exact.gp_truth, K + (noise + jitter) I, evaluated at dps digits."""
    X, Xp = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(Xp, dtype=np.float64))
    y = np.asarray(Y, dtype=np.float64).reshape(-1)
    N, d = X.shape
    P = Xp.shape[0]
    with mpmath.workdps(dps):
        mpf = mpmath.mpf
        ls = [mpf(float(v)) for v in np.asarray(hyp["lenscale_sq"], dtype=np.float64).ravel()]
        A, m = mpf(float(hyp["amp"])), mpf(float(hyp["mean"]))
        Xm = [[mpf(float(v)) for v in r] for r in X]
        Pm = [[mpf(float(v)) for v in r] for r in Xp]

        def k(a, b):
            return A * mpmath.exp(-sum((a[i] - b[i]) ** 2 / ls[i] for i in range(d)) / 2)

        K = mpmath.matrix(N, N)
        for i in range(N):
            for j in range(i + 1):
                K[i, j] = K[j, i] = k(Xm[i], Xm[j])
            K[i, i] += mpf(float(hyp["noise"])) + mpf(float(jitter))
        L = mpmath.cholesky(K)
        r = mpmath.matrix([mpf(float(v)) - m for v in y])
        alpha = E._bwd(L, E._fwd(L, r))
        ks = [mpmath.matrix([k(Pm[p], Xm[i]) for i in range(N)]) for p in range(P)]
        V = [E._fwd(L, ks[p]) for p in range(P)]
        mu = [m + mpmath.fsum(ks[p][i] * alpha[i] for i in range(N)) for p in range(P)]
        cov = mpmath.matrix(P, P)
        for p in range(P):
            for q in range(p + 1):
                cov[p, q] = cov[q, p] = k(Pm[p], Pm[q]) - mpmath.fsum(V[p][i] * V[q][i] for i in range(N))
        return mu, cov


def lapack_cov(X, Y, hyp, Xp, jitter=0.0, kscale=1.0):
    """The same algebra in float64 LAPACK on the host's K (kscale: off-diagonal covariances multiplied by it, as
    _exact.lapack_fit does): (mu, cov), None if dpotrf fails."""
    from oracle import gp
    X, Xp = np.asarray(X, dtype=np.float64), np.atleast_2d(np.asarray(Xp, dtype=np.float64))
    K = gp.ardse(X, None, hyp["lenscale_sq"], hyp["amp"])
    if kscale != 1.0:
        K *= kscale
        K[np.diag_indices(len(X))] /= kscale
    K[np.diag_indices(len(X))] += hyp["noise"] + jitter
    L, info = lapack.dpotrf(K, lower=1, clean=1)
    if info != 0:
        return None
    r = np.asarray(Y, dtype=np.float64).reshape(-1, 1) - hyp["mean"]
    alpha = solve_triangular(L, solve_triangular(L, r, lower=True), lower=True, trans="T")
    Ks = gp.ardse(Xp, X, hyp["lenscale_sq"], hyp["amp"]) * kscale
    V = solve_triangular(L, Ks.T, lower=True)
    return hyp["mean"] + (Ks @ alpha)[:, 0], gp.ardse(Xp, None, hyp["lenscale_sq"], hyp["amp"]) - V.T @ V


def mp_flat(M):
    return [M[i, j] for i in range(M.rows) for j in range(M.cols)]


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
def fantasy_normals(seed, P, n):
    """Z (P x n) of b7_gp_fantasize: z(k, s) = counter_normal(seed, k n + s), the RAW seed (mod 2^64) as the generator's key."""
    ctr = np.arange(P, dtype=np.uint64)[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]
    return T.counter_normal(np.uint64(int(seed) & (2 ** 64 - 1)), ctr)


def recover_factor(Y, mu, Z):
    """L_est = (Y - mu 1') pinv(Z) by least squares (P x P), and Delta, the Frobenius bound on what rounding puts into it:
    row i of Y is mu_i + sum_k L_ik z_ks with z off by DRAW_ULP (4 ulp = 4 eps relative), P products and P additions in order
    ((P + 1) u on the magnitude sum, mu included); the residual of the solve is that perturbation times ||pinv(Z)||_2, and the
    factor 2 covers the first-order terms dropped and lstsq's own backward error (cond(Z) < 4 at n = 4 P)."""
    Y, mu, Z = np.asarray(Y, dtype=np.float64), np.asarray(mu, dtype=np.float64).ravel(), np.asarray(Z, dtype=np.float64)
    P = Y.shape[0]
    Lt, _, rank, sv = np.linalg.lstsq(Z.T, (Y - mu[:, None]).T, rcond=None)
    L_est = Lt.T
    pert = (DRAW_ULP * EPS + (P + 1) * U) * (np.abs(L_est) @ np.abs(Z)) + (P + 1) * U * np.abs(mu)[:, None] * np.ones_like(Z)
    delta = 2.0 / sv.min() * float(np.linalg.norm(pert))
    return L_est, delta, float(sv.max() / sv.min())


def fantasy_schedule(eps=1e-8, growth=1.1):
    """b7_gp_fantasize's jitter attempts: the schedule of utils.math.chol without its Frobenius cap (the loop gives up after 4000
    attempts instead): _exact.jitter_schedule capped where the doubles end."""
    return E.jitter_schedule(1e300, eps=eps, growth=growth)[:4001]


def match_schedule(j, eps=1e-8, growth=1.1, rtol=1e-3):
    """Index of the schedule value that j equals to rtol (steps are 10 % apart), or None."""
    s = np.array(fantasy_schedule(eps, growth))
    i = int(np.argmin(np.abs(s - j)))
    return i if abs(s[i] - j) <= rtol * s[i] else None


def jitter_cases():
    """The two constructions of C.3 on grid inputs (N = 8, d = 2, lenscale_sq = 4^-2, amp 1, noise 0): (a) P = 8 pending rows, rows
    4 .. 7 bit-equal to rows 3 .. 0 (so X_pend[P - 1] = X_pend[0]); (b) P = 6 pending rows of which four are bit-equal to
    observations.  In exact arithmetic both covariances are singular."""
    X, Y = E.grid_data(8, 2, seed=8)
    h = dict(grid_hyp(2, j=-2), noise=0.0)
    A = grid_points(4, 2, seed=21)
    Bp = grid_points(2, 2, seed=22)
    return [("duplicate pending rows", X, Y, h, np.concatenate([A, A[::-1]])),
            ("pending rows equal to observations", X, Y, h, np.concatenate([Bp, X[[1, 3, 4, 6]]]))]


def matern_gap(X, Z, lenscale_sq):
    """Per-entry relative distance between the device's Matern K and the host's: each is within (4 + s) ulp of the truth
    (_matern_ref.within_matern_bar's constants), s = sqrt(5 D)."""
    from oracle import gp
    return (8.0 + 2.0 * np.sqrt(5.0 * gp.pdist(X, Z, lenscale_sq))) * EPS


# ---- long double refit -------------------------------------------------------------------------------------------------------------
def ld_cholesky(K):
    A = np.array(K, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    return L


def ld_solve_lower(L, B):
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def ld_posterior(K, Ks, r, mean, amp):
    """(mu M x c, var M) of a refit in long double on the given K (noise on its diagonal) and K*."""
    L = ld_cholesky(K)
    V = ld_solve_lower(L, np.asarray(Ks, dtype=LD).T)
    t = ld_solve_lower(L, np.asarray(r, dtype=LD))
    return LD(mean) + V.T @ t, LD(amp) - np.einsum("ij,ij->j", V, V)


# ---- the append chain --------------------------------------------------------------------------------------------------------------
def append_step(Linv, k, kappa):
    """One b7_gp_append in float64 numpy on the n x n inverse factor: l = Linv k, e = |Linv| |k|, l2 = kappa - l'l; refused iff
    !(l2 > 2 g sum |l_i| e_i + g l'l) with g = (n + 2) u.  Returns (accepted, l, lam, new inverse row, l2, tol)."""
    n = Linv.shape[0]
    l = Linv @ k
    e = np.abs(Linv) @ np.abs(k)
    ll = float(l @ l)
    l2 = kappa - ll
    g = (n + 2) * U
    tol = 2.0 * g * float(np.abs(l) @ e) + g * ll
    if not l2 > tol:
        return False, l, 0.0, None, l2, tol
    lam = math.sqrt(l2)
    return True, l, lam, -(Linv.T @ l) / lam, l2, tol


def append_chain(K, n0, n1=None):
    """From LAPACK's factor of K[:n0, :n0] (K carries its noise on the diagonal), append rows n0 .. n1 - 1 one at a time.  Returns
    (L, Linv, n_end, steps): the factors at the size reached and per step (n, accepted, l2, tol); the chain stops at its first
    refusal.  None if dpotrf fails at n0."""
    K = np.asarray(K, dtype=np.float64)
    n1 = K.shape[0] if n1 is None else n1
    L0, info = lapack.dpotrf(K[:n0, :n0].copy(), lower=1, clean=1)
    if info != 0:
        return None
    L = np.zeros((n1, n1))
    Li = np.zeros((n1, n1))
    L[:n0, :n0] = L0
    Li[:n0, :n0] = solve_triangular(L0, np.eye(n0), lower=True)
    steps, n = [], n0
    while n < n1:
        ok, l, lam, row, l2, tol = append_step(Li[:n, :n], K[n, :n], K[n, n])
        steps.append((n, ok, l2, tol))
        if not ok:
            break
        L[n, :n], L[n, n] = l, lam
        Li[n, :n], Li[n, n] = row, 1.0 / lam
        n += 1
    return L[:n, :n], Li[:n, :n], n, steps


def lapack_factors(K):
    """(L, Linv) by dpotrf and a triangular solve; None where dpotrf fails."""
    L, info = lapack.dpotrf(np.array(K, dtype=np.float64), lower=1, clean=1)
    if info != 0:
        return None
    return L, solve_triangular(L, np.eye(len(L)), lower=True)


def chain_yardstick(K, n0, n_end=None):
    """The yardstick of section D at size n_end: the larger of LAPACK's and the restated chain's backward errors on the same K.
    Returns ((factor, inverse), restated, lapack); lapack is None where dpotrf fails, restated None where its chain stopped short."""
    n_end = K.shape[0] if n_end is None else n_end
    Kn = K[:n_end, :n_end]
    ch = append_chain(K, n0, n_end)
    rs = E.backward_errors(Kn, ch[0], ch[1]) if ch is not None and ch[2] == n_end else None
    lf = lapack_factors(Kn)
    la = E.backward_errors(Kn, lf[0], lf[1]) if lf is not None else None
    both = [v for v in (rs, la) if v is not None]
    if not both:
        return None, rs, la
    return (max(v[0] for v in both), max(v[1] for v in both)), rs, la
