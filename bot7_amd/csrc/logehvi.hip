// Log-space expected hypervolume improvement for two and three objectives: log of ehvi.hip's / ehvi3.hip's marginal score, evaluated
// so that it never underflows -- the multi-objective twin of LogEI (Ament et al., "Unexpected Improvements to Expected Improvement",
// NeurIPS 2023).  No counterpart in the reference's scores/.  All objectives are minimised.  The linear scores are exactly 0 wherever
// a Psi has z < -37.5 in every strip or box (a reference point no observation has reached, late trials, most of a large grid), and
// score:max(1) then nominates row 1; this score still ranks those rows.
//
// Arithmetic (the same text in bot7hip.h and in tests/_logehvi_ref.py's numpy restatement):
//   logPsi(a; mu, var) = b7_logei(mu, var, fmin = a, xi = 0)           logei_math.h: its three branches, its edge cases; a = -inf: -inf
//   ldiff(u, l) = log(e^u - e^l):   l == -inf: u exactly;   !(l < u): -inf (the linear code's clamp at 0);
//                                   d = l - u:  u + log(-expm1(d)) if d > -ln 2, else u + log1p(-exp(d))
//   LSE over terms t_1 .. t_n in a fixed order, RUNNING-MAX form: (m, acc) = (-inf, 0); a term t == -inf is skipped; otherwise
//                                   e = exp(-|t - m|) and (m, acc) = (t, acc e + 1) if t > m, else (m, acc + e);
//                                   the value is -inf if m == -inf, else m + log(acc).  One exp per term, one log at the end; an empty
//                                   sum is -inf, a single term comes back exactly (acc = 1), and the error does not grow with |value|.
//   two objectives, strips as in ehvi.hip (a_0 = -inf, a_P+1 = r1, b_0 = r2):
//     log score = LSE_k[(LSE_s ldiff(logPsi(a_k+1; s), logPsi(a_k; s)) - log S1) + (LSE_t logPsi(b_k; t) - log S2)]
//     k ascending, s / t ascending within it; logPsi(a_k+1; s) is evaluated once and kept as strip k + 1's logPsi(a_k; s).
//   three objectives, boxes of b7_nondominated_boxes3 in its order, LT_m(c) = LSE_s logPsi(c; s) - log S_m, LT_m(-inf) = -inf:
//     log score = LSE_b[(ldiff(LT1(u1), LT1(l1)) + ldiff(LT2(u2), LT2(l2))) + LT3(u3)]
// log S is ocml's log of the sample count (S = 1: exactly 0).  Contraction off; erfc, erfcx, exp, expm1, log, log1p are ocml's.
// Thin strips need no special care: a strip's cancellation error is a few eps |log Psi| of Psi1(a_k+1) B_k, and the total is at least
// that product because the strips below it have the larger B (three objectives: the non-dominated region is down-closed).
// Row classes: NaN exactly where the linear score is NaN -- any mu or var NaN, any var < 0, in any objective.  Otherwise, for finite
// input, never NaN and never +inf; -inf is a legal value (every var == 0 and the point dominated).
//
// logehvi_kernel: ehvi_kernel's layout.  One candidate per lane, one wave per workgroup; the front and ref through wave-uniform
// (scalar) loads; per sample (mu, sigma = sqrt(var), log sigma) taken once, ahead of the strip loop; the first B7_EHVI_SREG samples
// of each objective and the running logPsi(a_k; s) in registers, the rest in the lane's own LDS columns ([sample][lane]: no bank
// conflict, no barrier), (4 x1 + 3 x2) 512 bytes for x1 / x2 samples beyond the registers, 78 848 at most (above 64 KiB: opted in).
// logehvi3_table_kernel / logehvi3_box_kernel: ehvi3.hip's layout, chunking (chunk3) and table buffer.  The table kernel keeps
// a running (m, acc) pair per cut; the box kernel keeps four boxes' table reads in flight and folds the boxes in their order.  A row's
// bits do not depend on the chunking: every work item sees one candidate only.
//
// The nominations write the marginal log score into the first context's accumulator as a LOG accumulator (score.hip's acc_* state),
// so b7_score_finish(1) downloads it and b7_feas_add_acc takes it: constrained multi-objective nomination is b7_feas_reset,
// b7_feas_add / b7_feas_add_acc, b7_feas_nominate.
//
// Out of scope, as for the linear scores: four or more objectives, correlated objectives / multi-task GPs, batches, refinement,
// sharded grids and groups, the Bayesian-linear head, trust regions with three objectives, the bot's config.bot.constraints combined
// with objectives.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"
#include "logei_math.h"

namespace {

constexpr int SR = B7_EHVI_SREG;
constexpr int LOGEHVI_LANES = 64;
constexpr int LOGEHVI3_LANES = 64;      // == ehvi3.hip's: chunk3 cuts the candidates into whole waves of this size
constexpr int LOGEHVI3_BOX_LANES = 64;
constexpr int LOGEHVI3_CB = 8;          // cuts per work item of the table kernel

__device__ __forceinline__ double log_psi(double a, double m, double sd, double lsd) { return b7_logei_core<true>(m, sd, lsd, a, 0.0); }

// log(e^u - e^l) (the header)
__device__ __forceinline__ double ldiff(double u, double l) {
  if (l == -INFINITY) return u;
  if (!(l < u)) return -INFINITY;
  const double d = l - u;
  return d > -0.69314718055994530942 ? u + log(-expm1(d)) : u + log1p(-exp(d));
}

// the running-max log-sum-exp (the header)
struct Lse {
  double m = -INFINITY, acc = 0.0;
  __device__ __forceinline__ void add(double t) {
    if (t == -INFINITY) return;
    const bool up = t > m;
    const double e = exp(up ? m - t : t - m);
    acc = up ? (acc * e) + 1.0 : acc + e;
    m = up ? t : m;
  }
  __device__ __forceinline__ double value() const { return m == -INFINITY ? -INFINITY : m + log(acc); }
};

struct LogEhviArgs {
  const double *mu1, *var1, *mu2, *var2;  // [S1][M], [S2][M]
  const double *av, *bv;                  // [P + 1]: a_1 .. a_P, r1 | r2, b_1 .. b_P
  long long M;
  int S1, S2, P;
  double *out;                            // [M]
};

__global__ void __launch_bounds__(LOGEHVI_LANES) logehvi_kernel(LogEhviArgs g) {
  extern __shared__ double sh[];
  const long long j = (long long)blockIdx.x * LOGEHVI_LANES + threadIdx.x;
  if (j >= g.M) return;
  const int x1 = g.S1 > SR ? g.S1 - SR : 0, x2 = g.S2 > SR ? g.S2 - SR : 0;
  // sample i of the lane at [i * 64]: objective 1's mu, sigma, log sigma, running logPsi; objective 2's mu, sigma, log sigma
  double *lm1 = sh + threadIdx.x, *ls1 = lm1 + x1 * LOGEHVI_LANES, *ll1 = ls1 + x1 * LOGEHVI_LANES, *lp1 = ll1 + x1 * LOGEHVI_LANES;
  double *lm2 = lp1 + x1 * LOGEHVI_LANES, *ls2 = lm2 + x2 * LOGEHVI_LANES, *ll2 = ls2 + x2 * LOGEHVI_LANES;
  double m1[SR], s1[SR], l1[SR], p1[SR], m2[SR], s2[SR], l2[SR];
  bool bad = false;
#pragma unroll
  for (int s = 0; s < SR; ++s)
    if (s < g.S1) {
      const double m = g.mu1[(long long)s * g.M + j], v = g.var1[(long long)s * g.M + j];
      bad = bad || !(v >= 0.0) || m != m;
      const double sd = sqrt(v);
      m1[s] = m, s1[s] = sd, l1[s] = log(sd), p1[s] = -INFINITY;
    }
  for (int s = SR; s < g.S1; ++s) {
    const double m = g.mu1[(long long)s * g.M + j], v = g.var1[(long long)s * g.M + j];
    bad = bad || !(v >= 0.0) || m != m;
    const double sd = sqrt(v);
    lm1[(s - SR) * LOGEHVI_LANES] = m, ls1[(s - SR) * LOGEHVI_LANES] = sd, ll1[(s - SR) * LOGEHVI_LANES] = log(sd);
    lp1[(s - SR) * LOGEHVI_LANES] = -INFINITY;
  }
#pragma unroll
  for (int t = 0; t < SR; ++t)
    if (t < g.S2) {
      const double m = g.mu2[(long long)t * g.M + j], v = g.var2[(long long)t * g.M + j];
      bad = bad || !(v >= 0.0) || m != m;
      const double sd = sqrt(v);
      m2[t] = m, s2[t] = sd, l2[t] = log(sd);
    }
  for (int t = SR; t < g.S2; ++t) {
    const double m = g.mu2[(long long)t * g.M + j], v = g.var2[(long long)t * g.M + j];
    bad = bad || !(v >= 0.0) || m != m;
    const double sd = sqrt(v);
    lm2[(t - SR) * LOGEHVI_LANES] = m, ls2[(t - SR) * LOGEHVI_LANES] = sd, ll2[(t - SR) * LOGEHVI_LANES] = log(sd);
  }
  if (bad) {
    g.out[j] = NAN;
    return;
  }
  const double ln1 = log((double)g.S1), ln2 = log((double)g.S2);
  Lse score;
  for (int k = 0; k <= g.P; ++k) {
    const double a = g.av[k], b = g.bv[k];
    Lse A, B;
#pragma unroll
    for (int s = 0; s < SR; ++s)
      if (s < g.S1) {
        const double p = log_psi(a, m1[s], s1[s], l1[s]);
        A.add(ldiff(p, p1[s]));
        p1[s] = p;
      }
    for (int s = 0; s < x1; ++s) {
      const double p = log_psi(a, lm1[s * LOGEHVI_LANES], ls1[s * LOGEHVI_LANES], ll1[s * LOGEHVI_LANES]);
      A.add(ldiff(p, lp1[s * LOGEHVI_LANES]));
      lp1[s * LOGEHVI_LANES] = p;
    }
#pragma unroll
    for (int t = 0; t < SR; ++t)
      if (t < g.S2) B.add(log_psi(b, m2[t], s2[t], l2[t]));
    for (int t = 0; t < x2; ++t) B.add(log_psi(b, lm2[t * LOGEHVI_LANES], ls2[t * LOGEHVI_LANES], ll2[t * LOGEHVI_LANES]));
    score.add((A.value() - ln1) + (B.value() - ln2));
  }
  g.out[j] = score.value();
}

size_t logehvi_lds_bytes(int S1, int S2) {
  const int x1 = S1 > SR ? S1 - SR : 0, x2 = S2 > SR ? S2 - SR : 0;
  return sizeof(double) * LOGEHVI_LANES * (size_t)(4 * x1 + 3 * x2);
}

// the log score of M rows onto out (device), on c's stream; the front staged by front_stage
int launch_logehvi(b7_ctx *c, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2, int P, int64_t M,
                   double *out) {
  PhaseScope ps(c, "logehvi");
  LogEhviArgs g;
  g.mu1 = mu1, g.var1 = var1, g.mu2 = mu2, g.var2 = var2;
  g.av = (const double *)c->ehvi_front.p, g.bv = g.av + (P + 1);
  g.M = (long long)M, g.S1 = S1, g.S2 = S2, g.P = P, g.out = out;
  const int64_t nb = (M + LOGEHVI_LANES - 1) / LOGEHVI_LANES;
  if (nb > 0x7fffffffLL) return b7_fail(c, B7_ERR_INVALID, "logehvi: %lld rows are more than one launch takes", (long long)M);
  const size_t lds = logehvi_lds_bytes(S1, S2);
  // dynamic LDS above the 64 KiB default needs an explicit opt-in, per device (gfx950 has 160 KiB per workgroup)
  if (lds > (size_t)(64 << 10))
    B7_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(logehvi_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(logehvi_kernel, dim3((unsigned)nb), dim3(LOGEHVI_LANES), lds, c->stream, g);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// ---- three objectives: ehvi3.hip's two kernels in log space ----
struct LogEhvi3TableArgs {
  const double *mu[3], *var[3];  // [S_m][ld], already moved to the chunk's first candidate
  long long ld;                  // candidates of the whole posterior
  const double *cuts;            // cuts of objective 0 | 1 | 2, each ascending and distinct, r_m last
  int S[3], ncut[3];
  double *T;                     // [rows][C]: LT
  int *flag;                     // [3][C]: the objective's row class (1: NaN)
  long long C, n;                // the table's row stride, the candidates of this chunk (n <= C)
};

__global__ void __launch_bounds__(LOGEHVI3_LANES) logehvi3_table_kernel(LogEhvi3TableArgs g) {
  const long long j = (long long)blockIdx.x * LOGEHVI3_LANES + threadIdx.x;
  if (j >= g.n) return;
  // blockIdx.y -> (objective, first cut): wave-uniform
  const int nb0 = (g.ncut[0] + LOGEHVI3_CB - 1) / LOGEHVI3_CB, nb1 = (g.ncut[1] + LOGEHVI3_CB - 1) / LOGEHVI3_CB;
  int y = (int)blockIdx.y, m = 0, cut0 = 0, row0 = 0;
  if (y >= nb0 + nb1) m = 2, y -= nb0 + nb1, cut0 = g.ncut[0] + g.ncut[1], row0 = g.ncut[0] + g.ncut[1] + 2;
  else if (y >= nb0) m = 1, y -= nb0, cut0 = g.ncut[0], row0 = g.ncut[0] + 1;
  const int k0 = y * LOGEHVI3_CB, nk = g.ncut[m] - k0;  // this item's cuts: k0 .. k0 + min(nk, CB) - 1
  const double *mu = g.mu[m], *var = g.var[m];
  const int S = g.S[m];
  double cv[LOGEHVI3_CB];
  Lse acc[LOGEHVI3_CB];
#pragma unroll
  for (int k = 0; k < LOGEHVI3_CB; ++k) cv[k] = k < nk ? g.cuts[cut0 + k0 + k] : 0.0;
  bool bad = false;
  for (int s = 0; s < S; ++s) {
    const double mm = mu[(long long)s * g.ld + j], v = var[(long long)s * g.ld + j];
    bad = bad || !(v >= 0.0) || mm != mm;
    const double sd = sqrt(v), lsd = log(sd);
#pragma unroll
    for (int k = 0; k < LOGEHVI3_CB; ++k)
      if (k < nk) acc[k].add(log_psi(cv[k], mm, sd, lsd));
  }
  const double ln = log((double)S);
  double *Trow = g.T + (long long)(row0 + 1 + k0) * g.C + j;  // row0: the objective's zero row
#pragma unroll
  for (int k = 0; k < LOGEHVI3_CB; ++k)
    if (k < nk) Trow[(long long)k * g.C] = acc[k].value() - ln;
  if (y == 0) {
    g.T[(long long)row0 * g.C + j] = -INFINITY;
    g.flag[(long long)m * g.C + j] = bad ? 1 : 0;
  }
}

struct LogEhvi3BoxArgs {
  const double *T;
  const int *flag;
  const int *box;  // [B][5]: the table rows of l1, u1, l2, u2, u3
  int B;
  long long C, n;
  double *out;     // [n]
};

__global__ void __launch_bounds__(LOGEHVI3_BOX_LANES) logehvi3_box_kernel(LogEhvi3BoxArgs g) {
  const long long j = (long long)blockIdx.x * LOGEHVI3_BOX_LANES + threadIdx.x;
  if (j >= g.n) return;
  if ((g.flag[j] | g.flag[g.C + j] | g.flag[2 * g.C + j]) != 0) {
    g.out[j] = NAN;
    return;
  }
  const double *T = g.T + j;
  Lse score;
  // four boxes' reads in flight, as in ehvi3_box_kernel; the fold stays in box order
#pragma unroll 4
  for (int b = 0; b < g.B; ++b) {
    const int *q = g.box + 5 * b;
    const double l1 = T[(long long)q[0] * g.C], u1 = T[(long long)q[1] * g.C], l2 = T[(long long)q[2] * g.C], u2 = T[(long long)q[3] * g.C];
    const double u3 = T[(long long)q[4] * g.C];
    score.add((ldiff(u1, l1) + ldiff(u2, l2)) + u3);
  }
  g.out[j] = score.value();
}

// the log score of M rows onto out (device), on c's stream: launch_ehvi3 (ehvi3.hip) with the log kernels, the same staging buffers
int launch_logehvi3(b7_ctx *c, const double *const *mu, const double *const *var, const int *S, const Staged3 &st, int64_t M, double *out) {
  if (M > 0x7fffffffLL * LOGEHVI3_LANES) return b7_fail(c, B7_ERR_INVALID, "logehvi3: %lld rows are more than one launch takes", (long long)M);
  // what the kernels index by: every box row inside the table, the box and cut counts inside their staging
  for (int r : st.box)
    if (r < 0 || r >= st.rows) return b7_fail(c, B7_ERR_INVALID, "logehvi3: a box edge is none of the cuts (row %d of %d)", r, st.rows);
  if (st.B > EHVI3_BOXES_MAX || st.rows > 3 * (B7_EHVI3_PMAX + 2))
    return b7_fail(c, B7_ERR_INVALID, "logehvi3: %d boxes over %d table rows are more than a front of %d points gives", st.B, st.rows, B7_EHVI3_PMAX);
  const size_t cut_bytes = sizeof(double) * (size_t)(3 * (B7_EHVI3_PMAX + 1));
  B7_TRY(b7_ensure(c, c->ehvi3_front, cut_bytes + sizeof(int) * 5 * (size_t)EHVI3_BOXES_MAX));
  double *cuts_d = (double *)c->ehvi3_front.p;
  int *box_d = (int *)((char *)c->ehvi3_front.p + cut_bytes);
  B7_HIP(c, hipMemcpyAsync(cuts_d, st.cuts.data(), sizeof(double) * st.cuts.size(), hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(box_d, st.box.data(), sizeof(int) * st.box.size(), hipMemcpyHostToDevice, c->stream));
  const int64_t C = chunk3(c, st.rows, M);
  const size_t tab_bytes = sizeof(double) * (size_t)st.rows * (size_t)C;
  B7_TRY(b7_ensure(c, c->ehvi3_table, tab_bytes + sizeof(int) * 3 * (size_t)C));
  int nblk = 0;
  for (int m = 0; m < 3; ++m) nblk += (st.ncut[m] + LOGEHVI3_CB - 1) / LOGEHVI3_CB;
  for (int64_t j0 = 0; j0 < M; j0 += C) {
    const int64_t n = std::min<int64_t>(C, M - j0);
    LogEhvi3TableArgs t;
    for (int m = 0; m < 3; ++m) t.mu[m] = mu[m] + j0, t.var[m] = var[m] + j0, t.S[m] = S[m], t.ncut[m] = st.ncut[m];
    t.ld = (long long)M, t.cuts = cuts_d;
    t.T = (double *)c->ehvi3_table.p, t.flag = (int *)((char *)c->ehvi3_table.p + tab_bytes);
    t.C = (long long)C, t.n = (long long)n;
    {
      PhaseScope ps(c, "logehvi3_tab");
      hipLaunchKernelGGL(logehvi3_table_kernel, dim3((unsigned)((n + LOGEHVI3_LANES - 1) / LOGEHVI3_LANES), (unsigned)nblk), dim3(LOGEHVI3_LANES), 0,
                         c->stream, t);
      B7_HIP(c, hipGetLastError());
    }
    LogEhvi3BoxArgs b;
    b.T = t.T, b.flag = t.flag, b.box = box_d, b.B = st.B, b.C = t.C, b.n = t.n, b.out = out + j0;
    {
      PhaseScope ps(c, "logehvi3_box");
      hipLaunchKernelGGL(logehvi3_box_kernel, dim3((unsigned)((n + LOGEHVI3_BOX_LANES - 1) / LOGEHVI3_BOX_LANES)), dim3(LOGEHVI3_BOX_LANES), 0,
                         c->stream, b);
      B7_HIP(c, hipGetLastError());
    }
  }
  return B7_OK;
}

}  // namespace

extern "C" {

int b7_logehvi_compute(b7_ctx *c, const double *mu1, const double *var1, int S1, const double *mu2, const double *var2, int S2,
                       const double *front, int P, const double *ref, int64_t M, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (M < 0 || (M > 0 && (!mu1 || !var1 || !mu2 || !var2 || !out))) return b7_fail(c, B7_ERR_INVALID, "logehvi_compute: bad arguments (M >= 0, arrays required)");
  B7_TRY(samples_refuse(c, "logehvi_compute", S1, S2));
  B7_TRY(front_refuse(c, "logehvi_compute", front, P, ref));
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t m = (size_t)M, n1 = (size_t)S1 * m, n2 = (size_t)S2 * m;
  B7_TRY(b7_ensure(c, c->ehvi_user, sizeof(double) * (2 * n1 + 2 * n2 + m)));  // b7_ehvi_compute's staging: the kept posterior stays
  double *d1 = (double *)c->ehvi_user.p, *v1 = d1 + n1, *d2 = v1 + n1, *v2 = d2 + n2, *od = v2 + n2;
  std::vector<double> fh;
  B7_TRY(front_stage(c, front, P, ref, &fh));
  B7_HIP(c, hipMemcpyAsync(d1, mu1, sizeof(double) * n1, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(v1, var1, sizeof(double) * n1, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(d2, mu2, sizeof(double) * n2, hipMemcpyHostToDevice, c->stream));
  B7_HIP(c, hipMemcpyAsync(v2, var2, sizeof(double) * n2, hipMemcpyHostToDevice, c->stream));
  B7_TRY(launch_logehvi(c, d1, v1, S1, d2, v2, S2, P, M, od));
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staged front are consumed
  return B7_OK;
}

int b7_logehvi_nominate(b7_ctx *c, b7_ctx *other, const double *front, int P, const double *ref, double *best_val, int64_t *best_idx1) {
  if (!c) return B7_ERR_INVALID;
  if (!other) return b7_fail(c, B7_ERR_INVALID, "logehvi_nominate: the second objective's context is NULL");
  if (!best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "logehvi_nominate: NULL argument (best_val and best_idx1 are needed)");
  if (c->group || other->group)
    return b7_fail(c, B7_ERR_STATE, "logehvi_nominate: a context belongs to a group (two objectives over a sharded grid are not built)");
  if (other->device != c->device)
    return b7_fail(c, B7_ERR_UNSUPPORTED, "logehvi_nominate: the second objective's context is on device %d, this one on device %d (a posterior across devices is not built)", other->device, c->device);
  if (!c->post_valid)
    return b7_fail(c, B7_ERR_STATE, "logehvi_nominate: no kept posterior of the first objective (call b7_eval_posterior; a change of the grid or the data forgets it)");
  if (!other->post_valid)
    return b7_fail(c, B7_ERR_STATE, "logehvi_nominate: no kept posterior of the second objective (call b7_eval_posterior on its context; a change of the grid or the data forgets it)");
  if (other->post_M != c->post_M)
    return b7_fail(c, B7_ERR_INVALID, "logehvi_nominate: the second objective's grid has %lld rows, this one %lld", (long long)other->post_M, (long long)c->post_M);
  B7_TRY(samples_refuse(c, "logehvi_nominate", c->post_S, other->post_S));
  B7_TRY(front_refuse(c, "logehvi_nominate", front, P, ref));
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->post_M;  // == c->M: a grid change would have forgotten the posterior
  const size_t SM1 = (size_t)c->post_S * (size_t)M, SM2 = (size_t)other->post_S * (size_t)M;
  const double *mu1 = (const double *)c->post.p, *mu2 = (const double *)other->post.p;
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)M));
  std::vector<double> fh;
  B7_TRY(front_stage(c, front, P, ref, &fh));
  // the two streams are ordered by events both ways, as b7_ehvi_nominate orders them (its events)
  if (other != c) {
    for (hipEvent_t &e : c->ev_ehvi)
      if (!e) B7_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    B7_HIP(c, hipEventRecord(c->ev_ehvi[0], other->stream));
    B7_HIP(c, hipStreamWaitEvent(c->stream, c->ev_ehvi[0], 0));
  }
  acc_declare_log_written(c);  // the kernel writes every row of it
  B7_TRY(launch_logehvi(c, mu1, mu1 + SM1, c->post_S, mu2, mu2 + SM2, other->post_S, P, M, (double *)c->acc.p));
  if (other != c) {
    B7_HIP(c, hipEventRecord(c->ev_ehvi[1], c->stream));
    B7_HIP(c, hipStreamWaitEvent(other->stream, c->ev_ehvi[1], 0));
  }
  // score:max(1) of the log accumulator, the divisor 1 (log 1 == 0 is subtracted); waits, so the staged front is consumed
  return launch_finish(c, (double *)c->acc.p, M, 1.0, best_val, best_idx1, true);
}

int b7_logehvi3_compute(b7_ctx *c, const double *const *mu, const double *const *var, const int *S, const double *front, int P, const double *ref,
                        int64_t M, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (!mu || !var || !S) return b7_fail(c, B7_ERR_INVALID, "logehvi3_compute: NULL argument (mu, var and S of three objectives are needed)");
  if (M < 0 || (M > 0 && (!mu[0] || !var[0] || !mu[1] || !var[1] || !mu[2] || !var[2] || !out)))
    return b7_fail(c, B7_ERR_INVALID, "logehvi3_compute: bad arguments (M >= 0, arrays required)");
  B7_TRY(samples3_refuse(c, "logehvi3_compute", S));
  B7_TRY(front3_refuse(c, "logehvi3_compute", front, P, ref));
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t m = (size_t)M, total = (size_t)(S[0] + S[1] + S[2]) * m;
  B7_TRY(b7_ensure(c, c->ehvi3_user, sizeof(double) * (2 * total + m)));  // b7_ehvi3_compute's staging: the kept posterior stays
  double *p = (double *)c->ehvi3_user.p;
  const double *dmu[3], *dvar[3];
  for (int o = 0; o < 3; ++o) {
    const size_t n = (size_t)S[o] * m;
    B7_HIP(c, hipMemcpyAsync(p, mu[o], sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    B7_HIP(c, hipMemcpyAsync(p + n, var[o], sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    dmu[o] = p, dvar[o] = p + n, p += 2 * n;
  }
  Staged3 st;
  stage3_host(front, P, ref, &st);
  B7_TRY(launch_logehvi3(c, dmu, dvar, S, st, M, p));
  B7_HIP(c, hipMemcpyAsync(out, p, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staged front are consumed
  return B7_OK;
}

int b7_logehvi3_nominate(b7_ctx *c, b7_ctx *other2, b7_ctx *other3, const double *front, int P, const double *ref, double *best_val,
                         int64_t *best_idx1) {
  if (!c) return B7_ERR_INVALID;
  if (!other2) return b7_fail(c, B7_ERR_INVALID, "logehvi3_nominate: the second objective's context is NULL");
  if (!other3) return b7_fail(c, B7_ERR_INVALID, "logehvi3_nominate: the third objective's context is NULL");
  if (!best_val || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "logehvi3_nominate: NULL argument (best_val and best_idx1 are needed)");
  b7_ctx *o[3] = {c, other2, other3};
  static const char *const nth[3] = {"first", "second", "third"};
  if (c->group || other2->group || other3->group)
    return b7_fail(c, B7_ERR_STATE, "logehvi3_nominate: a context belongs to a group (three objectives over a sharded grid are not built)");
  for (int m = 1; m < 3; ++m)
    if (o[m]->device != c->device)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "logehvi3_nominate: the %s objective's context is on device %d, this one on device %d (a posterior across devices is not built)",
                     nth[m], o[m]->device, c->device);
  for (int m = 0; m < 3; ++m)
    if (!o[m]->post_valid)
      return b7_fail(c, B7_ERR_STATE, "logehvi3_nominate: no kept posterior of the %s objective (call b7_eval_posterior on its context; a change of the grid or the data forgets it)",
                     nth[m]);
  for (int m = 1; m < 3; ++m)
    if (o[m]->post_M != c->post_M)
      return b7_fail(c, B7_ERR_INVALID, "logehvi3_nominate: the %s objective's grid has %lld rows, this one %lld", nth[m], (long long)o[m]->post_M,
                     (long long)c->post_M);
  const int S[3] = {c->post_S, other2->post_S, other3->post_S};
  B7_TRY(samples3_refuse(c, "logehvi3_nominate", S));
  B7_TRY(front3_refuse(c, "logehvi3_nominate", front, P, ref));
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->post_M;  // == c->M: a grid change would have forgotten the posterior
  const double *mu[3], *var[3];
  for (int m = 0; m < 3; ++m) mu[m] = (const double *)o[m]->post.p, var[m] = mu[m] + (size_t)S[m] * (size_t)M;
  B7_TRY(b7_ensure(c, c->acc, sizeof(double) * (size_t)M));
  Staged3 st;
  stage3_host(front, P, ref, &st);
  // the streams are ordered by events both ways, as b7_ehvi3_nominate orders them (its events)
  const bool wait2 = other2 != c, wait3 = other3 != c && other3 != other2;
  if (wait2 || wait3)
    for (hipEvent_t &e : c->ev_ehvi3)
      if (!e) B7_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (wait2) {
    B7_HIP(c, hipEventRecord(c->ev_ehvi3[0], other2->stream));
    B7_HIP(c, hipStreamWaitEvent(c->stream, c->ev_ehvi3[0], 0));
  }
  if (wait3) {
    B7_HIP(c, hipEventRecord(c->ev_ehvi3[1], other3->stream));
    B7_HIP(c, hipStreamWaitEvent(c->stream, c->ev_ehvi3[1], 0));
  }
  acc_declare_log_written(c);  // the box kernel writes every row of it
  B7_TRY(launch_logehvi3(c, mu, var, S, st, M, (double *)c->acc.p));
  if (wait2 || wait3) {
    B7_HIP(c, hipEventRecord(c->ev_ehvi3[2], c->stream));
    if (wait2) B7_HIP(c, hipStreamWaitEvent(other2->stream, c->ev_ehvi3[2], 0));
    if (wait3) B7_HIP(c, hipStreamWaitEvent(other3->stream, c->ev_ehvi3[2], 0));
  }
  return launch_finish(c, (double *)c->acc.p, M, 1.0, best_val, best_idx1, true);  // score:max(1) of the log accumulator; waits
}

}  // extern "C"
