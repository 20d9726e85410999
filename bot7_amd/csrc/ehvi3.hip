// Three-objective nomination: the exact expected hypervolume improvement over a box decomposition of the non-dominated region,
// marginalised over the hyper samples of three independent GPs, linear (b7_ehvi3_*) and in log space (b7_logehvi3_*).
// No counterpart in the reference's scores/.  All objectives are minimised.  The kept posteriors it reads are b7_eval_posterior's
// (ehvi.hip).
//
// The region that no front point dominates, inside (-inf, r], is cut into disjoint boxes [l_b, u_b] with l_b3 = -inf
// (b7_nondominated_boxes3 below: the front swept in the order of the third objective over a two-dimensional staircase, 2P + 1 boxes in
// general position).  With Psi(a; mu, sigma) = E[(a - y)+] (ehvi_math.h's ehvi_psi)
//   T_m(c) = (1/S_m) sum_s Psi(c; mu_ms, sigma_ms),   T_m(-inf) = 0
//   score  = sum_b max(T_1(u_b1) - T_1(l_b1), 0) max(T_2(u_b2) - T_2(l_b2), 0) T_3(u_b3)
// exactly, without random numbers; every term is non-negative.  The volume of the dominated region is never subtracted from the box's.
// Order: s ascending within a T, each T divided once by its sample count; boxes in the decomposition's order, per box
// ((d1 * d2) * T_3) added to the running sum; contraction off, erfc and exp ocml's: one rounded operation per operator.  The log-space
// form of each of these operations is ehvi_math.h's EhviLog: ((ldiff + ldiff) + LT_3) folded by log-sum-exp.
// Row classes: any mu or var NaN, any var < 0, in any objective: NaN.  Otherwise finite for finite input and >= 0, P = 0 included:
// T_1(r1) T_2(r2) T_3(r3) (log space: -inf is legal).
//
// Two kernels per chunk of candidates, on the context's stream, each one body for Alg = EhviLin and EhviLog:
//   ehvi3_table_kernel  T[row][candidate] for the rows of the three objectives one after the other; an objective's rows are a zero row
//                       (-inf) and its distinct cuts ascending, r_m last.  One work item per (candidate, block of EHVI3_CB cuts of one
//                       objective): the samples are walked once, EHVI3_CB running sums (log space: running (m, acc) pairs) in
//                       registers, stores coalesced across candidates.
//                       Cut block 0 of an objective also writes the zero row and the objective's row-class flag.
//   ehvi3_box_kernel    one candidate per lane, one wave per workgroup; the boxes as five table rows each (wave-uniform: ordinary
//                       loads of a small device array that come out as scalar loads), five coalesced table reads and the clamped
//                       product per box, the reads of four boxes in flight at a time (the walk is a chain of memory round trips),
//                       the sum in box order.
// The table is (sum_m (cuts_m + 1)) doubles per candidate; the candidates are cut into chunks so that it stays within
// min(workspace, EHVI3_TABLE_BYTES) (b7_set_workspace) in a buffer of its own.  256 MiB by measurement: a chunk
// must hold enough candidates for the box walk to fill the chip (P = 128: 85 696), and the walk still reads the table from the caches.
// A row's bits do not depend on the chunking: every work item sees one candidate only.
// An LDS-resident table ([cut][lane], one wave per workgroup) would cap P near 41 in 64 KiB and was not built: fronts up to
// B7_EHVI3_PMAX need the table in memory either way.
//
// Out of scope, refused by name where it can be asked for: four or more objectives, correlated objectives / multi-task GPs,
// batches, refinement, constraints combined with objectives, sharded grids and groups, the Bayesian-linear head,
// trust regions.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "b7_internal.h"
#include "ehvi_math.h"

namespace {

constexpr int EHVI3_LANES = 64;                        // table kernel: one wave per workgroup
constexpr int EHVI3_BOX_LANES = 64;                    // box kernel: one wave per workgroup too, so that a chunk spreads over the CUs
constexpr int EHVI3_CB = 8;                            // cuts per work item of the table kernel
#ifndef B7_EHVI3_TABLE_MIB
#define B7_EHVI3_TABLE_MIB 256                         // (a build-time switch for the comparison of 16 / 64 / 256 / 1024 in DESIGN section 8 only)
#endif
constexpr size_t EHVI3_TABLE_BYTES = (size_t)B7_EHVI3_TABLE_MIB << 20;  // the table's share of a chunk, at most
constexpr int EHVI3_BOXES_MAX = 3 * B7_EHVI3_PMAX + 1;

struct Ehvi3TableArgs {
  const double *mu[3], *var[3];  // [S_m][ld], already moved to the chunk's first candidate
  long long ld;                  // candidates of the whole posterior
  const double *cuts;            // cuts of objective 0 | 1 | 2, each ascending and distinct, r_m last
  int S[3], ncut[3];
  double *T;                     // [rows][C]: T, or LT in log space
  int *flag;                     // [3][C]: the objective's row class (1: NaN)
  long long C, n;                // the table's row stride, the candidates of this chunk (n <= C)
};

template <class Alg>
__global__ void __launch_bounds__(EHVI3_LANES) ehvi3_table_kernel(Ehvi3TableArgs g) {
  const long long j = (long long)blockIdx.x * EHVI3_LANES + threadIdx.x;
  if (j >= g.n) return;
  // blockIdx.y -> (objective, first cut): wave-uniform
  const int nb0 = (g.ncut[0] + EHVI3_CB - 1) / EHVI3_CB, nb1 = (g.ncut[1] + EHVI3_CB - 1) / EHVI3_CB;
  int y = (int)blockIdx.y, m = 0, cut0 = 0, row0 = 0;
  if (y >= nb0 + nb1) m = 2, y -= nb0 + nb1, cut0 = g.ncut[0] + g.ncut[1], row0 = g.ncut[0] + g.ncut[1] + 2;
  else if (y >= nb0) m = 1, y -= nb0, cut0 = g.ncut[0], row0 = g.ncut[0] + 1;
  const int k0 = y * EHVI3_CB, nk = g.ncut[m] - k0;  // this item's cuts: k0 .. k0 + min(nk, CB) - 1
  const double *mu = g.mu[m], *var = g.var[m];
  const int S = g.S[m];
  double cv[EHVI3_CB];
  typename Alg::Fold acc[EHVI3_CB];
#pragma unroll
  for (int k = 0; k < EHVI3_CB; ++k) cv[k] = k < nk ? g.cuts[cut0 + k0 + k] : 0.0, acc[k] = Alg::empty();
  bool bad = false;
  for (int s = 0; s < S; ++s) {
    const double mm = mu[(long long)s * g.ld + j], v = var[(long long)s * g.ld + j];
    bad = bad || !(v >= 0.0) || mm != mm;
    double sv[Alg::NV];
    Alg::stage(mm, v, sv);
#pragma unroll
    for (int k = 0; k < EHVI3_CB; ++k)
      if (k < nk) Alg::add(acc[k], Alg::psi(cv[k], sv));
  }
  const double n = Alg::count(S);
  double *Trow = g.T + (long long)(row0 + 1 + k0) * g.C + j;  // row0: the objective's zero row
#pragma unroll
  for (int k = 0; k < EHVI3_CB; ++k)
    if (k < nk) Trow[(long long)k * g.C] = Alg::mean(acc[k], n);
  if (y == 0) {
    g.T[(long long)row0 * g.C + j] = Alg::none();
    g.flag[(long long)m * g.C + j] = bad ? 1 : 0;
  }
}

struct Ehvi3BoxArgs {
  const double *T;
  const int *flag;
  const int *box;  // [B][5]: the table rows of l1, u1, l2, u2, u3
  int B;
  long long C, n;
  double *out;     // [n]
};

template <class Alg>
__global__ void __launch_bounds__(EHVI3_BOX_LANES) ehvi3_box_kernel(Ehvi3BoxArgs g) {
  const long long j = (long long)blockIdx.x * EHVI3_BOX_LANES + threadIdx.x;
  if (j >= g.n) return;
  if ((g.flag[j] | g.flag[g.C + j] | g.flag[2 * g.C + j]) != 0) {
    g.out[j] = NAN;
    return;
  }
  const double *T = g.T + j;
  typename Alg::Fold score = Alg::empty();
  // four boxes' reads in flight: a lane's box walk is a chain of memory round trips, and the sum stays in box order
#pragma unroll 4
  for (int b = 0; b < g.B; ++b) {
    const int *q = g.box + 5 * b;
    const double l1 = T[(long long)q[0] * g.C], u1 = T[(long long)q[1] * g.C], l2 = T[(long long)q[2] * g.C], u2 = T[(long long)q[3] * g.C];
    const double u3 = T[(long long)q[4] * g.C];
    Alg::add(score, Alg::times(Alg::times(Alg::diff(u1, l1), Alg::diff(u2, l2)), u3));
  }
  g.out[j] = Alg::value(score);
}

bool finite3(const double *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }
bool inside3(const double *p, const double *ref) { return p[0] < ref[0] && p[1] < ref[1] && p[2] < ref[2]; }
bool dominates3(const double *q, const double *p) { return q[0] <= p[0] && q[1] <= p[1] && q[2] <= p[2]; }  // weakly: q != p is the caller's
// the canonical order: by the third objective, then the first, then the second
bool before3(const double *p, const double *q) {
  if (p[2] != q[2]) return p[2] < q[2];
  if (p[0] != q[0]) return p[0] < q[0];
  return p[1] < q[1];
}

// 0: canonical.  Otherwise what is wrong, for the messages: 1 ref not finite; 2 point k not finite; 3 point k not strictly inside the
// box; 4 points k - 1, k not strictly ascending in the order (third, first, second); 5 point k dominated by point k2
int front3_defect(const double *front, int P, const double *ref, int *k_out, int *k2_out) {
  *k_out = 0, *k2_out = 0;
  if (!finite3(ref)) return 1;
  for (int k = 0; k < P; ++k) {
    const double *p = front + 3 * (size_t)k;
    *k_out = k;
    if (!finite3(p)) return 2;
    if (!inside3(p, ref)) return 3;
    if (k > 0 && !before3(p - 3, p)) return 4;
  }
  for (int k = 0; k < P; ++k)
    for (int q = 0; q < P; ++q)
      if (q != k && dominates3(front + 3 * (size_t)q, front + 3 * (size_t)k)) {
        *k_out = k, *k2_out = q;
        return 5;
      }
  return 0;
}

}  // namespace

// front3_refuse, samples3_refuse, stage3_host and launch_ehvi3 are ehvi.hip's ehvi_nominate's too (b7_internal.h, with Staged3)
int front3_refuse(b7_ctx *c, const char *who, const double *front, int P, const double *ref) {
  if (!ref) return b7_fail(c, B7_ERR_INVALID, "%s: ref is NULL", who);
  if (P < 0 || P > B7_EHVI3_PMAX) return b7_fail(c, B7_ERR_INVALID, "%s: a front of %d points (0..%d are built)", who, P, B7_EHVI3_PMAX);
  if (P > 0 && !front) return b7_fail(c, B7_ERR_INVALID, "%s: front is NULL", who);
  int k = 0, k2 = 0;
  const int what = front3_defect(front, P, ref, &k, &k2);
  const double *p = front + 3 * (size_t)k;
  switch (what) {
    case 0: return B7_OK;
    case 1: return b7_fail(c, B7_ERR_INVALID, "%s: the reference point (%g, %g, %g) is not finite", who, ref[0], ref[1], ref[2]);
    case 2: return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d (%g, %g, %g) is not finite", who, k + 1, p[0], p[1], p[2]);
    case 3:
      return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d (%g, %g, %g) is not strictly inside the reference box (%g, %g, %g)",
                     who, k + 1, p[0], p[1], p[2], ref[0], ref[1], ref[2]);
    case 4:
      return b7_fail(c, B7_ERR_INVALID,
                     "%s: the front is not canonical: points %d and %d are not sorted, strictly ascending by the third, then the first, then the second objective",
                     who, k, k + 1);
    default:
      return b7_fail(c, B7_ERR_INVALID, "%s: the front is not canonical: point %d is dominated by point %d", who, k + 1, k2 + 1);
  }
}

int samples3_refuse(b7_ctx *c, const char *who, const int *S) {
  for (int m = 0; m < 3; ++m)
    if (S[m] < 1 || S[m] > B7_EHVI_SMAX)
      return b7_fail(c, B7_ERR_INVALID, "%s: S = (%d, %d, %d) hyper samples (1..%d per objective are built)", who, S[0], S[1], S[2], B7_EHVI_SMAX);
  return B7_OK;
}

namespace {

// The decomposition (bot7hip.h): boxes as l1, u1, l2, u2, u3 appended to `out`.  The front is canonical.
void boxes3(const double *front, int P, const double *ref, std::vector<double> *out) {
  std::vector<std::pair<double, double>> st;  // the staircase of the projections seen so far: a ascending, b descending, both strictly
  for (int k = 0; k < P; ++k) {
    const double a = front[3 * k], b = front[3 * k + 1], cc = front[3 * k + 2];
    size_t i = 0;
    while (i < st.size() && st[i].first <= a) ++i;  // the first staircase point to the right of a
    double level = i == 0 ? ref[1] : st[i - 1].second;
    if (!(level > b)) continue;                      // the projection is dominated already: nothing new (ties in the third objective only)
    double x = a;
    for (size_t j = i;; ++j) {
      const double nx = j < st.size() ? st[j].first : ref[0];
      const double box[5] = {x, nx, b, level, cc};
      out->insert(out->end(), box, box + 5);
      if (j == st.size()) break;
      level = st[j].second;
      if (!(level > b)) break;
      x = nx;
    }
    st.erase(std::remove_if(st.begin(), st.end(), [&](const std::pair<double, double> &p) { return p.first >= a && p.second >= b; }), st.end());
    st.insert(std::upper_bound(st.begin(), st.end(), std::make_pair(a, b)), std::make_pair(a, b));
  }
  for (size_t k = 0; k <= st.size(); ++k) {
    const double box[5] = {k == 0 ? -INFINITY : st[k - 1].first, k < st.size() ? st[k].first : ref[0], -INFINITY,
                           k == 0 ? ref[1] : st[k - 1].second, ref[2]};
    out->insert(out->end(), box, box + 5);
  }
}

}  // namespace

void stage3_host(const double *front, int P, const double *ref, Staged3 *st) {
  int row0[3], cut0[3];
  st->cuts.clear();
  st->rows = 0;
  for (int m = 0; m < 3; ++m) {
    std::vector<double> v;
    for (int k = 0; k < P; ++k) v.push_back(front[3 * k + m]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    v.push_back(ref[m]);  // above every coordinate of the front
    cut0[m] = (int)st->cuts.size(), row0[m] = st->rows;
    st->ncut[m] = (int)v.size(), st->rows += (int)v.size() + 1;
    st->cuts.insert(st->cuts.end(), v.begin(), v.end());
  }
  std::vector<double> bx;
  boxes3(front, P, ref, &bx);
  st->B = (int)(bx.size() / 5);
  st->box.resize(bx.size());
  static const int obj[5] = {0, 0, 1, 1, 2};
  for (size_t i = 0; i < bx.size(); ++i) {
    const int m = obj[i % 5];
    const double *lo = st->cuts.data() + cut0[m], *hi = lo + st->ncut[m];
    // -inf is the zero row; every other edge is a coordinate of the front or of ref, hence one of the cuts exactly (-1 otherwise:
    // launch_ehvi3 refuses it)
    const double *it = std::lower_bound(lo, hi, bx[i]);
    st->box[i] = bx[i] == -INFINITY ? row0[m] : (it != hi && *it == bx[i]) ? row0[m] + 1 + (int)(it - lo) : -1;
  }
}

namespace {

// candidates per chunk: the table within min(workspace, EHVI3_TABLE_BYTES), whole waves of the table kernel, at least one
int64_t chunk3(const b7_ctx *c, int rows, int64_t M) {
  const size_t per = sizeof(double) * (size_t)rows + 3 * sizeof(int);
  int64_t C = (int64_t)(std::min(c->ks_bytes, EHVI3_TABLE_BYTES) / per) / EHVI3_LANES * EHVI3_LANES;
  C = std::max<int64_t>(C, EHVI3_LANES);
  return std::min<int64_t>(C, round_up(M, EHVI3_LANES));
}

// the score of M rows onto out (device), on c's stream: mu[m] / var[m] [S_m][M] on the device.  The host block `st` must outlive the
// copies (the callers wait)
template <class Alg>
int launch_ehvi3_as(b7_ctx *c, const double *const *mu, const double *const *var, const int *S, const Staged3 &st, int64_t M, double *out) {
  const char *who = Alg::name3;
  if (M > 0x7fffffffLL * EHVI3_LANES) return b7_fail(c, B7_ERR_INVALID, "%s: %lld rows are more than one launch takes", who, (long long)M);
  // what the kernels index by: every box row inside the table, the box and cut counts inside their staging
  for (int r : st.box)
    if (r < 0 || r >= st.rows) return b7_fail(c, B7_ERR_INVALID, "%s: a box edge is none of the cuts (row %d of %d)", who, r, st.rows);
  if (st.B > EHVI3_BOXES_MAX || st.rows > 3 * (B7_EHVI3_PMAX + 2))
    return b7_fail(c, B7_ERR_INVALID, "%s: %d boxes over %d table rows are more than a front of %d points gives", who, st.B, st.rows, B7_EHVI3_PMAX);
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
  for (int m = 0; m < 3; ++m) nblk += (st.ncut[m] + EHVI3_CB - 1) / EHVI3_CB;
  for (int64_t j0 = 0; j0 < M; j0 += C) {
    const int64_t n = std::min<int64_t>(C, M - j0);
    Ehvi3TableArgs t;
    for (int m = 0; m < 3; ++m) t.mu[m] = mu[m] + j0, t.var[m] = var[m] + j0, t.S[m] = S[m], t.ncut[m] = st.ncut[m];
    t.ld = (long long)M, t.cuts = cuts_d;
    t.T = (double *)c->ehvi3_table.p, t.flag = (int *)((char *)c->ehvi3_table.p + tab_bytes);
    t.C = (long long)C, t.n = (long long)n;
    {
      PhaseScope ps(c, Alg::phase3_tab);
      hipLaunchKernelGGL(ehvi3_table_kernel<Alg>, dim3((unsigned)((n + EHVI3_LANES - 1) / EHVI3_LANES), (unsigned)nblk), dim3(EHVI3_LANES), 0, c->stream, t);
      B7_HIP(c, hipGetLastError());
    }
    Ehvi3BoxArgs b;
    b.T = t.T, b.flag = t.flag, b.box = box_d, b.B = st.B, b.C = t.C, b.n = t.n, b.out = out + j0;
    {
      PhaseScope ps(c, Alg::phase3_box);
      hipLaunchKernelGGL(ehvi3_box_kernel<Alg>, dim3((unsigned)((n + EHVI3_BOX_LANES - 1) / EHVI3_BOX_LANES)), dim3(EHVI3_BOX_LANES), 0, c->stream, b);
      B7_HIP(c, hipGetLastError());
    }
  }
  return B7_OK;
}

// the two-dimensional area that the projections of `pts` (a, b pairs, any order) dominate under (r1, r2): b7_hypervolume2's sum over
// the staircase of the set
double area2(std::vector<std::pair<double, double>> pts, double r1, double r2) {
  std::sort(pts.begin(), pts.end());
  std::vector<std::pair<double, double>> st;
  double low = INFINITY;
  for (const auto &p : pts)
    if (p.second < low) st.push_back(p), low = p.second;
  double area = 0.0;
  for (size_t k = 0; k < st.size(); ++k) {
    const double next = k + 1 < st.size() ? st[k + 1].first : r1;
    area = area + ((next - st[k].first) * (r2 - st[k].second));
  }
  return area;
}

}  // namespace

int launch_ehvi3(b7_ctx *c, bool log, const double *const *mu, const double *const *var, const int *S, const Staged3 &st, int64_t M, double *out) {
  return log ? launch_ehvi3_as<EhviLog>(c, mu, var, S, st, M, out) : launch_ehvi3_as<EhviLin>(c, mu, var, S, st, M, out);
}

// b7_ehvi3_compute / b7_logehvi3_compute: the score of the caller's host arrays
static int ehvi3_compute(b7_ctx *c, bool log, const char *who, const double *const *mu, const double *const *var, const int *S, const double *front,
                         int P, const double *ref, int64_t M, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (!mu || !var || !S) return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (mu, var and S of three objectives are needed)", who);
  if (M < 0 || (M > 0 && (!mu[0] || !var[0] || !mu[1] || !var[1] || !mu[2] || !var[2] || !out)))
    return b7_fail(c, B7_ERR_INVALID, "%s: bad arguments (M >= 0, arrays required)", who);
  B7_TRY(samples3_refuse(c, who, S));
  B7_TRY(front3_refuse(c, who, front, P, ref));
  if (M == 0) return B7_OK;
  B7_HIP(c, hipSetDevice(c->device));
  const size_t m = (size_t)M, total = (size_t)(S[0] + S[1] + S[2]) * m;
  B7_TRY(b7_ensure(c, c->ehvi3_user, sizeof(double) * (2 * total + m)));  // a buffer of its own: the kept posterior stays
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
  B7_TRY(launch_ehvi3(c, log, dmu, dvar, S, st, M, p));
  B7_HIP(c, hipMemcpyAsync(out, p, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staged front are consumed
  return B7_OK;
}

extern "C" {

int b7_pareto_front3(const double *Y, int64_t n, const double *ref, double *front_out, int64_t *rows1_out, int *P_out) {
  if (!ref || !P_out || n < 0 || (n > 0 && (!Y || !front_out))) return B7_ERR_INVALID;
  *P_out = 0;
  if (!finite3(ref)) return B7_ERR_INVALID;
  std::vector<int64_t> in;
  for (int64_t i = 0; i < n; ++i)
    if (finite3(Y + 3 * i) && inside3(Y + 3 * i, ref)) in.push_back(i);
  // in the canonical order, then by the row: a point can only be dominated by, or equal to, one that comes before it
  std::sort(in.begin(), in.end(), [&](int64_t p, int64_t q) {
    if (before3(Y + 3 * p, Y + 3 * q)) return true;
    if (before3(Y + 3 * q, Y + 3 * p)) return false;
    return p < q;
  });
  std::vector<int64_t> keep;
  for (int64_t i : in) {
    bool dom = false;
    for (int64_t q : keep)
      if (dominates3(Y + 3 * q, Y + 3 * i)) {  // equal rows too: the lowest stays
        dom = true;
        break;
      }
    if (!dom) keep.push_back(i);
  }
  *P_out = keep.size() > (size_t)0x7fffffff ? 0x7fffffff : (int)keep.size();
  if (keep.size() > (size_t)B7_EHVI3_PMAX) return B7_ERR_INVALID;
  for (size_t k = 0; k < keep.size(); ++k) {
    for (int m = 0; m < 3; ++m) front_out[3 * k + m] = Y[3 * keep[k] + m];
    if (rows1_out) rows1_out[k] = keep[k] + 1;
  }
  return B7_OK;
}

int b7_nondominated_boxes3(const double *front, int P, const double *ref, double *boxes_out, int *B_out) {
  if (!ref || !B_out || !boxes_out || P < 0 || P > B7_EHVI3_PMAX || (P > 0 && !front)) return B7_ERR_INVALID;
  *B_out = 0;
  int k = 0, k2 = 0;
  if (front3_defect(front, P, ref, &k, &k2) != 0) return B7_ERR_INVALID;
  std::vector<double> bx;
  boxes3(front, P, ref, &bx);
  *B_out = (int)(bx.size() / 5);
  std::copy(bx.begin(), bx.end(), boxes_out);
  return B7_OK;
}

int b7_hypervolume3(const double *front, int P, const double *ref, double *hv_out) {
  if (!ref || !hv_out || P < 0 || (P > 0 && !front)) return B7_ERR_INVALID;
  int k = 0, k2 = 0;
  if (P > B7_EHVI3_PMAX || front3_defect(front, P, ref, &k, &k2) != 0) return B7_ERR_INVALID;
  // slabs between consecutive distinct third coordinates (the last one up to r3), each times the area its points and all below dominate
  double hv = 0.0;
  std::vector<std::pair<double, double>> pts;
  for (k = 0; k < P;) {
    const double z = front[3 * k + 2];
    for (; k < P && front[3 * k + 2] == z; ++k) pts.push_back(std::make_pair(front[3 * k], front[3 * k + 1]));
    const double znext = k < P ? front[3 * k + 2] : ref[2];
    hv = hv + (area2(pts, ref[0], ref[1]) * (znext - z));
  }
  *hv_out = hv;
  return B7_OK;
}


int b7_ehvi3_compute(b7_ctx *c, const double *const *mu, const double *const *var, const int *S, const double *front, int P, const double *ref,
                     int64_t M, double *out) {
  return ehvi3_compute(c, false, "ehvi3_compute", mu, var, S, front, P, ref, M, out);
}

int b7_logehvi3_compute(b7_ctx *c, const double *const *mu, const double *const *var, const int *S, const double *front, int P, const double *ref,
                        int64_t M, double *out) {
  return ehvi3_compute(c, true, "logehvi3_compute", mu, var, S, front, P, ref, M, out);
}

int b7_ehvi3_nominate(b7_ctx *c, b7_ctx *other2, b7_ctx *other3, const double *front, int P, const double *ref, double *best_val,
                      int64_t *best_idx1) {
  b7_ctx *const o[3] = {c, other2, other3};
  return ehvi_nominate(o, 3, false, "ehvi3_nominate", front, P, ref, best_val, best_idx1);
}

int b7_logehvi3_nominate(b7_ctx *c, b7_ctx *other2, b7_ctx *other3, const double *front, int P, const double *ref, double *best_val,
                         int64_t *best_idx1) {
  b7_ctx *const o[3] = {c, other2, other3};
  return ehvi_nominate(o, 3, true, "logehvi3_nominate", front, P, ref, best_val, best_idx1);
}

}  // extern "C"
