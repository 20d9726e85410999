// Multi-objective Thompson sampling: q nominees per call from the kept sample paths of two or three independent GPs --
// b7_ts_hvi_nominate, b7_ts_hvi3_nominate, b7_hvi_compute.  TSEMO's rule (Bradford, Schweidtmann & Lapkin 2018): under a sample path
// the world is deterministic, so the best addition to a batch is the row whose sampled values improve the hypervolume most.  No
// counterpart in the reference.  All objectives are minimised.  The paths are b7_ts_paths' (or a b7_ts_nominate's; rff.hip), one
// context per objective, each drawn with its own seed and hyper samples.
//
// The score is the deterministic limit of the closed forms of ehvi.hip and ehvi3.hip: no Psi, no erfc, no hyper-sample loop.
//   two objectives, front (a_k, b_k) canonical, a_0 = -inf, a_P+1 = r1, b_0 = r2 (front_stage's arrays):
//     hvi(y) = sum_{k = 0 .. P} max(a_k+1 - max(a_k, y1), 0) * max(b_k - y2, 0)                    k ascending, running sum from 0
//   three objectives, over the boxes (l1, u1, l2, u2, u3) of b7_nondominated_boxes3, in its order:
//     hvi(y) = sum_b (max(u1 - max(l1, y1), 0) * max(u2 - max(l2, y2), 0)) * max(u3 - y3, 0)      running sum from 0
// Contraction off: one rounded operation per operator.  A row with a value that is not finite scores NaN, and a NaN never wins.
//
// hvi2_kernel / hvi3_kernel: one candidate per lane in a grid-stride loop, the front or the boxes read through a wave-uniform index
// (scalar loads), no LDS for the score.  Objective m's values are read as (base, row stride): column j of an [M][q] path buffer
// (stride q), a contiguous column of a [q][M] copy (stride 1), or a column of b7_hvi_compute's M1 x m host array (stride m).  The
// arg-max is fused: every workgroup leaves its best (value, row) over the rows not in taken[0 .. j), the largest value first and the
// lowest row among equals; argbest.h's final kernel folds the partials into taken[j] / val[j].  No score vector is stored during a
// nomination; b7_hvi_compute runs the same kernel with `out` set and no partials.  A value depends on its own row and the front alone.
//
// The pick loop is sequential, path j = 0 .. q - 1: the working front of path j is the canonical front (b7_pareto_front2 / 3) of the
// caller's front points followed by the earlier picks' values under path j, made on the host from comparisons alone; the pick's q
// values per objective come back with its row in one record (hvi_gather_kernel).  Where no row improves the hypervolume the pick is
// the first minimum of objective 1 + (j mod m)'s path j over the rows not taken, by b7_ts_nominate's own arg-min kernels.
//
// Layout (c->ts_hvi_layout; the diagnostic build reads B7_TS_HVI_LAYOUT = 0 / 1 at b7_create): a pick that reads column j of [M][q] touches every cache line of
// the buffer for 1 / q of its bytes; ts_transpose_kernel copies each objective's paths to [q][M] once per call (two passes) and every
// pick then reads M 8-byte values per objective.  q = 1 has one layout.  The bits are the same either way.
//
// Out of scope, refused by name: sharded grids and groups, the Bayesian-linear (DNGO) head's paths, contexts on different devices,
// four or more objectives, correlated objectives.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"

namespace {

constexpr int HVI_THREADS = 256;
constexpr int HVI_BLOCKS_MAX = 1024;  // argbest_blocks' cap: the partials' room in c->ts_hvi
constexpr int HVI_BOXES_MAX = 3 * B7_EHVI3_PMAX + 1;
constexpr int HVI_REC = 2 + 3 * B7_BATCH_MAX;  // a pick's record in doubles: value | row (long long) | y[m][q] at 2 + 16 m + p
constexpr int TR_ROWS = 64;                    // rows per workgroup of the transposition

struct HviArgs {
  const double *y[3];        // objective m's values: row g at y[m][g * stride[m]]
  long long stride[3];
  const double *fr;          // two objectives: a_1 .. a_P, r1 | r2, b_1 .. b_P; three: the boxes, five doubles each
  int n;                     // P, or the box count
  long long M;
  const long long *taken;    // rows kept out of the arg-max: taken[0 .. j)
  int j;
  double *out;               // [M], or null: no score vector
  ArgBest *part;             // [gridDim.x], or null: no arg-max
};

__device__ __forceinline__ bool hvi_finite(double v) { return fabs(v) < INFINITY; }  // false for NaN too

__device__ __forceinline__ double hvi_pos(double v) { return v > 0.0 ? v : 0.0; }

template <int NOBJ>
__device__ __forceinline__ double hvi_score(const HviArgs &g, long long row) {
  double y[NOBJ];
  bool ok = true;
#pragma unroll
  for (int m = 0; m < NOBJ; ++m) {
    y[m] = g.y[m][row * g.stride[m]];
    ok = ok && hvi_finite(y[m]);
  }
  if (!ok) return NAN;
  double sum = 0.0;
  if (NOBJ == 2) {
    const double *av = g.fr, *bv = g.fr + (g.n + 1);
    double lo = -INFINITY;
    for (int k = 0; k <= g.n; ++k) {
      const double a = av[k], b = bv[k];
      const double w = hvi_pos(a - (lo > y[0] ? lo : y[0]));
      const double h = hvi_pos(b - y[1]);
      sum = sum + (w * h);
      lo = a;
    }
  } else {
    for (int b = 0; b < g.n; ++b) {
      const double *q = g.fr + 5 * b;
      const double l1 = q[0], u1 = q[1], l2 = q[2], u2 = q[3], u3 = q[4];
      const double w1 = hvi_pos(u1 - (l1 > y[0] ? l1 : y[0]));
      const double w2 = hvi_pos(u2 - (l2 > y[1] ? l2 : y[1]));
      const double w3 = hvi_pos(u3 - y[NOBJ - 1]);
      sum = sum + ((w1 * w2) * w3);
    }
  }
  return sum;
}

// The score fused with the arg-max (argbest.h: OrderMaxNoNan, which is a total order only without NaNs: a NaN score is skipped
// here, ahead of the comparison, and so never wins)
template <int NOBJ>
__device__ __forceinline__ void hvi_body(const HviArgs &g, ArgBest *sh) {
  long long ex[ARGBEST_MAX_EXCL];
  argbest_load_excl(g.taken, g.part ? g.j : 0, ex);
  ArgBest b{0.0, -1};
  for (long long r = (long long)blockIdx.x * HVI_THREADS + threadIdx.x; r < g.M; r += (long long)gridDim.x * HVI_THREADS) {
    const double v = hvi_score<NOBJ>(g, r);
    if (g.out) g.out[r] = v;
    const ArgBest cnd{v, r};
    if (v == v && !argbest_excluded(ex, r) && OrderMaxNoNan()(cnd, b)) b = cnd;
  }
  if (!g.part) return;  // uniform over the launch
  b = block_best<OrderMaxNoNan>(b, sh);
  if (threadIdx.x == 0) g.part[blockIdx.x] = b;
}

__global__ void __launch_bounds__(HVI_THREADS) hvi2_kernel(HviArgs g) {
  __shared__ ArgBest sh[4];
  hvi_body<2>(g, sh);
}

__global__ void __launch_bounds__(HVI_THREADS) hvi3_kernel(HviArgs g) {
  __shared__ ArgBest sh[4];
  hvi_body<3>(g, sh);
}

// pick j's record: its value, its row and the row's q values under every objective's [M][q] paths
struct HviGatherArgs {
  const double *paths[3];
  const long long *taken;
  const double *val;
  double *rec;
  int j, q, m;
};
__global__ void __launch_bounds__(64) hvi_gather_kernel(HviGatherArgs g) {
  const long long row = g.taken[g.j];
  const int t = threadIdx.x;
  if (t == 0) {
    g.rec[0] = g.val[g.j];
    reinterpret_cast<long long *>(g.rec)[1] = row;
  }
  if (row < 0) return;
  if (t < g.m * B7_BATCH_MAX) {
    const int o = t / B7_BATCH_MAX, p = t - o * B7_BATCH_MAX;
    if (p < g.q) g.rec[2 + t] = g.paths[o][row * g.q + p];
  }
}

// out[p][i] = in[i][p], i < M, p < q <= 16
__global__ void __launch_bounds__(HVI_THREADS) ts_transpose_kernel(const double *__restrict__ in, long long M, int q, double *__restrict__ out) {
  __shared__ double tile[TR_ROWS * (B7_BATCH_MAX + 1)];
  const long long row0 = (long long)blockIdx.x * TR_ROWS;
  const int rows = (int)(M - row0 < TR_ROWS ? M - row0 : TR_ROWS);
  for (int e = threadIdx.x; e < rows * q; e += HVI_THREADS) {
    const int r = e / q, p = e - r * q;
    tile[r * (B7_BATCH_MAX + 1) + p] = in[row0 * q + e];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < TR_ROWS * q; e += HVI_THREADS) {
    const int p = e / TR_ROWS, r = e - p * TR_ROWS;
    if (r < rows) out[(long long)p * M + row0 + r] = tile[r * (B7_BATCH_MAX + 1) + p];
  }
}

// c->ts_hvi in doubles: the staged front or boxes | the picks' records [q] | taken [q] | val [q] | the fallback's minima [q] | partials
struct HviWork {
  double *fr, *rec, *val, *pmin;
  long long *taken;
  ArgBest *part;
};
constexpr size_t HVI_FR = 5 * (size_t)HVI_BOXES_MAX > 2 * (size_t)(B7_EHVI_PMAX + 1) ? 5 * (size_t)HVI_BOXES_MAX : 2 * (size_t)(B7_EHVI_PMAX + 1);
int hvi_work(b7_ctx *c, HviWork *w) {
  const size_t fr = (size_t)round_up((int64_t)HVI_FR, 32), rec = (size_t)round_up(B7_BATCH_MAX * HVI_REC, 32), small = 32;
  B7_TRY(b7_ensure(c, c->ts_hvi, sizeof(double) * (fr + rec + 3 * small + 2 * (size_t)HVI_BLOCKS_MAX)));
  double *p = (double *)c->ts_hvi.p;
  w->fr = p, w->rec = p + fr;
  w->taken = reinterpret_cast<long long *>(p + fr + rec);
  w->val = p + fr + rec + small, w->pmin = w->val + small;
  w->part = reinterpret_cast<ArgBest *>(w->pmin + small);
  return B7_OK;
}

// the front as the kernels read it into `host` (which must outlive the copy: the callers wait) and onto the device; *n_out: P or B
int hvi_stage(b7_ctx *c, int m, const double *front, int P, const double *ref, double *dev, std::vector<double> *host, int *n_out) {
  if (m == 2) {
    host->resize(2 * (size_t)(P + 1));
    double *av = host->data(), *bv = av + (P + 1);
    for (int k = 0; k < P; ++k) av[k] = front[2 * k], bv[k + 1] = front[2 * k + 1];
    av[P] = ref[0], bv[0] = ref[1];
    *n_out = P;
  } else {
    host->resize(5 * (size_t)HVI_BOXES_MAX);
    int B = 0;
    if (b7_nondominated_boxes3(front, P, ref, host->data(), &B) != B7_OK || B > HVI_BOXES_MAX)
      return b7_fail(c, B7_ERR_INVALID, "ts_hvi: the box decomposition of a front of %d points failed", P);
    host->resize(5 * (size_t)B);
    *n_out = B;
  }
  B7_HIP(c, hipMemcpyAsync(dev, host->data(), sizeof(double) * host->size(), hipMemcpyHostToDevice, c->stream));
  return B7_OK;
}

int launch_hvi(b7_ctx *c, int m, const HviArgs &g, int nblk) {
  PhaseScope ps(c, m == 2 ? "hvi2" : "hvi3");
  if (m == 2) hipLaunchKernelGGL(hvi2_kernel, dim3(nblk), dim3(HVI_THREADS), 0, c->stream, g);
  else hipLaunchKernelGGL(hvi3_kernel, dim3(nblk), dim3(HVI_THREADS), 0, c->stream, g);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

int ts_hvi_nominate(b7_ctx *const *o, int m, const char *who, const double *front, int P, const double *ref, double *hvi_out,
                    int64_t *best_idx1, double *y_out) {
  static const char *const nth[3] = {"first", "second", "third"};
  b7_ctx *c = o[0];
  if (!c) return B7_ERR_INVALID;
  for (int k = 1; k < m; ++k)
    if (!o[k]) return b7_fail(c, B7_ERR_INVALID, "%s: the %s objective's context is NULL", who, nth[k]);
  if (!hvi_out || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (hvi_out and best_idx1 are needed)", who);
  for (int k = 0; k < m; ++k)
    if (o[k]->group)
      return b7_fail(c, B7_ERR_STATE, "%s: a context belongs to a group (Thompson batches over a sharded grid are not built)", who);
  for (int k = 1; k < m; ++k)
    if (o[k]->device != c->device)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the %s objective's context is on device %d, this one on device %d (paths across devices are not built)",
                     who, nth[k], o[k]->device, c->device);
  for (int k = 0; k < m; ++k) {
    const int state = ts_state(o[k]);
    if (state == TS_STATE_NONE)
      return b7_fail(c, B7_ERR_STATE, "%s: no kept paths of the %s objective (call b7_ts_paths on its context)", who, nth[k]);
    if (state == TS_STATE_BLR)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the %s objective's kept paths were left by b7_blr_ts_nominate (the DNGO head is not built here)", who,
                     nth[k]);
    if (state == TS_STATE_STALE)
      return b7_fail(c, B7_ERR_STATE, "%s: the kept paths of the %s objective are stale: its grid or its data changed since (call b7_ts_paths again)",
                     who, nth[k]);
  }
  for (int k = 1; k < m; ++k) {
    if (o[k]->ts.M != c->ts.M)
      return b7_fail(c, B7_ERR_INVALID, "%s: the %s objective's grid has M = %lld rows, this one %lld", who, nth[k], (long long)o[k]->ts.M,
                     (long long)c->ts.M);
    if (o[k]->ts.q != c->ts.q)
      return b7_fail(c, B7_ERR_INVALID, "%s: the %s objective keeps q = %d paths, this one %d", who, nth[k], o[k]->ts.q, c->ts.q);
  }
  B7_TRY(m == 2 ? front_refuse(c, who, front, P, ref) : front3_refuse(c, who, front, P, ref));
  const int q = c->ts.q, pmax = m == 2 ? B7_EHVI_PMAX : B7_EHVI3_PMAX;
  if (P + q - 1 > pmax)
    return b7_fail(c, B7_ERR_INVALID, "%s: P + q - 1 = %d exceeds %d front points (the working front can grow by a point per pick)", who, P + q - 1,
                   pmax);
  B7_HIP(c, hipSetDevice(c->device));
  const int64_t M = c->ts.M;
  const int nblk = argbest_blocks(M);
  HviWork w;
  B7_TRY(hvi_work(c, &w));
  const double *paths[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < m; ++k) paths[k] = (const double *)o[k]->ts_paths.p;
  const bool transposed = c->ts_hvi_layout != 0 && q > 1;
  if (transposed) B7_TRY(b7_ensure(c, c->ts_hvi_t, sizeof(double) * (size_t)m * (size_t)q * (size_t)M));
  B7_TRY(streams_order(o, m, true));
  if (transposed) {
    PhaseScope ps(c, "ts_transpose");
    for (int k = 0; k < m; ++k)
      hipLaunchKernelGGL(ts_transpose_kernel, dim3((unsigned)((M + TR_ROWS - 1) / TR_ROWS)), dim3(HVI_THREADS), 0, c->stream, paths[k], (long long)M, q,
                         (double *)c->ts_hvi_t.p + (size_t)k * q * (size_t)M);
    B7_HIP(c, hipGetLastError());
  }

  std::vector<double> pts((size_t)(P + q) * m), wf((size_t)(P + q) * m), staged;
  std::vector<double> yv((size_t)q * m * q);  // pick i's value under objective k's path p at (i m + k) q + p
  std::copy(front, front + (size_t)P * m, pts.begin());
  double rec[HVI_REC];
  int rc = B7_OK;
  for (int j = 0; j < q && rc == B7_OK; ++j) {
    // the working front of path j: the caller's points first, then the earlier picks under this path
    for (int i = 0; i < j; ++i)
      for (int k = 0; k < m; ++k) pts[(size_t)(P + i) * m + k] = yv[((size_t)i * m + k) * q + j];
    int Pw = 0;
    rc = m == 2 ? b7_pareto_front2(pts.data(), P + j, ref, wf.data(), nullptr, &Pw) : b7_pareto_front3(pts.data(), P + j, ref, wf.data(), nullptr, &Pw);
    if (rc != B7_OK) {
      rc = b7_fail(c, B7_ERR_INVALID, "%s: the working front of path %d has %d points, more than are built", who, j, Pw);
      break;
    }
    HviArgs g;
    int n = 0;
    if ((rc = hvi_stage(c, m, wf.data(), Pw, ref, w.fr, &staged, &n)) != B7_OK) break;
    for (int k = 0; k < 3; ++k) g.y[k] = nullptr, g.stride[k] = 0;
    for (int k = 0; k < m; ++k) {
      if (transposed) g.y[k] = (const double *)c->ts_hvi_t.p + ((size_t)k * q + j) * (size_t)M, g.stride[k] = 1;
      else g.y[k] = paths[k] + j, g.stride[k] = q;
    }
    g.fr = w.fr, g.n = n, g.M = (long long)M, g.taken = w.taken, g.j = j, g.out = nullptr, g.part = w.part;
    if ((rc = launch_hvi(c, m, g, nblk)) != B7_OK) break;
    hipLaunchKernelGGL(argbest_final_kernel<OrderMaxNoNan>, dim3(1), dim3(HVI_THREADS), 0, c->stream, (const ArgBest *)w.part, nblk, j, w.taken, w.val);
    HviGatherArgs ga;
    for (int k = 0; k < 3; ++k) ga.paths[k] = paths[k];
    ga.taken = w.taken, ga.val = w.val, ga.rec = w.rec + (size_t)j * HVI_REC, ga.j = j, ga.q = q, ga.m = m;
    auto fetch = [&]() {  // the pick's record; waits, so the staged front is consumed too
      hipLaunchKernelGGL(hvi_gather_kernel, dim3(1), dim3(64), 0, c->stream, ga);
      B7_HIP(c, hipGetLastError());
      B7_HIP(c, hipMemcpyAsync(rec, ga.rec, sizeof(double) * HVI_REC, hipMemcpyDeviceToHost, c->stream));
      B7_HIP(c, hipStreamSynchronize(c->stream));
      return (int)B7_OK;
    };
    if ((rc = fetch()) != B7_OK) break;
    long long row = reinterpret_cast<const long long *>(rec)[1];
    double value = rec[0];
    if (row < 0 || !(value > 0.0)) {
      // no row improves the hypervolume under this path: objective 1 + (j mod m)'s first minimum over the rows not taken
      const int fo = j % m;
      if ((rc = launch_ts_argmin(c, paths[fo], M, q, j, w.pmin, w.taken, w.part, nblk)) != B7_OK) break;
      ga.val = w.pmin;
      if ((rc = fetch()) != B7_OK) break;
      row = reinterpret_cast<const long long *>(rec)[1];
      value = 0.0;
      if (row < 0) {
        rc = b7_fail(c, B7_ERR_STATE, "%s: path %d has no row left to pick", who, j);
        break;
      }
    }
    hvi_out[j] = value;
    best_idx1[j] = (int64_t)row + 1;
    for (int k = 0; k < m; ++k) {
      for (int p = 0; p < q; ++p) yv[((size_t)j * m + k) * q + p] = rec[2 + k * B7_BATCH_MAX + p];
      if (y_out) y_out[(size_t)j * m + k] = rec[2 + k * B7_BATCH_MAX + j];
    }
  }
  const int rc2 = streams_order(o, m, false);
  return rc != B7_OK ? rc : rc2;
}

}  // namespace

extern "C" {

int b7_ts_hvi_nominate(b7_ctx *c, b7_ctx *other, const double *front, int P, const double *ref, double *hvi_out, int64_t *best_idx1,
                       double *y_out) {
  b7_ctx *const o[3] = {c, other, nullptr};
  return ts_hvi_nominate(o, 2, "ts_hvi_nominate", front, P, ref, hvi_out, best_idx1, y_out);
}

int b7_ts_hvi3_nominate(b7_ctx *c, b7_ctx *other2, b7_ctx *other3, const double *front, int P, const double *ref, double *hvi_out,
                        int64_t *best_idx1, double *y_out) {
  b7_ctx *const o[3] = {c, other2, other3};
  return ts_hvi_nominate(o, 3, "ts_hvi3_nominate", front, P, ref, hvi_out, best_idx1, y_out);
}

int b7_hvi_compute(b7_ctx *c, const double *Y, int64_t M1, int m, const double *front, int P, const double *ref, double *out) {
  if (!c) return B7_ERR_INVALID;
  if (m != 2 && m != 3) return b7_fail(c, B7_ERR_INVALID, "hvi_compute: m = %d objectives (2 and 3 are built)", m);
  if (M1 < 0 || (M1 > 0 && (!Y || !out))) return b7_fail(c, B7_ERR_INVALID, "hvi_compute: bad arguments (M1 >= 0, arrays required)");
  B7_TRY(m == 2 ? front_refuse(c, "hvi_compute", front, P, ref) : front3_refuse(c, "hvi_compute", front, P, ref));
  if (M1 == 0) return B7_OK;
  if ((M1 + HVI_THREADS - 1) / HVI_THREADS > 0x7fffffffLL) return b7_fail(c, B7_ERR_INVALID, "hvi_compute: %lld rows are more than one launch takes", (long long)M1);
  B7_HIP(c, hipSetDevice(c->device));
  HviWork w;
  B7_TRY(hvi_work(c, &w));
  const size_t n = (size_t)M1;
  B7_TRY(b7_ensure(c, c->ts_hvi_user, sizeof(double) * (n * m + n)));  // a buffer of its own: the kept paths stay
  double *Yd = (double *)c->ts_hvi_user.p, *od = Yd + n * m;
  std::vector<double> staged;
  HviArgs g;
  B7_TRY(hvi_stage(c, m, front, P, ref, w.fr, &staged, &g.n));
  B7_HIP(c, hipMemcpyAsync(Yd, Y, sizeof(double) * n * m, hipMemcpyHostToDevice, c->stream));
  for (int k = 0; k < 3; ++k) g.y[k] = k < m ? Yd + k : nullptr, g.stride[k] = m;
  g.fr = w.fr, g.M = (long long)M1, g.taken = nullptr, g.j = 0, g.out = od, g.part = nullptr;
  B7_TRY(launch_hvi(c, m, g, argbest_blocks(M1)));
  B7_HIP(c, hipMemcpyAsync(out, od, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  B7_HIP(c, hipStreamSynchronize(c->stream));  // the caller's arrays and the staged front are consumed
  return B7_OK;
}

}  // extern "C"
