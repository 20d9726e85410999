// Constrained Thompson sampling: q feasible-first nominees per call from the kept sample paths of an objective and C constraints --
// b7_ts_feas_nominate, b7_ts_feas_compute.  The selection rule of SCBO (Eriksson & Poloczek, AISTATS 2021): under a joint sample path
// (f_j, c_1j .. c_Cj) the world is deterministic, so path j takes the row of lowest f_j among the rows where every c_kj <= t_k, and
// where the path sees no such row the row of smallest total violation.  No feasibility weight, no incumbent.  No counterpart in the
// reference.  The paths are b7_ts_paths' (or a b7_ts_nominate's; rff.hip), one context per model, each drawn with its own seed and
// hyper samples.
//
// The key of (row i, path j), thresholds t_k finite, contraction off, one rounded operation per operator:
//   viol = ((0 + max(c_1j[i] - t_1, 0)) + max(c_2j[i] - t_2, 0)) + ..            k ascending, running sum from 0
//   class -1  any of the 1 + C values is NaN: the row never wins
//   class  0  viol == 0 (every c_k <= t_k: a difference of two distinct doubles is never 0), key f_j[i]
//   class  1  otherwise, key viol
// Class 0 before class 1, the smaller key within a class, the lowest row among equal keys.  The terms are non-negative, so +-inf need
// no special case.  C = 0 is b7_ts_nominate's rule.  A key depends on its own row and the thresholds alone.
//
// ts_feas_kernel<Q>: one grid row per lane in a grid-stride loop; the lane reads the row's Q contiguous doubles from each of the 1 + C
// [M][Q] buffers (pointers and thresholds in the argument struct: scalar registers) and keeps the best (class, key, row) of each of the
// Q paths in registers -- Q is a template parameter, so that the per-path bests are never indexed dynamically (no scratch).  No
// exclusions here.  The workgroup folds its lanes' bests through LDS by halving, four paths at a time, and leaves partials
// [nblk][Q].  With `out` set the pass also writes viol as [M][Q], NaN for class -1 (b7_ts_feas_compute).  Every buffer is read once.
// ts_feas_path_kernel: the same body for one path j (column j at stride q) over the rows not in taken[0 .. nt).
// ts_feas_fold_kernel (one workgroup): the partials into best[j], the best row of path j, with the row's 1 + C path-j values.
//
// The pick is sequential in the exclusions alone: path j's key does not depend on the earlier picks.  After ONE wait the host walks
// j = 0 .. q - 1: where b[j], the best over all rows, is not among taken[0 .. j) it is the pick (exact: it is the best over a superset
// and it is not excluded); otherwise path j is run again alone with the exclusion list (one more wait; counted in reruns).  A path
// with no scoring row reports index 0, class -1, key NaN and excludes nothing.  With distinct minimisers the stage is two launches and
// one wait.
//
// c->ts_feas_onepass (the diagnostic build reads B7_TS_FEAS_ONEPASS = 0 / 1 at b7_create): 0, THE DEFAULT, picks path by path, q
// passes of the one-path kernel chained on the device, each with the earlier picks excluded -- launch_ts_argmins' shape --, one wait,
// reruns reported as 0.  Measured: the one pass is 8 times faster than sixteen path passes, but paths of one
// posterior share their minimisers, 13 or 14 of 16 paths ran again at 2^20 rows, and with a wait per rerun the one-pass arm came
// out 1.3 - 1.4 times SLOWER than the chained passes.  The bits are the same.
//
// Out of scope, refused by name: sharded grids and groups, the Bayesian-linear (DNGO) head's paths, contexts on different devices,
// more than B7_TS_FEAS_CMAX constraints.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <vector>

#include "b7_internal.h"

namespace {

constexpr int TF_THREADS = 256;
constexpr int TF_CHUNK = 4;  // paths per trip of the workgroup's reduction through LDS
constexpr int TF_BLOCKS_MAX = 1024;
constexpr int TF_YW = 1 + B7_TS_FEAS_CMAX;  // a pick's values: f, c_1 .. c_C

struct TfBest {
  double key;
  long long row;  // -1: none
  int cls, pad;
};

struct TfArgs {
  const double *buf[TF_YW];  // f, c_1 .. c_C: [M][q] each
  double t[B7_TS_FEAS_CMAX];
  int C, q;
  long long M;
  double *out;    // viol [M][q], or null
  TfBest *part;   // [gridDim.x][q] (the one-path kernel: [gridDim.x]), or null: no arg-min
  int j, nt;      // the one-path kernel: the path, and how many of taken[] are excluded
  const long long *taken;
};

// the class of (row, path) with its key and its violation (NaN for class -1); e: the entry's index row * q + path
__device__ __forceinline__ int tf_key(const TfArgs &g, long long e, double *key, double *viol_out) {
  const double f = g.buf[0][e];
  bool nan = f != f;
  double viol = 0.0;
  for (int k = 0; k < g.C; ++k) {  // uniform bounds: the pointers and thresholds stay in scalar registers
    const double cv = g.buf[1 + k][e];
    nan = nan || cv != cv;
    const double d = cv - g.t[k];
    viol = viol + (d > 0.0 ? d : 0.0);
  }
  if (nan) {
    *key = NAN, *viol_out = NAN;
    return -1;
  }
  *viol_out = viol;
  if (viol == 0.0) {
    *key = f;
    return 0;
  }
  *key = viol;
  return 1;
}

// a: a candidate; b: the best so far.  A class below 0 is no candidate.
__device__ __forceinline__ bool tf_better(int ac, double ak, long long ai, int bc, double bk, long long bi) {
  if (ac < 0) return false;
  if (bc < 0) return true;
  if (ac != bc) return ac < bc;
  if (ak != bk) return ak < bk;
  return ai < bi;
}

__device__ __forceinline__ bool tf_better(const TfBest &a, const TfBest &b) { return tf_better(a.cls, a.key, a.row, b.cls, b.key, b.row); }

// sm[0 .. n) into sm[0] by halving, n a power of two, one entry per thread of the group; t: the thread's place in its group
__device__ __forceinline__ void tf_tree(TfBest *sm, int t, int n) {
  __syncthreads();
  for (int s = n / 2; s > 0; s >>= 1) {
    if (t < s && tf_better(sm[t + s], sm[t])) sm[t] = sm[t + s];
    __syncthreads();
  }
}

template <int Q>
__global__ void __launch_bounds__(TF_THREADS) ts_feas_kernel(TfArgs g) {
  __shared__ TfBest sm[TF_CHUNK][TF_THREADS];
  int bc[Q];
  double bk[Q];
  long long bi[Q];
#pragma unroll
  for (int p = 0; p < Q; ++p) bc[p] = -1, bk[p] = NAN, bi[p] = -1;
  for (long long r = (long long)blockIdx.x * TF_THREADS + threadIdx.x; r < g.M; r += (long long)gridDim.x * TF_THREADS) {
    // tf_key for the row's Q paths at once, constraint by constraint: the same operations in the same order; a NaN value makes the
    // running sum NaN, and a NaN stays one
    double fv[Q], viol[Q];
    const double *fp = g.buf[0] + r * Q;
#pragma unroll
    for (int p = 0; p < Q; ++p) fv[p] = fp[p], viol[p] = 0.0;
#pragma clang loop unroll(disable)
    for (int k = 0; k < g.C; ++k) {  // uniform bounds: the pointers and thresholds stay in scalar registers
      const double *cp = g.buf[1 + k] + r * Q;
      const double t = g.t[k];
#pragma unroll
      for (int p = 0; p < Q; ++p) {
        const double cv = cp[p];
        const double d = cv - t;
        const double sum = viol[p] + (d > 0.0 ? d : 0.0);
        viol[p] = cv != cv ? (double)NAN : sum;
      }
    }
#pragma unroll
    for (int p = 0; p < Q; ++p) {
      const bool nan = fv[p] != fv[p] || viol[p] != viol[p];
      const int cls = nan ? -1 : viol[p] == 0.0 ? 0 : 1;
      const double key = cls == 0 ? fv[p] : viol[p];
      if (g.out) g.out[r * Q + p] = nan ? (double)NAN : viol[p];
      if (tf_better(cls, key, r, bc[p], bk[p], bi[p])) bc[p] = cls, bk[p] = key, bi[p] = r;
    }
  }
  if (!g.part) return;  // uniform over the launch
  // the workgroup's best of every path: TF_CHUNK paths at a time through LDS, halving
  const int t = threadIdx.x;
#pragma unroll
  for (int p0 = 0; p0 < Q; p0 += TF_CHUNK) {
#pragma unroll
    for (int i = 0; i < TF_CHUNK; ++i)
      if (p0 + i < Q) sm[i][t].key = bk[p0 + i], sm[i][t].row = bi[p0 + i], sm[i][t].cls = bc[p0 + i], sm[i][t].pad = 0;
    __syncthreads();
    for (int s = TF_THREADS / 2; s > 0; s >>= 1) {
      if (t < s) {
#pragma unroll
        for (int i = 0; i < TF_CHUNK; ++i)
          if (p0 + i < Q && tf_better(sm[i][t + s], sm[i][t])) sm[i][t] = sm[i][t + s];
      }
      __syncthreads();
    }
    if (t < TF_CHUNK && p0 + t < Q) g.part[(size_t)blockIdx.x * Q + p0 + t] = sm[t][0];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(TF_THREADS) ts_feas_path_kernel(TfArgs g) {
  __shared__ TfBest sm[TF_THREADS];
  long long tk[B7_BATCH_MAX];
#pragma unroll
  for (int i = 0; i < B7_BATCH_MAX; ++i) tk[i] = i < g.nt ? g.taken[i] : -1;  // (-1 is no row: a path that picked nothing excludes nothing)
  int bc = -1;
  double bk = NAN;
  long long bi = -1;
  for (long long r = (long long)blockIdx.x * TF_THREADS + threadIdx.x; r < g.M; r += (long long)gridDim.x * TF_THREADS) {
    double key, viol;
    int cls = tf_key(g, r * g.q + g.j, &key, &viol);
#pragma unroll
    for (int i = 0; i < B7_BATCH_MAX; ++i) cls = tk[i] == r ? -1 : cls;
    if (tf_better(cls, key, r, bc, bk, bi)) bc = cls, bk = key, bi = r;
  }
  TfBest &mine = sm[threadIdx.x];
  mine.key = bk, mine.row = bi, mine.cls = bc, mine.pad = 0;
  tf_tree(sm, threadIdx.x, TF_THREADS);
  if (threadIdx.x == 0) g.part[blockIdx.x] = sm[0];
}

// The partials [nblk][np] of paths j0 .. j0 + np - 1 into best[j0 + p], taken[j0 + p] (-1: no row scored) and the row's 1 + C values
// under its path into y[(j0 + p) TF_YW + k].  Sixteen lanes per path.
struct TfFoldArgs {
  const double *buf[TF_YW];
  const TfBest *part;
  TfBest *best;
  long long *taken;
  double *y;
  int nblk, np, j0, C, q;
};
__global__ void __launch_bounds__(TF_THREADS) ts_feas_fold_kernel(TfFoldArgs g) {
  __shared__ TfBest sm[TF_THREADS];
  const int p = threadIdx.x >> 4, l = threadIdx.x & 15;
  TfBest b;
  b.key = NAN, b.row = -1, b.cls = -1, b.pad = 0;
  if (p < g.np)
    for (int k = l; k < g.nblk; k += 16) {
      const TfBest o = g.part[(size_t)k * g.np + p];
      if (tf_better(o, b)) b = o;
    }
  sm[threadIdx.x] = b;
  tf_tree(sm + 16 * p, l, 16);   // (every thread meets every barrier: the groups halve side by side)
  if (p >= g.np) return;
  b = sm[16 * p];
  const int j = g.j0 + p;
  if (b.cls < 0) b.key = NAN, b.row = -1;
  if (l == 0) g.best[j] = b, g.taken[j] = b.row;
  if (l <= g.C && l < TF_YW) g.y[j * TF_YW + l] = b.row < 0 ? (double)NAN : g.buf[l][b.row * g.q + j];
}

// c->ts_feas: partials [TF_BLOCKS_MAX][16] | best [16] | taken [16] | y [16][TF_YW]
struct TfWork {
  TfBest *part, *best;
  long long *taken;
  double *y;
};
int tf_work(b7_ctx *c, TfWork *w) {
  const size_t part = sizeof(TfBest) * (size_t)TF_BLOCKS_MAX * B7_BATCH_MAX, best = sizeof(TfBest) * B7_BATCH_MAX;
  const size_t taken = sizeof(long long) * B7_BATCH_MAX, y = sizeof(double) * B7_BATCH_MAX * TF_YW;
  B7_TRY(b7_ensure(c, c->ts_feas, part + best + taken + y));
  char *p = (char *)c->ts_feas.p;
  w->part = reinterpret_cast<TfBest *>(p);
  w->best = reinterpret_cast<TfBest *>(p + part);
  w->taken = reinterpret_cast<long long *>(p + part + best);
  w->y = reinterpret_cast<double *>(p + part + best + taken);
  return B7_OK;
}

int tf_blocks(int64_t M) { return (int)std::min<int64_t>(TF_BLOCKS_MAX, (M + TF_THREADS - 1) / TF_THREADS); }

template <int Q>
void tf_launch_q(b7_ctx *c, const TfArgs &g, int nblk) {
  hipLaunchKernelGGL(ts_feas_kernel<Q>, dim3(nblk), dim3(TF_THREADS), 0, c->stream, g);
}

int launch_ts_feas(b7_ctx *c, const TfArgs &g, int nblk) {
  switch (g.q) {
    case 1: tf_launch_q<1>(c, g, nblk); break;
    case 2: tf_launch_q<2>(c, g, nblk); break;
    case 3: tf_launch_q<3>(c, g, nblk); break;
    case 4: tf_launch_q<4>(c, g, nblk); break;
    case 5: tf_launch_q<5>(c, g, nblk); break;
    case 6: tf_launch_q<6>(c, g, nblk); break;
    case 7: tf_launch_q<7>(c, g, nblk); break;
    case 8: tf_launch_q<8>(c, g, nblk); break;
    case 9: tf_launch_q<9>(c, g, nblk); break;
    case 10: tf_launch_q<10>(c, g, nblk); break;
    case 11: tf_launch_q<11>(c, g, nblk); break;
    case 12: tf_launch_q<12>(c, g, nblk); break;
    case 13: tf_launch_q<13>(c, g, nblk); break;
    case 14: tf_launch_q<14>(c, g, nblk); break;
    case 15: tf_launch_q<15>(c, g, nblk); break;
    case 16: tf_launch_q<16>(c, g, nblk); break;
    default: return b7_fail(c, B7_ERR_INVALID, "ts_feas: q = %d not in [1, %d]", g.q, B7_BATCH_MAX);
  }
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}
static_assert(B7_BATCH_MAX == 16, "launch_ts_feas instantiates ts_feas_kernel for q = 1 .. 16");

// path j alone over the rows not in w.taken[0 .. nt), then its fold into best[j] / taken[j] / y[j]
int launch_ts_feas_path(b7_ctx *c, TfArgs g, TfFoldArgs fa, const TfWork &w, int j, int nt, int nblk) {
  g.out = nullptr, g.part = w.part, g.j = j, g.nt = nt, g.taken = w.taken;
  hipLaunchKernelGGL(ts_feas_path_kernel, dim3(nblk), dim3(TF_THREADS), 0, c->stream, g);
  fa.np = 1, fa.j0 = j;
  hipLaunchKernelGGL(ts_feas_fold_kernel, dim3(1), dim3(TF_THREADS), 0, c->stream, fa);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// The pick stage over 1 + C device buffers [M][q] on c's stream: both entries' kernels and resolution.  viol: [M][q] on the device, or
// null.  Waits for the stream before it returns.
int tf_pick(b7_ctx *c, const double *const *buf, const double *thr, int C, int64_t M, int q, double *viol, double *key_out, int *class_out,
            int64_t *best_idx1, double *y_out, int *reruns_out) {
  TfWork w;
  B7_TRY(tf_work(c, &w));
  const int nblk = tf_blocks(M);
  TfArgs g;
  TfFoldArgs fa;
  for (int k = 0; k < TF_YW; ++k) g.buf[k] = fa.buf[k] = k <= C ? buf[k] : nullptr;
  for (int k = 0; k < B7_TS_FEAS_CMAX; ++k) g.t[k] = k < C ? thr[k] : 0.0;
  g.C = C, g.q = q, g.M = (long long)M, g.out = viol, g.part = w.part, g.j = 0, g.nt = 0, g.taken = w.taken;
  fa.part = w.part, fa.best = w.best, fa.taken = w.taken, fa.y = w.y, fa.nblk = nblk, fa.np = q, fa.j0 = 0, fa.C = C, fa.q = q;
  TfBest best[B7_BATCH_MAX];
  double y[B7_BATCH_MAX * TF_YW];
  long long tk[B7_BATCH_MAX];
  int reruns = 0;
  auto fetch = [&](int j0, int n) {
    B7_HIP(c, hipMemcpyAsync(best + j0, w.best + j0, sizeof(TfBest) * n, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipMemcpyAsync(y + j0 * TF_YW, w.y + j0 * TF_YW, sizeof(double) * n * TF_YW, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
    return (int)B7_OK;
  };
  // (phases do not nest: "ts_feas" is the one pass with its fold, "ts_feas_rerun" one path's second run -- its launch count is the
  // number of reruns --, "ts_feas_paths" the per-path arm)
  const bool onepass = c->ts_feas_onepass != 0;
  if (onepass || viol) {
    PhaseScope ps(c, "ts_feas");
    if (!onepass) g.part = nullptr;  // the violations alone: they are this pass's to write
    B7_TRY(launch_ts_feas(c, g, nblk));
    if (onepass) {
      hipLaunchKernelGGL(ts_feas_fold_kernel, dim3(1), dim3(TF_THREADS), 0, c->stream, fa);
      B7_HIP(c, hipGetLastError());
    }
  }
  if (onepass) {
    B7_TRY(fetch(0, q));
    for (int j = 0; j < q; ++j) {
      bool hit = false;
      for (int i = 0; i < j; ++i) hit = hit || (best[j].row >= 0 && tk[i] == best[j].row);
      if (hit) {
        // path j's best row went to an earlier path: path j alone over the rows not taken
        PhaseScope ps(c, "ts_feas_rerun");
        B7_HIP(c, hipMemcpyAsync(w.taken, tk, sizeof(long long) * j, hipMemcpyHostToDevice, c->stream));
        B7_TRY(launch_ts_feas_path(c, g, fa, w, j, j, nblk));
        B7_TRY(fetch(j, 1));  // (waits: tk is consumed)
        ++reruns;
      }
      tk[j] = best[j].cls < 0 ? -1 : best[j].row;
    }
  } else {
    // the per-path arm: q passes chained on the device, pass j over the rows not in taken[0 .. j), which pass i < j's fold wrote
    PhaseScope ps(c, "ts_feas_paths");
    for (int j = 0; j < q; ++j) B7_TRY(launch_ts_feas_path(c, g, fa, w, j, j, nblk));
    B7_TRY(fetch(0, q));
  }
  for (int j = 0; j < q; ++j) {
    const bool none = best[j].cls < 0;
    key_out[j] = none ? (double)NAN : best[j].key;
    class_out[j] = none ? -1 : best[j].cls;
    best_idx1[j] = none ? 0 : (int64_t)best[j].row + 1;
    if (y_out)
      for (int k = 0; k <= C; ++k) y_out[(size_t)j * (1 + C) + k] = none ? (double)NAN : y[j * TF_YW + k];
  }
  if (reruns_out) *reruns_out = reruns;
  return B7_OK;
}

int tf_thresholds(b7_ctx *c, const char *who, const double *thr, int C) {
  if (C < 0 || C > B7_TS_FEAS_CMAX) return b7_fail(c, B7_ERR_INVALID, "%s: C = %d constraints (0..%d are built)", who, C, B7_TS_FEAS_CMAX);
  if (C > 0 && !thr) return b7_fail(c, B7_ERR_INVALID, "%s: thresholds is NULL", who);
  for (int k = 0; k < C; ++k)
    if (!(fabs(thr[k]) < INFINITY)) return b7_fail(c, B7_ERR_INVALID, "%s: threshold %d (%g) is not finite", who, k + 1, thr[k]);
  return B7_OK;
}

}  // namespace

extern "C" {

int b7_ts_feas_nominate(b7_ctx *c, b7_ctx *const *cons, const double *thresholds, int C, double *key_out, int *class_out, int64_t *best_idx1,
                        double *y_out, int *reruns_out) {
  const char *who = "ts_feas_nominate";
  if (!c) return B7_ERR_INVALID;
  if (!key_out || !class_out || !best_idx1) return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (key_out, class_out and best_idx1 are needed)", who);
  B7_TRY(tf_thresholds(c, who, thresholds, C));
  if (C > 0 && !cons) return b7_fail(c, B7_ERR_INVALID, "%s: cons is NULL with C = %d constraints", who, C);
  b7_ctx *o[TF_YW];
  o[0] = c;
  for (int k = 0; k < C; ++k) {
    if (!cons[k]) return b7_fail(c, B7_ERR_INVALID, "%s: constraint %d's context is NULL", who, k + 1);
    o[1 + k] = cons[k];
  }
  const int n = 1 + C;
  auto name = [&](int k, char *s, size_t len) {
    if (k == 0) snprintf(s, len, "the objective");
    else snprintf(s, len, "constraint %d", k);
    return s;
  };
  char nm[32];
  for (int k = 0; k < n; ++k)
    if (o[k]->group)
      return b7_fail(c, B7_ERR_STATE, "%s: the context of %s belongs to a group (Thompson batches over a sharded grid are not built)", who,
                     name(k, nm, sizeof nm));
  for (int k = 0; k < n; ++k)
    if (o[k]->comm && o[k]->comm_world > 1)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the context of %s has a communicator of %d ranks (sharded Thompson sampling is not built)", who,
                     name(k, nm, sizeof nm), o[k]->comm_world);
  for (int k = 1; k < n; ++k)
    if (o[k]->device != c->device)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the context of %s is on device %d, this one on device %d (paths across devices are not built)", who,
                     name(k, nm, sizeof nm), o[k]->device, c->device);
  for (int k = 0; k < n; ++k) {
    const int state = ts_state(o[k]);
    if (state == TS_STATE_NONE)
      return b7_fail(c, B7_ERR_STATE, "%s: no kept paths of %s (call b7_ts_paths on its context)", who, name(k, nm, sizeof nm));
    if (state == TS_STATE_BLR)
      return b7_fail(c, B7_ERR_UNSUPPORTED, "%s: the kept paths of %s were left by b7_blr_ts_nominate (the DNGO head is not built here)", who,
                     name(k, nm, sizeof nm));
    if (state == TS_STATE_STALE)
      return b7_fail(c, B7_ERR_STATE, "%s: the kept paths of %s are stale: its grid, its data or its kernel changed since (call b7_ts_paths again)",
                     who, name(k, nm, sizeof nm));
  }
  for (int k = 1; k < n; ++k) {
    if (o[k]->ts.M != c->ts.M)
      return b7_fail(c, B7_ERR_INVALID, "%s: the grid of %s has M = %lld rows, the objective's %lld", who, name(k, nm, sizeof nm),
                     (long long)o[k]->ts.M, (long long)c->ts.M);
    if (o[k]->ts.q != c->ts.q)
      return b7_fail(c, B7_ERR_INVALID, "%s: %s keeps q = %d paths, the objective %d", who, name(k, nm, sizeof nm), o[k]->ts.q, c->ts.q);
  }
  const int q = c->ts.q;
  const int64_t M = c->ts.M;
  if (q < 1 || q > B7_BATCH_MAX || M < q) return b7_fail(c, B7_ERR_INVALID, "%s: q = %d not in [1, %d] or above the grid's %lld rows", who, q, B7_BATCH_MAX, (long long)M);
  B7_HIP(c, hipSetDevice(c->device));
  const double *buf[TF_YW];
  for (int k = 0; k < n; ++k) buf[k] = (const double *)o[k]->ts_paths.p;
  B7_TRY(streams_order(o, n, true));
  const int rc = tf_pick(c, buf, thresholds, C, M, q, nullptr, key_out, class_out, best_idx1, y_out, reruns_out);
  const int rc2 = streams_order(o, n, false);
  return rc != B7_OK ? rc : rc2;
}

int b7_ts_feas_compute(b7_ctx *c, const double *f, const double *cvals, const double *thresholds, int64_t M1, int q, int C, double *viol_out,
                       double *key_out, int *class_out, int64_t *best_idx1) {
  const char *who = "ts_feas_compute";
  if (!c) return B7_ERR_INVALID;
  if (!f || !key_out || !class_out || !best_idx1)
    return b7_fail(c, B7_ERR_INVALID, "%s: NULL argument (f, key_out, class_out and best_idx1 are needed)", who);
  B7_TRY(tf_thresholds(c, who, thresholds, C));
  if (C > 0 && !cvals) return b7_fail(c, B7_ERR_INVALID, "%s: cvals is NULL with C = %d constraints", who, C);
  if (q < 1 || q > B7_BATCH_MAX) return b7_fail(c, B7_ERR_INVALID, "%s: q = %d not in [1, %d]", who, q, B7_BATCH_MAX);
  if (M1 < q) return b7_fail(c, B7_ERR_INVALID, "%s: M1 = %lld rows are fewer than q = %d paths", who, (long long)M1, q);
  B7_HIP(c, hipSetDevice(c->device));
  const size_t n = (size_t)M1 * q;
  B7_TRY(b7_ensure(c, c->ts_feas_user, sizeof(double) * n * (size_t)(2 + C)));  // a buffer of its own: the kept paths stay
  double *fd = (double *)c->ts_feas_user.p, *vd = fd + n * (size_t)(1 + C);
  B7_HIP(c, hipMemcpyAsync(fd, f, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  if (C > 0) B7_HIP(c, hipMemcpyAsync(fd + n, cvals, sizeof(double) * n * C, hipMemcpyHostToDevice, c->stream));
  const double *buf[TF_YW];
  for (int k = 0; k <= C; ++k) buf[k] = fd + n * k;
  B7_TRY(tf_pick(c, buf, thresholds, C, M1, q, viol_out ? vd : nullptr, key_out, class_out, best_idx1, nullptr, nullptr));
  if (viol_out) {
    B7_HIP(c, hipMemcpyAsync(viol_out, vd, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    B7_HIP(c, hipStreamSynchronize(c->stream));
  }
  return B7_OK;
}

}  // extern "C"
