// Trust-region nomination (TuRBO: Eriksson, Pearce, Gardner, Turner & Poloczek, NeurIPS 2019): the device map that turns a
// resident grid of base points u in [0, 1) into a candidate set inside a box around the best observation, and the host-only
// arithmetic both host languages share: the box from the ARD lengthscales (b7_tr_box) and the success / failure counters that
// resize it (b7_tr_init / b7_tr_update).  No counterpart in the reference.
//
// The map, per element (row i, column k), g = row_offset + i:
//   rotation   t = u + shift[k]; if (t >= 1.0) t -= 1.0;                       (Cranley-Patterson; only with a shift)
//   mask       perturbed iff counter_uniform(counter_key(seed, 0), g d + k) < prob, or k == f(g),
//              f(g) = min(d - 1, (int)(counter_uniform(counter_key(seed, 1), g) * d))
//   value      perturbed: x = t * (hi[k] + (-lo[k])); x = x + lo[k]; clamped into [lo[k], hi[k]]     (two rounded operations)
//              otherwise: x = center[k], bit for bit
// DIFFERENCE FROM ERIKSSON ET AL.: they force one column of a row only when the Bernoulli draw perturbed none of it; here column
// f(g) of EVERY row is perturbed, so that an element is a pure function of (seed, g, k) and no reduction runs across a row.  The
// expected number of perturbed columns is 1 + (d - 1) prob instead of d prob + (1 - prob)^d.
//
// The kernel is bound by memory: one read and one write of M d doubles; a thread's accesses are 8 bytes wide and a wave's are
// consecutive along the row-major array.  Row and column of a thread's next element follow from the last by one add and one
// compare each (no division in the loop).  The five per-column vectors (center, lo, span, shift, hi) sit in LDS, loaded once per workgroup.
#pragma clang fp contract(off)
#include <math.h>

#include "b7_internal.h"
#include "counter_rng.h"

namespace {

__global__ void __launch_bounds__(256) trust_region_kernel(double *__restrict__ g, int64_t total, int d, const double *__restrict__ vec,
                                                           int rotate, double prob, uint64_t key_mask, uint64_t key_col,
                                                           int64_t row_offset) {
  __shared__ double scen[B7_MAX_D], slo[B7_MAX_D], sspan[B7_MAX_D], sshift[B7_MAX_D], shi[B7_MAX_D];
  if ((int)threadIdx.x < d) {
    const int k = threadIdx.x;
    scen[k] = vec[k];
    slo[k] = vec[d + k];
    sspan[k] = vec[2 * d + k];
    sshift[k] = rotate ? vec[3 * d + k] : 0.0;
    shi[k] = vec[4 * d + k];
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t drow = stride / d;
  const int dcol = (int)(stride - drow * d);
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t row = e / d;
  int col = (int)(e - row * d);
  const double dd = (double)d;
  for (; e < total; e += stride) {
    const uint64_t gr = (uint64_t)(row_offset + row);
    int f = (int)(counter_uniform(key_col, gr) * dd);
    f = f < d - 1 ? f : d - 1;
    const bool moved = col == f || counter_uniform(key_mask, gr * (uint64_t)d + (uint64_t)col) < prob;
    double x = scen[col];
    if (moved) {
      double t = g[e];
      if (rotate) {
        t = t + sshift[col];
        if (t >= 1.0) t -= 1.0;
      }
      x = t * sspan[col];
      x = x + slo[col];
      const double lo = slo[col], hi = shi[col];
      x = x < lo ? lo : x;
      x = x > hi ? hi : x;
    }
    g[e] = x;
    row += drow;
    col += dcol;
    if (col >= d) {
      col -= d;
      row += 1;
    }
  }
}

}  // namespace

int launch_trust_region(b7_ctx *c, double *grid, int64_t M, int d, const double *vec_dev, bool rotate, double prob, uint64_t seed,
                        int64_t row_offset) {
  PhaseScope ps(c, "trust_region");
  const int64_t total = M * d;
  if (total <= 0) return B7_OK;
  int64_t blocks = (total + 255) / 256;
  const int64_t cap = (int64_t)c->cus * 8;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(trust_region_kernel, dim3((unsigned)blocks), dim3(256), 0, c->stream, grid, total, d, vec_dev, rotate ? 1 : 0,
                     prob, counter_key(seed, 0), counter_key(seed, 1), row_offset);
  B7_HIP(c, hipGetLastError());
  return B7_OK;
}

// ---- host-only ------------------------------------------------------------------------------------------------------------------

extern "C" {

int b7_tr_box(int d, int S, const b7_hyp *hyps, const double *center, double length, const double *mins, const double *maxes,
              double *lo, double *hi) {
  if (d < 1 || d > B7_MAX_D || S < 1 || !hyps || !center || !mins || !maxes || !lo || !hi) return B7_ERR_INVALID;
  if (!(length > 0.0) || !isfinite(length)) return B7_ERR_INVALID;
  double logr[B7_MAX_D], range[B7_MAX_D];
  for (int s = 0; s < S; ++s) {
    if (!hyps[s].lenscale_sq) return B7_ERR_INVALID;
    for (int k = 0; k < d; ++k)
      if (!(hyps[s].lenscale_sq[k] > 0.0) || !isfinite(hyps[s].lenscale_sq[k])) return B7_ERR_INVALID;
  }
  for (int k = 0; k < d; ++k) {
    if (!isfinite(mins[k]) || !isfinite(maxes[k]) || !isfinite(center[k])) return B7_ERR_INVALID;
    range[k] = maxes[k] - mins[k];
    if (!(range[k] > 0.0) || !isfinite(range[k])) return B7_ERR_INVALID;
    if (center[k] < mins[k] || center[k] > maxes[k]) return B7_ERR_INVALID;
  }
  // log r_k = (1/S) sum_s (1/2) log lenscale_sq[s][k] - log range_k: the geometric mean over the samples of the lengthscale
  // relative to the range; sums run in index order
  double mean = 0.0;
  for (int k = 0; k < d; ++k) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += 0.5 * log(hyps[s].lenscale_sq[k]);
    logr[k] = a / (double)S - log(range[k]);
    mean += logr[k];
  }
  mean /= (double)d;
  for (int k = 0; k < d; ++k) {
    const double w = exp(logr[k] - mean);  // prod_k w_k = 1: the box keeps the volume length^d prod range before clipping
    const double half = w * length * range[k] / 2.0;
    const double a = center[k] - half, b = center[k] + half;
    lo[k] = a > mins[k] ? a : mins[k];
    hi[k] = b < maxes[k] ? b : maxes[k];
  }
  return B7_OK;
}

static void tr_reset(b7_tr_state *st) {
  st->length = st->length_init;
  st->best = NAN;  // unset: the next update's minimum is taken as it comes
  st->succ = st->fail = 0;
}

int b7_tr_init(b7_tr_state *st, int d, int q, double length_init, double length_min, double length_max, int succ_tol,
               int fail_tol) {
  if (!st || d < 1 || q < 1 || isnan(length_init) || isnan(length_min) || isnan(length_max)) return B7_ERR_INVALID;
  st->length_init = length_init > 0.0 ? length_init : 0.8;
  st->length_min = length_min > 0.0 ? length_min : 0.0078125;  // 2^-7
  st->length_max = length_max > 0.0 ? length_max : 1.6;
  st->succ_tol = succ_tol > 0 ? succ_tol : 3;
  const int m = d > 4 ? d : 4;
  st->fail_tol = fail_tol > 0 ? fail_tol : (m + q - 1) / q;  // ceil(max(4 / q, d / q))
  if (!isfinite(st->length_init) || !isfinite(st->length_min) || !isfinite(st->length_max) || st->length_init > st->length_max ||
      st->length_init < st->length_min)
    return B7_ERR_INVALID;
  st->restarts = 0;
  tr_reset(st);
  return B7_OK;
}

int b7_tr_update(b7_tr_state *st, const double *y, int q, int *restart_out) {
  if (!st || !y || q < 1) return B7_ERR_INVALID;
  double ymin = NAN;
  for (int i = 0; i < q; ++i)
    if (!isnan(y[i]) && (isnan(ymin) || y[i] < ymin)) ymin = y[i];
  // a NaN never succeeds; the first response after init / a restart sets `best` and counts as a success
  const bool ok = !isnan(ymin) && (isnan(st->best) || ymin < st->best - 1e-3 * fabs(st->best));
  if (ok) {
    st->best = ymin;
    st->succ += 1;
    st->fail = 0;
  } else {
    st->fail += 1;
    st->succ = 0;
  }
  if (st->succ >= st->succ_tol) {
    const double twice = 2.0 * st->length;
    st->length = twice < st->length_max ? twice : st->length_max;
    st->succ = st->fail = 0;
  } else if (st->fail >= st->fail_tol) {
    st->length /= 2.0;
    st->succ = st->fail = 0;
  }
  int restart = 0;
  if (st->length < st->length_min) {
    restart = 1;
    st->restarts += 1;
    tr_reset(st);
  }
  if (restart_out) *restart_out = restart;
  return B7_OK;
}

}  // extern "C"
