// A projected limited-memory BFGS with box bounds: host code only (no kernel, no context, no GPU), shared by both host languages
// the way b7_tr_update is.  No counterpart in the reference.
//
//   memory 8, two-loop recursion over the FREE components; a pair (s, y) is kept only where s'y > 1e-10 |s| |y|, and a skipped
//   pair empties the memory (the next direction is the steepest descent)
//   a component at a bound whose gradient points out of the box (and every component with lo == hi) is held for the step
//   the trial point is the projection of x + t dir onto the box, t = 1, 1/2, .. (at most 20 halvings), accepted by Armijo's test on
//   the projected step, f(x+) <= f(x) + 1e-4 g'(x+ - x); a non-finite value or gradient is a failed trial point
//   a quasi-Newton direction that is no descent direction, or whose search finds nothing, is replaced once by the projected
//   steepest descent (memory dropped); when that finds nothing either the run ends with B7_LBFGSB_LINESEARCH
// Every accepted step lowers f, so the result is never worse than x0.  No random numbers; every sum runs in ascending index order.
#include "lbfgsb.h"

#include <math.h>
#include <string.h>

#include <memory>

namespace {

constexpr int MEM = 8, NMAX = 99, HALVINGS = 20;
constexpr double C1 = 1e-4, CURV = 1e-10;

inline bool fin(double x) { return x - x == 0.0; }

struct Work {
  int n;
  const double *lo, *hi;
  double s[MEM][NMAX], y[MEM][NMAX], rho[MEM];
  int count = 0, head = 0;  // pairs kept; slot of the oldest
  bool held[NMAX];
};

double dot_free(const Work &w, const double *a, const double *b) {
  double r = 0.0;
  for (int i = 0; i < w.n; ++i)
    if (!w.held[i]) r += a[i] * b[i];
  return r;
}

// the components the step may not move: fixed ones, and those at an active bound whose gradient points outward
void hold(Work &w, const double *x, const double *g) {
  for (int i = 0; i < w.n; ++i)
    w.held[i] = w.lo[i] == w.hi[i] || (x[i] <= w.lo[i] && g[i] > 0.0) || (x[i] >= w.hi[i] && g[i] < 0.0);
}

// dir = -H g over the free components (two-loop recursion, newest pair first), 0 in the held ones
void direction(const Work &w, const double *g, double *dir) {
  double q[NMAX], a[MEM];
  for (int i = 0; i < w.n; ++i) q[i] = w.held[i] ? 0.0 : g[i];
  for (int k = w.count - 1; k >= 0; --k) {
    const int j = (w.head + k) % MEM;
    a[k] = w.rho[j] * dot_free(w, w.s[j], q);
    for (int i = 0; i < w.n; ++i)
      if (!w.held[i]) q[i] -= a[k] * w.y[j][i];
  }
  if (w.count > 0) {
    const int j = (w.head + w.count - 1) % MEM;
    const double yy = dot_free(w, w.y[j], w.y[j]), sy = dot_free(w, w.s[j], w.y[j]);
    const double gamma = (yy > 0.0 && sy > 0.0) ? sy / yy : 1.0;
    for (int i = 0; i < w.n; ++i) q[i] *= gamma;
  }
  for (int k = 0; k < w.count; ++k) {
    const int j = (w.head + k) % MEM;
    const double b = w.rho[j] * dot_free(w, w.y[j], q);
    for (int i = 0; i < w.n; ++i)
      if (!w.held[i]) q[i] += (a[k] - b) * w.s[j][i];
  }
  for (int i = 0; i < w.n; ++i) dir[i] = w.held[i] ? 0.0 : -q[i];
}

void remember(Work &w, const double *s, const double *y) {
  double ss = 0.0, yy = 0.0, sy = 0.0;
  for (int i = 0; i < w.n; ++i) ss += s[i] * s[i], yy += y[i] * y[i], sy += s[i] * y[i];
  if (!(sy > CURV * sqrt(ss) * sqrt(yy))) {  // also refuses a NaN
    // no positive curvature along the step (Armijo's test alone does not ask for it): the kept pairs describe another neighbourhood,
    // and a model frozen on them crawls; start the memory again from the steepest descent
    w.count = 0, w.head = 0;
    return;
  }
  int j;
  if (w.count < MEM) {
    j = (w.head + w.count) % MEM;
    w.count += 1;
  } else {
    j = w.head;
    w.head = (w.head + 1) % MEM;
  }
  memcpy(w.s[j], s, sizeof(double) * w.n);
  memcpy(w.y[j], y, sizeof(double) * w.n);
  w.rho[j] = 1.0 / sy;
}

}  // namespace

int lbfgsb_run(b7_objective_fn fn, void *user, int n, const double *x0, const double *lo, const double *hi, const b7_lbfgsb_opts *opts,
               double *x_out, double *f_out, double *g_out, int *iters_out, int *evals_out, int *status_out, std::vector<double> *trace) {
  if (!fn || !x0 || !lo || !hi || !x_out || n < 1 || n > NMAX) return B7_ERR_INVALID;
  for (int i = 0; i < n; ++i)
    if (!fin(x0[i]) || !(lo[i] <= hi[i]) || !(x0[i] >= lo[i]) || !(x0[i] <= hi[i])) return B7_ERR_INVALID;
  const int max_iters = (opts && opts->max_iters >= 0) ? opts->max_iters : 50;
  const int max_evals = (opts && opts->max_evals > 0) ? opts->max_evals : 0;  // 0: no cap of its own
  const double gtol_abs = (opts && opts->gtol > 0.0) ? opts->gtol : 0.0;
  const std::unique_ptr<Work> wp(new Work);  // 13 KiB: off the caller's stack
  Work &w = *wp;
  w.n = n, w.lo = lo, w.hi = hi;
  double x[NMAX], g[NMAX], xt[NMAX], gt[NMAX], dir[NMAX], sv[NMAX], yv[NMAX];
  double f = NAN, ft = NAN;
  int iters = 0, evals = 0, status = 0;
  memcpy(x, x0, sizeof(double) * n);
  for (int i = 0; i < n; ++i) g[i] = NAN;
  auto record = [&](double step) {
    if (!trace) return;
    trace->insert(trace->end(), x, x + n);
    trace->push_back(f);
    trace->push_back(step);
  };
  auto all_finite = [&](double fv, const double *gv) {
    bool ok = fin(fv);
    for (int i = 0; i < n; ++i) ok = ok && fin(gv[i]);
    return ok;
  };
  if (trace) trace->clear();
  evals = 1;
  if (fn(user, n, x, &f, g) != 0)
    status |= B7_LBFGSB_STOPPED;
  else if (!all_finite(f, g))
    status |= B7_LBFGSB_BAD_START;
  record(0.0);
  while (status == 0) {
    hold(w, x, g);
    double pg = 0.0;
    for (int i = 0; i < n; ++i)
      if (!w.held[i] && fabs(g[i]) > pg) pg = fabs(g[i]);
    const double af = fabs(f);
    if (pg <= (gtol_abs > 0.0 ? gtol_abs : 1e-5 * (af > 1.0 ? af : 1.0))) {
      status |= B7_LBFGSB_CONVERGED;
      break;
    }
    if (iters >= max_iters) {
      status |= B7_LBFGSB_MAX_ITERS;
      break;
    }
    bool accepted = false;
    double step = 0.0;
    // attempt 0: the quasi-Newton direction, where there is a memory; attempt 1: the projected steepest descent, memory dropped
    for (int attempt = w.count > 0 ? 0 : 1; attempt < 2 && !accepted && status == 0; ++attempt) {
      if (attempt == 0) {
        direction(w, g, dir);
        if (!(dot_free(w, dir, g) < 0.0)) continue;  // not a descent direction (or NaN)
      } else {
        w.count = 0, w.head = 0;
        for (int i = 0; i < n; ++i) dir[i] = w.held[i] ? 0.0 : -g[i];
      }
      double t = 1.0;
      for (int h = 0; h <= HALVINGS && status == 0; ++h, t *= 0.5) {
        bool moved = false;
        double slope = 0.0;
        for (int i = 0; i < n; ++i) {
          double v = x[i] + t * dir[i];
          v = v < lo[i] ? lo[i] : (v > hi[i] ? hi[i] : v);
          if (w.held[i]) v = x[i];
          xt[i] = v;
          moved = moved || v != x[i];
          slope += g[i] * (v - x[i]);
        }
        if (!moved) break;  // the step has shrunk below the spacing of the doubles around x
        if (max_evals > 0 && evals >= max_evals) {
          status |= B7_LBFGSB_MAX_EVALS;
          break;
        }
        evals += 1;
        if (fn(user, n, xt, &ft, gt) != 0) {
          status |= B7_LBFGSB_STOPPED;
          break;
        }
        if (all_finite(ft, gt) && ft <= f + C1 * slope && ft <= f) {
          accepted = true;
          step = t;
          break;
        }
      }
    }
    if (status != 0) break;
    if (!accepted) {
      status |= B7_LBFGSB_LINESEARCH;
      break;
    }
    for (int i = 0; i < n; ++i) sv[i] = xt[i] - x[i], yv[i] = gt[i] - g[i];
    remember(w, sv, yv);
    memcpy(x, xt, sizeof(double) * n);
    memcpy(g, gt, sizeof(double) * n);
    f = ft;
    iters += 1;
    record(step);
  }
  memcpy(x_out, x, sizeof(double) * n);
  if (f_out) *f_out = f;
  if (g_out) memcpy(g_out, g, sizeof(double) * n);
  if (iters_out) *iters_out = iters;
  if (evals_out) *evals_out = evals;
  if (status_out) *status_out = status;
  return B7_OK;
}

extern "C" {

int b7_lbfgsb_default_opts(b7_lbfgsb_opts *o) {
  if (!o) return B7_ERR_INVALID;
  o->max_iters = 50;
  o->max_evals = 0;
  o->gtol = 0.0;
  return B7_OK;
}

int b7_lbfgsb_minimize(b7_objective_fn fn, void *user, int n, const double *x0, const double *lo, const double *hi,
                       const b7_lbfgsb_opts *opts, double *x_out, double *f_out, double *g_out, int *iters_out, int *evals_out,
                       int *status_out) {
  return lbfgsb_run(fn, user, n, x0, lo, hi, opts, x_out, f_out, g_out, iters_out, evals_out, status_out, nullptr);
}

}  // extern "C"
