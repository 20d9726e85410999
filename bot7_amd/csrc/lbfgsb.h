// The host optimiser's internal entry (lbfgsb.hip): b7_lbfgsb_minimize with an optional trace.  No HIP, no context.
#pragma once
#include <vector>

#include "bot7hip.h"

// trace (nullable): one record of n + 2 doubles per accepted iterate, record 0 the start: x | f | the step length that led there
int lbfgsb_run(b7_objective_fn fn, void *user, int n, const double *x0, const double *lo, const double *hi, const b7_lbfgsb_opts *opts,
               double *x_out, double *f_out, double *g_out, int *iters_out, int *evals_out, int *status_out, std::vector<double> *trace);
