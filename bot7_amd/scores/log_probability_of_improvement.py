"""Log probability of improvement, computed by b7_score_logpi.  No counterpart in the reference's scores/.

log PI(mu, var; fmin, xi) = log Phi(z), z = (fmin - mu - xi)/sigma, evaluated so that it neither underflows nor loses the upper
tail (erfc / erfcx branches; csrc/score.hip).  The marginal over hyper samples is log((1/S) sum_s Phi(z_s)) -- a log-sum-exp on
the device, not the mean of the logs.  On the GP of a constraint c_k, with ``fmin`` = the threshold t_k and ``tradeoff`` 0, it is
that constraint's log probability of feasibility log Pr[c_k(x) <= t_k] (Gelbart et al. 2014, Gardner et al. 2014; the log-space
form of Ament et al. 2023): what the constrained nomination adds onto the feasibility column (Context.feas_add_acc).
Constructor and defaults are those of expected_improvement (``tradeoff`` 0.0, ``nFantasies`` 100)."""
import numpy as np

from .expected_improvement import expected_improvement


class log_probability_of_improvement(expected_improvement):
    title = "bot7.scores.log_probability_of_improvement"

    def add_to(self, ctx, Y_obs, config=None):
        config = config or self.config
        fmin = np.asarray(Y_obs, dtype=np.float64).reshape(len(Y_obs), -1).min(axis=0)
        ctx.score_logpi(fmin, config.get("tradeoff") or 0.0)

    def device_spec(self, Y_obs, config=None):
        """Keyword arguments of Context.eval_nominate for this score (b7_score_spec)."""
        return dict(super().device_spec(Y_obs, config), score="logpi")

    @staticmethod
    def compute(ctx, fval, fvar, fmin, tradeoff=0.0):
        """log Phi(z) on caller-provided mean/var (b7_logpi_compute)."""
        return ctx.logpi_compute(fval, fvar, fmin, tradeoff)
