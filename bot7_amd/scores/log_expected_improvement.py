"""Log-space expected improvement, computed by b7_score_logei.  No counterpart in the reference's scores/.

log EI(mu, var; fmin, xi) = log(sigma) + log(phi(z) + z * Phi(z)), z = (fmin - mu - xi)/sigma, evaluated so that it never
underflows (Ament et al., "Unexpected Improvements to Expected Improvement", NeurIPS 2023): where the GP is confident that a
candidate is worse than the incumbent EI is exactly 0 and ranks nothing; its logarithm still orders the candidates.  The
marginal over hyper samples is log((1/S) sum_s EI_s) -- a log-sum-exp on the device, not the mean of the logs.  Constructor
and defaults are those of expected_improvement (``tradeoff`` 0.0, ``nFantasies`` 100)."""
import numpy as np

from .expected_improvement import expected_improvement


class log_expected_improvement(expected_improvement):
    title = "bot7.scores.log_expected_improvement"

    def add_to(self, ctx, Y_obs, config=None):
        config = config or self.config
        fmin = np.asarray(Y_obs, dtype=np.float64).reshape(len(Y_obs), -1).min(axis=0)
        ctx.score_logei(fmin, config.get("tradeoff") or 0.0)

    def device_spec(self, Y_obs, config=None):
        """Keyword arguments of Context.eval_nominate for this score (b7_score_spec)."""
        return dict(super().device_spec(Y_obs, config), score="logei")

    @staticmethod
    def compute(ctx, fval, fvar, fmin, tradeoff=0.0):
        """log EI on caller-provided mean/var (b7_logei_compute)."""
        return ctx.logei_compute(fval, fvar, fmin, tradeoff)
