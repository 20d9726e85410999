"""Max-value entropy search, computed by b7_score_mes.  No counterpart in the reference's scores/.

The expected reduction of the entropy of the optimum's VALUE (Wang & Jegelka, "Max-value Entropy Search for Efficient Bayesian
Optimization", ICML 2017).  The library minimises, so the value is the minimum y*; its distribution is that of the minimum over the
resident candidates under each hyper sample, and ``nLevels`` (default 8) of its quantiles y*_k are found on the device by a
deterministic search -- no sampler, no random numbers.  With g = (mu - y*_k)/sigma,

    score = (1/K) sum_k [ g phi(g) / (2 Phi(g)) - log Phi(g) ]

averaged over the hyper samples like EI.  Rows with var == 0 score 0.0; rows with a NaN or a negative variance score NaN.  One
response column only: pending points (fantasies) are not supported."""
from .abstract import abstract


class max_value_entropy_search(abstract):
    title = "bot7.scores.max_value_entropy_search"

    def __init__(self, config=None):
        super().__init__()
        config = dict(config or {})
        config.setdefault("nLevels", 8)
        self.config = config

    def add_to(self, ctx, Y_obs=None, config=None):
        config = config or self.config
        ctx.mes_set_levels(config.get("nLevels") or 8)
        ctx.score_mes()

    def device_spec(self, Y_obs=None, config=None):
        """Keyword arguments of Context.eval_nominate for this score (b7_score_spec); the context's level count is the caller's
        to set (Context.mes_set_levels(config.nLevels)): ``levels`` rides along for that."""
        config = config or self.config
        return dict(score="mes", levels=int(config.get("nLevels") or 8))

    @staticmethod
    def compute(ctx, fval, fvar, ystar):
        """The score on caller-provided mean / var with the caller's y* (b7_mes_compute)."""
        return ctx.mes_compute(fval, fvar, ystar)
