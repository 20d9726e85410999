"""The knowledge gradient, computed by b7_kg_nominate.  No counterpart in the reference's scores/.

Not a per-point score of one posterior: the value of a candidate x is the expected decrease of the MINIMUM OF THE POSTERIOR MEAN
after one more, possibly noisy, evaluation at x (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011),

    KG(x) = min_i mu(a_i) - E_Z[min_i (mu(a_i) + b_i(x) Z)],    b_i(x) = cov(f(x), f(a_i)) / sqrt(var(x) + noise),

over a discretisation set A of ``points`` grid rows (default 16, the library's maximum) plus x itself.  It needs no incumbent
f_min, so it stays correct when the observations are noisy.  ``discretisation`` says where A comes from: 'mean' (default) lets the
library take the rows of lowest marginal posterior mean; 'thompson' hands over the minimisers of that many Thompson-sampling
paths (``nFeatures`` random features each).  It needs the posterior covariance against A, which a (mean, variance) pair does not
carry: there is nothing to add to an accumulator per hyper sample, and the bot calls Context.kg_nominate in place of its eval +
arg-max.  One GPU, one response column, GP models only."""
from .abstract import abstract


class knowledge_gradient(abstract):
    title = "bot7.scores.knowledge_gradient"

    def __init__(self, config=None):
        super().__init__()
        config = dict(config or {})
        config.setdefault("points", 16)
        config.setdefault("discretisation", "mean")
        config.setdefault("nFeatures", 1024)
        self.config = config

    def compute(self, *args, **kwargs):
        raise NotImplementedError("knowledge_gradient is not a per-point score of a mean and a variance: it needs the posterior "
                                  "covariance against its discretisation set (nominate through Context.kg_nominate)")

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("knowledge_gradient is not a per-point score: there is nothing to add to the accumulator "
                                  "(nominate through Context.kg_nominate)")

    def nominate(self, ctx, hyps, points=None, rows=None, config=None):
        """(value, 1-based nominee) over ctx's resident data and grid (Context.kg_nominate); rows: the discretisation set's 1-based
        grid rows, or None for the library's own choice of `points` rows."""
        config = config or self.config
        return ctx.kg_nominate(hyps, points=int(points or config.get("points") or 16), rows=rows)
