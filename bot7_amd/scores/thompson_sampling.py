"""Thompson sampling, computed by b7_ts_nominate.  No counterpart in the reference's scores/.

Not a per-point score: each nominee is the minimiser of one sample path of the posterior (Wilson, Borovitskiy, Terenin, Mostowsky,
Deisenroth, "Efficiently Sampling Functions from Gaussian Process Posteriors", ICML 2020),

    f_j(x) = m + phi(x)' w_j + K(x, X) inv(K) (y - m - Phi(X) w_j - eps_j),

with ``nFeatures`` (default 1024; a multiple of 16) random Fourier features phi of the prior.  Path j is drawn under hyper sample
j mod nSamples, and a path takes its first minimum among the rows no earlier path of the same call took.  There is no score
vector to add, average or download: the bot calls Context.ts_nominate in place of its eval + arg-max.  One GPU, one response
column, GP models only."""
from .abstract import abstract


class thompson_sampling(abstract):
    title = "bot7.scores.thompson_sampling"

    def __init__(self, config=None):
        super().__init__()
        config = dict(config or {})
        config.setdefault("nFeatures", 1024)
        self.config = config

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("thompson_sampling is not a per-point score: there is nothing to add to the accumulator "
                                  "(nominate through Context.ts_nominate)")

    def nominate(self, ctx, hyps, q, seed, config=None):
        """q 1-based nominees over ctx's resident data and grid (Context.ts_nominate)."""
        config = config or self.config
        return ctx.ts_nominate(hyps, q, n_features=int(config.get("nFeatures") or 1024), seed=seed)[1]
