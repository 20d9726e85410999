"""Thompson sampling, computed by b7_ts_nominate.  No counterpart in the reference's scores/.

Not a per-point score: each nominee is the minimiser of one sample path of the posterior (Wilson, Borovitskiy, Terenin, Mostowsky,
Deisenroth, "Efficiently Sampling Functions from Gaussian Process Posteriors", ICML 2020),

    f_j(x) = m + phi(x)' w_j + K(x, X) inv(K) (y - m - Phi(X) w_j - eps_j),

with ``nFeatures`` (default 1024; a multiple of 16) random Fourier features phi of the prior.  Path j is drawn under hyper sample
j mod nSamples, and a path takes its first minimum among the rows no earlier path of the same call took.  There is no score
vector to add, average or download: the bot calls Context.ts_nominate in place of its eval + arg-max.  One GPU, one response
column.

With the dngo model the posterior over the head's weights is a finite Gaussian and the path is exact, f_j(x) = mean + phi(x)' w_j with
w_j ~ N(m, inv(A)): no random features (``nFeatures`` is unused), computed by b7_blr_ts_nominate through dngo.ts_nominate.

With two or three objectives (config.bot.objectives; TSEMO, Bradford, Schweidtmann & Lapkin 2018) every objective's context keeps q
paths of its own (Context.ts_paths) and the first context nominates: path j picks the row whose sampled values improve the
hypervolume of the front plus the earlier picks under path j the most (Context.ts_hvi_nominate; b7_ts_hvi_nominate /
b7_ts_hvi3_nominate).

``refine`` (default off; a dict of starts / iters / eta0) refines every nominee off the grid by descent on its own sample path
(Context.ts_nominate_refine; b7_ts_nominate_refine): a path is an explicit differentiable function of x, and optimising it by
gradient is how Wilson et al. use it.  The bot evaluates and observes the refined points and steals the grid nominees' rows."""
from .abstract import abstract

REFINE_DEFAULTS = {"starts": 16, "iters": 16, "eta0": 1.0 / 16.0}


class thompson_sampling(abstract):
    title = "bot7.scores.thompson_sampling"

    def __init__(self, config=None):
        super().__init__()
        config = dict(config or {})
        config.setdefault("nFeatures", 1024)
        if config.get("refine"):
            config["refine"] = dict(REFINE_DEFAULTS, **(config["refine"] if isinstance(config["refine"], dict) else {}))
        self.config = config

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("thompson_sampling is not a per-point score: there is nothing to add to the accumulator "
                                  "(nominate through Context.ts_nominate)")

    def nominate(self, ctx, hyps, q, seed, config=None, model=None, observed=None, responses=None, candidates=None):
        """q 1-based nominees.  A GP model: over ctx's resident data and grid (Context.ts_nominate).  A dngo model (passed with its
        observations, responses and candidates): exact paths on the head's weight posterior (dngo.ts_nominate), hyps its
        {'alpha', 'beta', 'mean'} tables; nFeatures plays no part."""
        if model is not None and model.class_() == "bot7.models.dngo":
            return model.ts_nominate(observed, responses, candidates, hyps, q, seed)[1]
        config = config or self.config
        return ctx.ts_nominate(hyps, q, n_features=int(config.get("nFeatures") or 1024), seed=seed)[1]

    def nominate_refine(self, ctx, hyps, q, seed, lo, hi, config=None):
        """q nominees refined on their own paths inside the box [lo, hi] -> (1-based grid nominees[q], refined points q x d)
        (Context.ts_nominate_refine).  A GP model over ctx's resident data and grid."""
        config = config or self.config
        ref = dict(REFINE_DEFAULTS, **(config["refine"] if isinstance(config.get("refine"), dict) else {}))
        _, idx, x, _, _ = ctx.ts_nominate_refine(hyps, q, n_features=int(config.get("nFeatures") or 1024), seed=seed, starts=int(ref["starts"]),
                                                 iters=int(ref["iters"]), eta0=float(ref["eta0"]), lo=lo, hi=hi)
        return idx, x

    def nominate_objectives(self, ctxs, hyps, q, seeds, front, ref, config=None):
        """q nominees for len(ctxs) = 2 or 3 objectives -> (hvi[q], 1-based indices[q], y[q x m]).  ctxs[k] holds objective k + 1's
        resident data and the common grid rows; hyps[k] / seeds[k] are its hyper samples and the seed of its paths.  The paths are
        drawn in objective order (Context.ts_paths), then the first context nominates (Context.ts_hvi_nominate)."""
        config = config or self.config
        for ctx, h, seed in zip(ctxs, hyps, seeds):
            ctx.ts_paths(h, q, n_features=int(config.get("nFeatures") or 1024), seed=seed)
        return ctxs[0].ts_hvi_nominate(ctxs[1] if len(ctxs) == 2 else tuple(ctxs[1:]), front, ref)
