"""Constrained Thompson sampling, computed by b7_ts_paths and b7_ts_feas_nominate.  No counterpart in the reference's scores/.

The selection rule of SCBO (Eriksson & Poloczek, "Scalable Constrained Bayesian Optimization", AISTATS 2021).  Not a per-point score:
the objective's model and every constraint's model keep q sample paths each (thompson_sampling's paths, ``nFeatures`` random Fourier
features, default 1024; a multiple of 16), drawn with a seed of their own, and under the joint path (f_j, c_1j .. c_Cj) nominee j is

    the row of lowest f_j among the rows where every c_kj <= t_k,
    or, where path j sees no such row, the row of smallest total violation sum_k max(c_kj - t_k, 0),

over the rows no earlier path of the same call took.  There is no feasibility weight, no incumbent and no special case while nothing
feasible has been observed; any config.bot.batch up to 16.  One GPU, GP models."""
from .abstract import abstract


class constrained_thompson_sampling(abstract):
    title = "bot7.scores.constrained_thompson_sampling"

    def __init__(self, config=None):
        super().__init__()
        config = dict(config or {})
        config.setdefault("nFeatures", 1024)
        self.config = config

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("constrained_thompson_sampling is not a per-point score: there is nothing to add to the accumulator "
                                  "(nominate through Context.ts_paths and Context.ts_feas_nominate)")

    def nominate_constrained(self, ctxs, hyps, q, seeds, thresholds, config=None):
        """q nominees under len(ctxs) - 1 constraints -> Context.ts_feas_nominate's dict.  ctxs[0] holds the objective's resident data
        and the common grid rows, ctxs[k] constraint k's; hyps[k] / seeds[k] are that model's hyper samples and the seed of its paths.
        The paths are drawn in that order (Context.ts_paths), then the first context nominates (Context.ts_feas_nominate)."""
        config = config or self.config
        for ctx, h, seed in zip(ctxs, hyps, seeds):
            ctx.ts_paths(h, q, n_features=int(config.get("nFeatures") or 1024), seed=seed)
        return ctxs[0].ts_feas_nominate(list(ctxs[1:]), thresholds)
