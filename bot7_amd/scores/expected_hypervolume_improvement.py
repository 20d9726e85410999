"""The exact two-objective expected hypervolume improvement, computed by b7_ehvi_nominate.  No counterpart in the reference's scores/.

Not a per-point score of one posterior: it values a candidate by the area it is expected to add to what the observed front
dominates inside a reference box (both objectives minimised; Emmerich, Yang & Deutz 2016),

    EHVI(x) = sum_k [Psi(a_k+1; mu1, sigma1) - Psi(a_k; mu1, sigma1)] Psi(b_k; mu2, sigma2),    Psi(a; mu, sigma) = E[(a - y)+],

over the strips of the canonical front (a_k, b_k) (bot7_amd._lib.pareto_front2), marginalised exactly over the hyper samples of TWO
independent models, one per objective.  It needs two posteriors, which one accumulator's (mean, variance) pair does not carry:
each model's context keeps its posterior (Context.eval_posterior) and the bot calls Context.ehvi_nominate in place of its eval +
arg-max.  One GPU, two objectives, independent GP models only."""
from .abstract import abstract


class expected_hypervolume_improvement(abstract):
    title = "bot7.scores.expected_hypervolume_improvement"

    def __init__(self, config=None):
        super().__init__()
        self.config = dict(config or {})

    def compute(self, *args, **kwargs):
        raise NotImplementedError("expected_hypervolume_improvement is not a per-point score of one mean and one variance: it needs "
                                  "the posteriors of two objectives, a front and a reference point (Context.ehvi_compute on host "
                                  "arrays, Context.ehvi_nominate over two kept posteriors)")

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("expected_hypervolume_improvement is not a per-point score: there is nothing to add to the "
                                  "accumulator per hyper sample (nominate through Context.ehvi_nominate)")

    def nominate(self, ctx, other, front, ref, config=None):
        """(value, 1-based nominee) over the kept posteriors of ctx (objective 1) and other (objective 2) (Context.eval_posterior on
        each first), the canonical front P x 2 and the reference point (r1, r2) (Context.ehvi_nominate)."""
        return ctx.ehvi_nominate(other, front, ref)
