"""The exact two-objective expected hypervolume improvement, computed by b7_ehvi_nominate.  No counterpart in the reference's scores/.

Not a per-point score of one posterior: it values a candidate by the area it is expected to add to what the observed front
dominates inside a reference box (both objectives minimised; Emmerich, Yang & Deutz 2016),

    EHVI(x) = sum_k [Psi(a_k+1; mu1, sigma1) - Psi(a_k; mu1, sigma1)] Psi(b_k; mu2, sigma2),    Psi(a; mu, sigma) = E[(a - y)+],

over the strips of the canonical front (a_k, b_k) (bot7_amd._lib.pareto_front2), marginalised exactly over the hyper samples of TWO
independent models, one per objective.  It needs two posteriors, which one accumulator's (mean, variance) pair does not carry:
each model's context keeps its posterior (Context.eval_posterior) and the bot calls Context.ehvi_nominate in place of its eval +
arg-max.  One GPU, independent GP models only.

With THREE objectives (nominate's `other` a pair of contexts) the strips have no counterpart; the region no front point dominates is
cut into boxes [l_b, u_b] first (bot7_amd._lib.nondominated_boxes3) and

    EHVI(x) = sum_b prod_m [Psi_m(u_bm) - Psi_m(l_bm)],    Psi(-inf) = 0,

marginalised exactly, box by box and objective by objective, by Context.ehvi3_nominate.  Four or more objectives are not built."""
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
        each first), the canonical front P x 2 and the reference point (r1, r2) (Context.ehvi_nominate).  `other` may be a pair
        (objective 2's context, objective 3's): three objectives, front P x 3, ref (r1, r2, r3) (Context.ehvi3_nominate)."""
        if isinstance(other, (tuple, list)):
            # THREE objectives: other = (objective 2's context, objective 3's), front P x 3 (bot7_amd._lib.pareto_front3), ref
            # (r1, r2, r3): the sum over the boxes of the non-dominated region (Context.ehvi3_nominate)
            if len(other) != 2:
                raise NotImplementedError("expected_hypervolume_improvement: %d objectives (two and three are built)" % (1 + len(other)))
            return ctx.ehvi3_nominate(other[0], other[1], front, ref)
        return ctx.ehvi_nominate(other, front, ref)
