"""The log of the exact expected hypervolume improvement, computed by b7_logehvi_nominate / b7_logehvi3_nominate.  No counterpart in
the reference's scores/.

expected_hypervolume_improvement in log space (the multi-objective twin of log_expected_improvement; Ament et al., NeurIPS 2023):
the same strips (two objectives) and boxes (three), the same exact marginal over independent models' hyper samples, but every Psi as
log Psi, every difference as log(e^u - e^l) and every sum as a log-sum-exp.  The linear score is exactly 0 wherever the models are sure
a candidate lies outside the improving region, and when every row is, its arg-max is row 1; this one still ranks those rows.  The
marginal log score is left in the first context's accumulator as a log accumulator, so Context.feas_add_acc takes it: constrained
multi-objective nomination composes from feas_reset / feas_add / feas_add_acc / feas_nominate."""
from .expected_hypervolume_improvement import expected_hypervolume_improvement


class log_expected_hypervolume_improvement(expected_hypervolume_improvement):
    title = "bot7.scores.log_expected_hypervolume_improvement"

    def compute(self, *args, **kwargs):
        raise NotImplementedError("log_expected_hypervolume_improvement is not a per-point score of one mean and one variance: it "
                                  "needs the posteriors of two objectives, a front and a reference point (Context.logehvi_compute on "
                                  "host arrays, Context.logehvi_nominate over two kept posteriors)")

    def add_to(self, ctx, Y_obs=None, config=None):
        raise NotImplementedError("log_expected_hypervolume_improvement is not a per-point score: there is nothing to add to the "
                                  "accumulator per hyper sample (nominate through Context.logehvi_nominate)")

    def nominate(self, ctx, other, front, ref, config=None):
        """expected_hypervolume_improvement.nominate by the log score: (log value, 1-based nominee); `other` one context (two
        objectives, Context.logehvi_nominate) or a pair (three, Context.logehvi3_nominate)."""
        if isinstance(other, (tuple, list)):
            if len(other) != 2:
                raise NotImplementedError("log_expected_hypervolume_improvement: %d objectives (two and three are built)" % (1 + len(other)))
            return ctx.logehvi3_nominate(other[0], other[1], front, ref)
        return ctx.logehvi_nominate(other, front, ref)
