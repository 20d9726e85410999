"""bot7.bots.bayesopt (bots/bayesopt.lua): MC-marginalised acquisition over GP hyper samples, then arg-max.

eval (bots/bayesopt.lua:56-82) keeps the reference's arithmetic -- score = zeros(M); per hyper sample
score:add(acq); score:div(nSamples) -- but the accumulator lives on the GPU (b7_score_reset / _ei|_cb /
_finish) so no M-vector crosses PCIe per sample; nominate (:85-99) takes the arg-max from the same finish call
(score:max(1): first maximum, 1-based).  When only the winner is wanted (nominate) and the score has a device
spec, the whole of eval + max is ONE library call, b7_eval_nominate: same hyper samples, same arithmetic, one host
synchronisation instead of one per sample (config.bot.fused, default True).

config.score.type picks the score from bot7_amd.scores.registry and every path below takes whatever it names: the registry's
'log_expected_improvement' (log-space EI, not in the reference) travels as score="logei" in the device spec -- fused, sharded and
group nominations alike -- and as b7_score_logei in the per-sample loop, where score_finish's division is the log accumulator's
subtraction of log(nSamples).  'max_value_entropy_search' (not in the reference either) travels as score="mes" with its
level count (config.score.nLevels) and as b7_score_mes in the per-sample loop, each hyper sample with its own y* search on the
device; on one GPU only -- a sharded candidate set or a batch (config.bot.batch > 1) answers "unsupported".
'thompson_sampling' (not in the reference) is not a per-point score: nominate and nominate_batch, q = 1 included, go through
b7_ts_nominate with a seed from the bot's own generator, and eval(want_scores=True) raises -- there is no score vector.  With
the dngo model the same calls go through b7_blr_ts_nominate: exact paths on the head's weight posterior, under the head's point
hypers or config.model.hyps, a list of {'alpha', 'beta', 'mean'} tables.
'knowledge_gradient' (not in the reference) is a policy too: eval and nominate go through b7_kg_nominate with config.score.points
discretisation rows (default 16), chosen by config.score.discretisation: 'mean' (default; the library takes the rows of lowest
marginal posterior mean) or 'thompson' (the minimisers of that many b7_ts_nominate paths, drawn with a seed from the bot's own
generator, are handed over).  What is not built is refused by name (kg_refusal, refine_refusal, constraint_refusal).

config.bot.refine (ours; False = the reference's loop, untouched) is a dict of starts / iters / eta0: a model-based trial then goes
through b7_eval_nominate_refine, which climbs the marginalised acquisition from the best grid rows inside the grid's box
(config.grid.mins / maxes); the trial steals the grid row the winner started from, evaluates the objective at the refined point
and observes that point.  What the library refuses is refused here by name (refine_refusal).

config.score.refine (ours; absent = today's loop) under config.score.type = 'thompson_sampling' is the same dict for THOMPSON
nominees: a model-based trial goes through b7_ts_nominate_refine, which lets every path's nominee descend on its own sample path
(a path, unlike the acquisition, is an explicit differentiable function of x); the trial steals the q grid nominees' rows, evaluates
the objective at the refined points and observes those.  With config.bot.trust_region the box is the trial's trust region.  What is
not built is refused by name (ts_refine_refusal); config.bot.refine with thompson_sampling stays refused.

config.bot.constraints (ours; None = the reference's loop, untouched) is a list of {"threshold": t, "model": {...}}: CONSTRAINED
nomination after Gelbart et al. 2014 / Gardner et al. 2014.  The objective returns a row [y, c_1 .. c_C]; the objective's model sees
column 0, constraint model k -- a GP with a context and sampler state of its own -- column k.  Per model-based trial every
constraint model samples its hypers, stages data and grid on its context and leaves log Pr[c_k(x) <= t_k], marginalised over its
samples, in that context's accumulator (eval_nominate(score="logpi", fmin=[t_k], tradeoff=0)); the objective's context sums them
into its feasibility column (feas_reset, feas_add_acc) and nominates with the weight (eval_nominate_feasible), fmin being the best
response among the rows that satisfy every constraint -- or, while no row does, by feasibility alone (feas_nominate).  The stolen
row leaves every context's resident grid.  What is not built is refused by name (constraint_refusal).

A constraint with "binary": True (ours) is one observed only as an OUTCOME -- a run diverged, ran out of memory, returned NaN: its
response column holds 0 (satisfied) or 1 (violated), its threshold is 0.5 (so feasible_rows / best_feasible_fmin read it as they are)
and its model is a gp_classifier, a probit GP by Laplace's method (Gelbart et al. 2014, section 2.3), which leaves the same log
accumulator through clf_eval_logfeas instead of eval_nominate(score="logpi").  The objective need not exist where such a constraint
is violated: with a binary constraint present, observed rows whose objective is not finite are left out of the OBJECTIVE model's data
(objective_rows); they stay in every constraint model's.  constrained_thompson_sampling refuses a binary constraint by name.

config.score.type = 'constrained_thompson_sampling' with config.bot.constraints is CONSTRAINED THOMPSON SAMPLING (the selection rule of
SCBO: Eriksson & Poloczek 2021), for any config.bot.batch from 1 to 16: per model-based trial the objective's model and every
constraint's model sample their hypers, stage their column on their own context and keep config.bot.batch sample paths (ts_paths, a
distinct seed from the bot's generator each); the objective's context nominates (ts_feas_nominate): path j takes the row of lowest
f_j among the rows where every c_kj <= t_k, or the row of smallest total violation where its paths see no feasible row.  No fmin, no
feasibility column.  The stolen rows leave every context's grid; last_constrained keeps hyps, seeds, thresholds, the picks, their
classes, keys and values, and the rerun count.  What is not built is refused by name (constrained_thompson_refusal).

config.bot.objectives (ours; None = the reference's loop, untouched) is {"ref": [r1, r2] | None, "model": {...}}: TWO-OBJECTIVE
nomination by the exact expected hypervolume improvement (Emmerich, Yang & Deutz 2016; config.score.type =
'expected_hypervolume_improvement', a policy like the knowledge gradient).  The objective returns a row [y1, y2], both minimised;
the bot's own model sees column 0, a second gp_regressor -- with a context and sampler state of its own -- column 1.  Per
model-based trial both models sample their hypers, both contexts keep their posterior (eval_posterior), the front of the
observations comes from pareto_front2 and the objective's context nominates (ehvi_nominate); the stolen row leaves both grids.
ref = None recomputes the reference point every trial as the per-column maximum of the observations plus 10 % of the column's
range (default_ref).  update_best / progress_report report the hypervolume and the front's size.  What is not built is refused
by name (objectives_refusal).
config.bot.objectives = {"ref": [r1, r2, r3] | None, "models": [{...}, {...}]} means THREE objectives: the objective returns a row
[y1, y2, y3], the two further gp_regressors -- each with a context and sampler state of its own -- see columns 1 and 2, the front
comes from pareto_front3 and the objective's context nominates over the boxes of the non-dominated region (ehvi3_nominate); the
stolen row leaves all three grids; the reports carry hypervolume3.  Four or more objectives, and with three also trust regions,
are refused by name (objectives3_refusal).
config.score.type = 'log_expected_hypervolume_improvement' runs the same trials, two or three objectives, by the LOG score
(logehvi_nominate / logehvi3_nominate): it still ranks the candidates where the linear score is 0 in every row -- a fixed ref that no
observation has reached yet, late trials, a large grid -- and the linear arg-max would take row 1.  last_objectives["value"] is then
the log value.  Everything refused with the linear type is refused with this one.

config.score.type = 'thompson_sampling' with either config.bot.objectives form is MULTI-OBJECTIVE THOMPSON SAMPLING (TSEMO: Bradford,
Schweidtmann & Lapkin 2018), for any config.bot.batch >= 1: per model-based trial every objective's model samples its hypers, stages
its column on its own context and keeps config.bot.batch sample paths (ts_paths, a seed from the bot's generator each, in objective
order); the first context nominates (ts_hvi_nominate): path j takes the row whose sampled values improve the hypervolume of the
observations' front plus the earlier picks under path j the most.  The stolen rows leave every objective's grid; last_objectives keeps
hyps, seeds, ref, front, the picks and their hvi.  Everything else refused with objectives stays refused.

config.bot.trust_region (ours; None = the reference's loop, untouched) is a dict of length_init / length_min / length_max /
success_tolerance / failure_tolerance / perturb / base: TRUST-REGION nomination (TuRBO-1: Eriksson et al. 2019).  No grid is made
up front; config.grid.size is the number of candidates per trial.  Per model-based trial the hyper samples are drawn on the
observations since the last restart, the box around the best of them comes from tr_box, a fresh base grid ('sobol', rotated, or
'random') is made on the device and mapped into the box (grid_trust_region), and the nomination goes through the branches above
unchanged on a ResidentGrid handle; the nominees' rows are downloaded, nothing is stolen, and the q responses resize the box
(TrustRegionState.update).  A restart moves the model's window, not the record.  self.tr_trace keeps a record per trial.  What is not
built is refused by name (trust_region_refusal)."""
import numpy as np

from .abstract import abstract
from .. import tensor as T
from bot7_amd.grids.abstract import DeviceGrid, ResidentGrid
from bot7_amd import models as Models
from bot7_amd import scores as Scores


REFINE_DEFAULTS = {"starts": 16, "iters": 16, "eta0": 1.0 / 16.0}


def refine_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot refine its nominee off the grid (b7_eval_nominate_refine's own refusals, by name), or None."""
    if int(config["bot"].get("batch", 1)) > 1:
        return "config.bot.refine with config.bot.batch > 1: refinement of a batch is not built"
    if sharded:
        return "config.bot.refine over sharded candidates: refinement over a sharded grid is not built"
    if model_class == "bot7.models.dngo":
        return "config.bot.refine with the dngo model: the Bayesian-linear head has no gradient kernels"
    kind = config["score"]["type"]
    if kind == "thompson_sampling":
        return "config.bot.refine with thompson_sampling: a sample path is not a per-point score"
    if kind == "max_value_entropy_search":
        return "config.bot.refine with max_value_entropy_search: the score has no gradient piece"
    if kind == "knowledge_gradient":
        return "config.bot.refine with knowledge_gradient: refinement of a knowledge-gradient nominee is not built"
    return None


def ts_refine_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot refine its Thompson nominees on their sample paths (config.score.refine; what
    b7_ts_nominate_refine and _run_trial_ts_refined do not do, by name), or None."""
    if not config["score"].get("refine"):
        return None
    kind = config["score"]["type"]
    if kind == "knowledge_gradient":
        return "config.score.refine with knowledge_gradient: the rows of the Thompson discretisation are grid rows (their refinement is not built)"
    if kind != "thompson_sampling":
        return "config.score.refine with %s: it refines thompson_sampling's nominees on their sample paths (config.bot.refine climbs a per-point score)" % kind
    if config["bot"].get("refine"):
        return refine_refusal(config, model_class, sharded)
    if sharded:
        return "config.score.refine over sharded candidates or a group: refinement of sample paths over a sharded grid is not built"
    if model_class == "bot7.models.dngo":
        return "config.score.refine with the dngo model: the gradient of the head's exact paths (the basis network's Jacobian) is not built"
    if config["bot"].get("constraints"):
        return "config.score.refine with config.bot.constraints: refinement of a constrained nominee is not built"
    if config["bot"].get("objectives"):
        return "config.score.refine with config.bot.objectives: refinement of a multi-objective nominee is not built"
    q = int(config["bot"].get("batch", 1))
    if q > TS_REFINE_BATCH_MAX:
        return "config.score.refine with config.bot.batch = %d: at most %d nominees per trial are built" % (q, TS_REFINE_BATCH_MAX)
    ref = config["score"]["refine"]
    unknown = sorted(set(ref) - set(REFINE_DEFAULTS)) if isinstance(ref, dict) else []
    if unknown:
        return "config.score.refine with unknown entries %s: %s are read" % (", ".join(unknown), ", ".join(sorted(REFINE_DEFAULTS)))
    return None


TS_REFINE_BATCH_MAX = 16   # B7_BATCH_MAX
CONSTRAINED_SCORES = ("expected_improvement", "log_expected_improvement", "log_probability_of_improvement")
CONSTRAINED_THOMPSON = "constrained_thompson_sampling"   # q nominees per trial from joint sample paths (b7_ts_feas_nominate)


def constrained_thompson_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate by constrained Thompson sampling (what b7_ts_feas_nominate does not do, by name), or
    None.  Any config.bot.batch up to BATCH_MAX passes."""
    kind = CONSTRAINED_THOMPSON
    cons = config["bot"].get("constraints")
    if not cons:
        return "%s without config.bot.constraints: the policy needs a constraint, each with a model of its own" % kind
    if config["bot"].get("refine"):
        return "%s with config.bot.refine: refinement of a constrained nominee is not built" % kind
    if config["bot"].get("objectives"):
        return "%s with config.bot.objectives: constraints combined with objectives are not built" % kind
    if config["bot"].get("trust_region"):
        return "%s with config.bot.trust_region: constraints inside a trust region (SCBO's outer loop) are not built" % kind
    if sharded:
        return "%s over sharded candidates: constrained Thompson sampling over a sharded grid is not built" % kind
    if model_class == "bot7.models.dngo":
        return "%s with the dngo model: joint paths with the Bayesian-linear head are not built" % kind
    for k, con in enumerate(cons):
        if con.get("binary"):
            return "%s with config.bot.constraints[%d] binary: sample paths of a classifier's latent are not built (binary constraints " \
                   "nominate through the feasibility weight)" % (kind, k)
        if (con.get("model") or {}).get("type", "gp_regressor") != "gp_regressor":
            return "%s with config.bot.constraints[%d] on the %s model: a constraint is modelled by a gp_regressor" % (kind, k, con["model"]["type"])
    if len(cons) > TS_FEAS_CMAX:
        return "%s with %d constraints: at most %d are built" % (kind, len(cons), TS_FEAS_CMAX)
    q = int(config["bot"].get("batch", 1))
    if q > BATCH_MAX:
        return "%s with config.bot.batch = %d: at most %d nominees per trial are built" % (kind, q, BATCH_MAX)
    return None


def constraint_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate under config.bot.constraints (what b7_eval_nominate_feasible does not do, by name), or
    None.  config.score.type = 'constrained_thompson_sampling' is judged by constrained_thompson_refusal."""
    if config["score"]["type"] == CONSTRAINED_THOMPSON:
        return constrained_thompson_refusal(config, model_class, sharded)
    if int(config["bot"].get("batch", 1)) > 1:
        return "config.bot.constraints with config.bot.batch > 1: feasibility-weighted believer batches are not built"
    if config["bot"].get("refine"):
        return "config.bot.constraints with config.bot.refine: refinement of a constrained nominee is not built"
    if sharded:
        return "config.bot.constraints over sharded candidates: constrained nomination over a sharded grid is not built"
    if model_class == "bot7.models.dngo":
        return "config.bot.constraints with the dngo model: the Bayesian-linear head has no feasibility weight"
    kind = config["score"]["type"]
    if kind == "thompson_sampling":
        return "config.bot.constraints with thompson_sampling: a sample path has no feasibility weight (%s nominates from joint paths)" \
            % CONSTRAINED_THOMPSON
    if kind == "confidence_bound":
        return "config.bot.constraints with confidence_bound: a signed score has no product form with a feasibility weight"
    if kind == "max_value_entropy_search":
        return "config.bot.constraints with max_value_entropy_search: the score has no feasibility weight"
    if kind == "knowledge_gradient":
        return "config.bot.constraints with knowledge_gradient: the knowledge gradient has no feasibility weight"
    if kind not in CONSTRAINED_SCORES:
        return "config.bot.constraints with %s: only %s are built" % (kind, ", ".join(CONSTRAINED_SCORES))
    for k, con in enumerate(config["bot"]["constraints"]):
        why = binary_refusal(k, con)
        if why:
            return why
        if not con.get("binary") and (con.get("model") or {}).get("type", "gp_regressor") != "gp_regressor":
            return "config.bot.constraints[%d] with the %s model: a constraint is modelled by a gp_regressor" % (k, con["model"]["type"])
    return None


def binary_refusal(k, con):
    """Why constraint k's binary flag and model do not go together, by name, or None.  A binary constraint -- response 0 or 1, 1 =
    violated -- is modelled by a gp_classifier, and a gp_classifier models nothing else."""
    mtype = (con.get("model") or {}).get("type", "gp_classifier" if con.get("binary") else "gp_regressor")
    if con.get("binary") and mtype != "gp_classifier":
        return "config.bot.constraints[%d] is binary with the %s model: a binary constraint is modelled by a gp_classifier" % (k, mtype)
    if not con.get("binary") and mtype == "gp_classifier":
        return "config.bot.constraints[%d] with the gp_classifier model: a classifier models a binary constraint (set binary = True)" % k
    if con.get("binary") and float(con.get("threshold", 0.5)) != 0.5:
        return "config.bot.constraints[%d] is binary with threshold %g: the labels are 0 (satisfied) and 1 (violated), threshold 0.5" % (
            k, float(con["threshold"]))
    return None


KG_DISCRETISATIONS = ("mean", "thompson")


def kg_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate by the knowledge gradient (b7_kg_nominate's own refusals, by name), or None."""
    if int(config["bot"].get("batch", 1)) > 1:
        return "knowledge_gradient with config.bot.batch > 1: knowledge-gradient batches are not built"
    if config["bot"].get("refine"):
        return refine_refusal(config, model_class, sharded)
    if config["bot"].get("constraints"):
        return constraint_refusal(config, model_class, sharded)
    if sharded:
        return "knowledge_gradient over sharded candidates: the knowledge gradient over a sharded grid is not built"
    if model_class == "bot7.models.dngo":
        return "knowledge_gradient with the dngo model: the Bayesian-linear head has no posterior-covariance kernel"
    kind = config["score"].get("discretisation", "mean")
    if kind not in KG_DISCRETISATIONS:
        return "knowledge_gradient with config.score.discretisation = %r: %s are built" % (kind, ", ".join(KG_DISCRETISATIONS))
    return None


EHVI = "expected_hypervolume_improvement"
LOG_EHVI = "log_expected_hypervolume_improvement"   # the same trials by the log score (b7_logehvi_nominate / b7_logehvi3_nominate)
EHVI_KINDS = (EHVI, LOG_EHVI)
THOMPSON = "thompson_sampling"   # with config.bot.objectives: q nominees per trial from every objective's sample paths (b7_ts_hvi_nominate)
BATCH_MAX = 16  # B7_BATCH_MAX
TS_FEAS_CMAX = 8  # B7_TS_FEAS_CMAX


def objectives_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate for two objectives (what b7_ehvi_nominate does not do, by name), or None."""
    kind = config["score"]["type"]
    obj = config["bot"].get("objectives")
    if obj is None:
        if kind in EHVI_KINDS:
            return "%s without config.bot.objectives: the score needs two objectives, each with a model of its own" % kind
        return None
    if "models" in obj:
        return objectives3_refusal(config, model_class, sharded)
    if int(config["bot"].get("batch", 1)) > 1 and kind != THOMPSON:
        return "config.bot.objectives with config.bot.batch > 1: two-objective batches are not built"
    if config["bot"].get("refine"):
        return "config.bot.objectives with config.bot.refine: refinement of a two-objective nominee is not built"
    if config["bot"].get("constraints"):
        return "config.bot.objectives with config.bot.constraints: constraints combined with objectives are not built"
    if sharded:
        return "config.bot.objectives over sharded candidates: two objectives over a sharded grid are not built"
    if model_class == "bot7.models.dngo":
        return "config.bot.objectives with the dngo model: the Bayesian-linear head keeps no posterior for a second objective"
    if kind == THOMPSON and int(config["bot"].get("batch", 1)) > BATCH_MAX:
        return "config.bot.objectives with config.bot.batch = %d: at most %d nominees per trial are built" % (int(config["bot"]["batch"]), BATCH_MAX)
    if kind not in EHVI_KINDS and kind != THOMPSON:
        return "config.bot.objectives with %s: only %s is built" % (kind, EHVI)
    if (obj.get("model") or {}).get("type", "gp_regressor") != "gp_regressor":
        return "config.bot.objectives with the %s model: the second objective is modelled by a gp_regressor" % obj["model"]["type"]
    return None


def objectives3_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate for three objectives (what b7_ehvi3_nominate does not do, by name), or None."""
    kind = config["score"]["type"]
    models = config["bot"]["objectives"].get("models") or []
    if len(models) != 2:
        return "config.bot.objectives with %d models: models holds the second and the third objective's (four or more objectives are not built)" \
            % len(models)
    if int(config["bot"].get("batch", 1)) > 1 and kind != THOMPSON:
        return "config.bot.objectives with config.bot.batch > 1: three-objective batches are not built"
    if config["bot"].get("refine"):
        return "config.bot.objectives with config.bot.refine: refinement of a three-objective nominee is not built"
    if config["bot"].get("constraints"):
        return "config.bot.objectives with config.bot.constraints: constraints combined with objectives are not built"
    if config["bot"].get("trust_region"):
        return "config.bot.objectives with config.bot.trust_region: three objectives inside a trust region are not built"
    if sharded:
        return "config.bot.objectives over sharded candidates: three objectives over a sharded grid are not built"
    if model_class == "bot7.models.dngo":
        return "config.bot.objectives with the dngo model: the Bayesian-linear head keeps no posterior for further objectives"
    if kind == THOMPSON and int(config["bot"].get("batch", 1)) > BATCH_MAX:
        return "config.bot.objectives with config.bot.batch = %d: at most %d nominees per trial are built" % (int(config["bot"]["batch"]), BATCH_MAX)
    if kind not in EHVI_KINDS and kind != THOMPSON:
        return "config.bot.objectives with %s: only %s is built" % (kind, EHVI)
    for m in models:
        if (m or {}).get("type", "gp_regressor") != "gp_regressor":
            return "config.bot.objectives with the %s model: the second and third objectives are modelled by a gp_regressor" % m["type"]
    return None


TR_BASES = ("sobol", "random")
TR_KEYS = ("length_init", "length_min", "length_max", "success_tolerance", "failure_tolerance", "perturb", "base")


def trust_region_refusal(config, model_class="bot7.models.gp_regressor", sharded=False):
    """Why this configuration cannot nominate inside a trust region (what _run_trial_trust_region does not do, by name), or None."""
    tr = config["bot"].get("trust_region")
    if not tr:
        return None
    if config["bot"].get("refine"):
        return "config.bot.trust_region with config.bot.refine: refinement inside a trust region is not built"
    if config["bot"].get("constraints"):
        return "config.bot.trust_region with config.bot.constraints: constraints inside a trust region are not built"
    if config["bot"].get("objectives") or config["score"]["type"] in EHVI_KINDS:
        return "config.bot.trust_region with config.bot.objectives / %s: two objectives inside a trust region are not built" % EHVI
    if sharded:
        return "config.bot.trust_region over sharded candidates or a group: the sharded trust-region loop is not built"
    if model_class == "bot7.models.dngo":
        return "config.bot.trust_region with the dngo model: the box is shaped by a GP's ARD lengthscales"
    unknown = sorted(set(tr) - set(TR_KEYS))
    if unknown:
        return "config.bot.trust_region with unknown entries %s: %s are read" % (", ".join(unknown), ", ".join(TR_KEYS))
    base = tr.get("base", config["grid"].get("type", "sobol"))
    if base not in TR_BASES:
        return "config.bot.trust_region with base = %r: %s are built" % (base, ", ".join(TR_BASES))
    if base == "sobol" and int(config["grid"]["dims"]) >= 40:
        return "config.bot.trust_region with base = 'sobol' in %d dimensions: the sobol grid is built for fewer than 40 (base = 'random' takes any)" \
            % int(config["grid"]["dims"])
    q = int(config["bot"].get("batch", 1))
    if q > BATCH_MAX:
        return "config.bot.trust_region with config.bot.batch = %d: at most %d nominees per trial are built" % (q, BATCH_MAX)
    if q > int(config["grid"]["size"]):
        return "config.bot.trust_region with config.bot.batch = %d above config.grid.size = %d candidates per trial" % (q, int(config["grid"]["size"]))
    if not 0.0 <= float(tr.get("perturb", 1.0)) <= 1.0:
        return "config.bot.trust_region with perturb = %r: a probability" % (tr["perturb"],)
    return None


class _KeptHypers(object):
    """The model as a nomination branch sees it during a trust-region trial: the trial's hyper samples were drawn before the box
    could be made, so the branch's own draws (the burn-in call, then one sample_hypers + parse_hypers per sample) hand those out
    again instead of advancing the sampler a second time.  Everything else is the model's."""

    def __init__(self, model, hyps):
        self._model, self._hyps, self._next = model, hyps, 0

    def sample_hypers(self, *args):
        return None

    def parse_hypers(self, _vec):
        hyp = self._hyps[self._next % len(self._hyps)]
        self._next += 1
        return hyp

    def __getattr__(self, name):
        return getattr(self._model, name)


def split_objectives(responses):
    """The objective's rows [y1, y2] -> (Y1 N x 1, Y2 N x 1)."""
    R = np.asarray(responses, dtype=np.float64)
    R = R.reshape(-1, 2) if R.ndim < 2 else R
    if R.shape[1] != 2:
        raise ValueError("config.bot.objectives: the objective must return rows of 2 columns [y1, y2], got %d" % R.shape[1])
    return np.ascontiguousarray(R[:, :1]), np.ascontiguousarray(R[:, 1:2])


def split_objectives3(responses):
    """The objective's rows [y1, y2, y3] -> (Y1 N x 1, Y2 N x 1, Y3 N x 1)."""
    R = np.asarray(responses, dtype=np.float64)
    R = R.reshape(-1, 3) if R.ndim < 2 else R
    if R.shape[1] != 3:
        raise ValueError("config.bot.objectives: with two further models the objective must return rows of 3 columns [y1, y2, y3], got %d" % R.shape[1])
    return tuple(np.ascontiguousarray(R[:, k:k + 1]) for k in range(3))


def default_ref(responses):
    """The reference point when config.bot.objectives.ref is None: per column the maximum of the observations plus 10 % of the
    column's range (the common nadir heuristic; a column without a range takes 10 % of max(|maximum|, 1) instead).  Rows with a NaN
    take no part."""
    R = np.asarray(responses, dtype=np.float64)
    three = R.ndim == 2 and R.shape[1] == 3      # (rows of three objectives: split_objectives3; anything else is judged as two)
    R = np.concatenate(split_objectives3(responses) if three else split_objectives(responses), axis=1)
    R = R[~np.isnan(R).any(axis=1)]
    hi, lo = R.max(axis=0), R.min(axis=0)
    span = np.where(hi > lo, hi - lo, np.maximum(np.abs(hi), 1.0))
    return hi + 0.1 * span


def split_columns(responses, C):
    """The objective's rows [y, c_1 .. c_C] -> (Y N x 1, [c_k N x 1 for each constraint])."""
    R = np.asarray(responses, dtype=np.float64)
    R = R.reshape(-1, 1 + C) if R.ndim < 2 else R
    if R.shape[1] != 1 + C:
        raise ValueError("config.bot.constraints: the objective must return rows of 1 + %d columns [y, c_1 .. c_C], got %d"
                         % (C, R.shape[1]))
    return np.ascontiguousarray(R[:, :1]), [np.ascontiguousarray(R[:, k:k + 1]) for k in range(1, C + 1)]


def feasible_rows(responses, thresholds):
    """Which observed rows satisfy every constraint, c_k <= t_k (a NaN satisfies nothing)."""
    _, cols = split_columns(responses, len(thresholds))
    ok = np.ones(cols[0].shape[0] if cols else np.asarray(responses).shape[0], dtype=bool)
    for c, t in zip(cols, thresholds):
        ok &= c[:, 0] <= float(t)
    return ok


def objective_rows(Y_obs, constraints):
    """Which observed rows reach the OBJECTIVE's model: all of them, unless a binary constraint is present -- the objective then does
    not exist where a run failed (NaN), and the rows whose objective is not finite are left out of its data.  They stay in every
    constraint model's."""
    Y = np.asarray(Y_obs, dtype=np.float64)
    if not any(c.get("binary") for c in constraints):
        return np.ones(Y.shape[0], dtype=bool)
    return np.isfinite(Y).all(axis=1)


def best_feasible_fmin(responses, thresholds):
    """fmin of the constrained nomination: the best objective value among the feasible rows, as a 1-vector -- or None when no row
    is feasible (the nomination then goes by feasibility alone)."""
    Y, _ = split_columns(responses, len(thresholds))
    ok = feasible_rows(responses, thresholds)
    return np.array([Y[ok, 0].min()]) if ok.any() else None


class bayesopt(abstract):
    title = "bot7.bots.bayesopt"

    def __init__(self, objective, hypers, config=None, cache=None):
        cache = cache or {}
        super().__init__(objective, hypers, config, cache)
        config = self.config
        self.model = cache.get("model") or Models.registry[config["model"]["type"]](config["model"])  # :31
        self.score = cache.get("score") or Scores.registry[config["score"]["type"]](config["score"])  # :32
        self._rng = np.random.default_rng(config["bot"]["seed"])
        self.last_scores = None
        self.constraints = None   # per constraint: threshold, model, ctx, grid (the DeviceGrid view of that context); set up on first use
        self.objective2 = None    # the second objective: model, ctx, grid (the DeviceGrid view of that context); set up on first use
        self.objectives23 = None  # three objectives: the second and the third, each as objective2 is; set up on first use
        self.tr_state = None      # the trust region's TrustRegionState; set up on the first trust-region trial
        self.tr_start = 0         # the model's window: observations [tr_start:] are those since the last restart
        self.tr_since = 0         # trials since the last restart (the first nInitial of them nominate at random)
        self.tr_trace = []        # per trial: what it takes to regenerate the trial's grid and nominees

    def configure(self, config):
        config = super().configure(config)
        config["model"] = self._model_defaults(config.get("model"), config["bot"]["nSamples"])
        score = dict(config.get("score") or {})
        score.setdefault("type", "expected_improvement")  # :49
        if score.get("refine"):                         # ours: absent / False, or a dict of starts / iters / eta0 (nominate_ts_refine)
            score["refine"] = dict(REFINE_DEFAULTS, **(score["refine"] if isinstance(score["refine"], dict) else {}))
        config["score"] = score
        config["bot"].setdefault("batch", 1)            # ours: nominees per trial (nominate_batch); 1 is the reference's loop
        config["bot"].setdefault("refine", False)       # ours: False, or a dict of starts / iters / eta0 (nominate_refine)
        if config["bot"]["refine"]:
            given = config["bot"]["refine"] if isinstance(config["bot"]["refine"], dict) else {}
            config["bot"]["refine"] = dict(REFINE_DEFAULTS, **given)
        config["bot"].setdefault("constraints", None)   # ours: None, or a list of {"threshold": t, "model": {...}} (nominate_constrained)
        if not config["bot"]["constraints"]:            # (an empty list constrains nothing: the reference's loop)
            config["bot"]["constraints"] = None
        if config["bot"]["constraints"] is not None:
            config["bot"]["constraints"] = [self._constraint_defaults(c, config["bot"]["nSamples"]) for c in config["bot"]["constraints"]]
        config["bot"].setdefault("objectives", None)    # ours: None, or {"ref": [r1, r2] | None, "model": {...}} (nominate_objectives)
        if config["bot"]["objectives"] is not None and "models" in config["bot"]["objectives"]:
            # THREE objectives: {"ref": [r1, r2, r3] | None, "models": [{...}, {...}]}, the second and the third objective's models
            obj = dict(config["bot"]["objectives"])
            ref = obj.get("ref")
            config["bot"]["objectives"] = {"ref": None if ref is None else [float(r) for r in ref],
                                           "models": [self._model_defaults(m, config["bot"]["nSamples"]) for m in (obj.get("models") or [])]}
        elif config["bot"]["objectives"] is not None:
            obj = dict(config["bot"]["objectives"])
            ref = obj.get("ref")
            config["bot"]["objectives"] = {"ref": None if ref is None else [float(ref[0]), float(ref[1])],
                                           "model": self._model_defaults(obj.get("model"), config["bot"]["nSamples"])}
        config["bot"].setdefault("trust_region", None)  # ours: None, or a dict of TR_KEYS (_run_trial_trust_region)
        if config["bot"]["trust_region"] is not None:
            tr = dict(config["bot"]["trust_region"]) if isinstance(config["bot"]["trust_region"], dict) else {}
            for key in TR_KEYS[:5]:
                tr.setdefault(key, None)                # None: the library's default (b7_tr_init)
            tr.setdefault("perturb", min(1.0, 20.0 / config["grid"]["dims"]))
            tr.setdefault("base", config["grid"]["type"])
            config["bot"]["trust_region"] = tr
        return config

    @classmethod
    def _constraint_defaults(cls, con, nSamples):
        """{"threshold": t, "model": {...}}; a BINARY constraint (ours: "binary": True -- the response column holds 0 or 1, 1 =
        violated, and the objective may be NaN there) keeps its flag and is modelled by a gp_classifier unless the config says otherwise
        (binary_refusal then names it)."""
        model = dict(con.get("model") or {})
        if con.get("binary"):
            model.setdefault("type", "gp_classifier")
        out = {"threshold": float(con["threshold"]), "model": cls._model_defaults(model, nSamples)}
        if con.get("binary"):
            out["binary"] = True
        return out

    @staticmethod
    def _model_defaults(model, nSamples):
        model = dict(model or {})
        model.setdefault("type", "gp_regressor")        # bots/bayesopt.lua:40
        model.setdefault("kernel", "ardse")             # :41
        model.setdefault("nzModel", "GaussianNoise_iso")  # :42
        model.setdefault("mean", "constant")            # :43
        model.setdefault("sampler", "slice")            # :44
        if model["sampler"] == "slice_device":          # ours: the chain on the device draws a trial's samples in one launch
            model["prefetch"] = nSamples
        return model

    def eval(self, candidates=None, want_scores=True):
        """bots/bayesopt.lua:56-82.  Returns (scores or None, best_value, best_index_1based)."""
        X_obs, Y_obs = self.observed, self.responses
        X_hid = self.candidates if candidates is None else candidates
        model, ctx = self.model, self.model.ctx
        if self._thompson():
            if want_scores:
                raise NotImplementedError("thompson_sampling has no score vector (eval with want_scores=False, or nominate)")
            idx = (self.nominate_objectives_ts(1, X_hid) if self._objectives() else self._ts_nominate(1, X_hid))[0]
            return None, None, idx
        if self._kg():
            val, idx = self._kg_nominate(X_hid)
            scores = ctx.score_finish(1.0, download=True)[2] if want_scores else None   # the accumulator holds the marginal KG
            self.last_scores = scores
            return scores, val, idx
        if model.class_() == "bot7.models.dngo":                  # :65-66: one score call, no marginalisation loop
            model.predict_device(X_obs, Y_obs, X_hid, None)
            ctx.score_reset()
            self.score.add_to(ctx, Y_obs)
            val, idx, scores = ctx.score_finish(1.0, download=want_scores)
            self.last_scores = scores
            return scores, val, idx
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        nSamples = self.config["bot"]["nSamples"]
        spec = getattr(self.score, "device_spec", None)
        if hasattr(X_hid, "commit"):
            # a candidate set sharded over GPUs: every shard scores its rows, ONE exchange names the winner in the union
            # (b7_eval_nominate with a communicator / b7_group_eval_nominate); ranks run this loop in lock step
            hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True)) for _ in range(nSamples)]
            X_hid.set_kernel(getattr(model, "kernel", "ardse"))   # config.model.kernel on every context the nomination uses
            X_hid.stage_data(X_obs, Y_obs)
            sp = spec(Y_obs)
            val, idx = X_hid.eval_nominate(hyps, sp)
            self.last_scores = None
            return None, val, idx
        if spec is not None and self.config["bot"].get("fused", True) and hasattr(model, "stage"):
            # (the driver never hands pending points to the score, :66,76)
            hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True)) for _ in range(nSamples)]
            model.stage(X_obs, Y_obs, X_hid)                      # data + grid resident (uploads only what changed)
            val, idx = ctx.eval_nominate(hyps, **spec(Y_obs))     # :73-79 + :96 in one call
            scores = ctx.score_finish(1.0, download=True)[2] if want_scores else None   # the accumulator holds score / S
            self.last_scores = scores
            return scores, val, idx
        first = True
        for _ in range(nSamples):                                 # :73-78
            hyp = model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
            model.predict_device(X_obs, Y_obs, X_hid, hyp)        # inside score(...) -> model:predict
            if first:
                ctx.score_reset()                                 # :69 torch.zeros(M)
                first = False
            self.score.add_to(ctx, Y_obs)                         # :76 score:add(...)
        val, idx, scores = ctx.score_finish(float(nSamples), download=want_scores)  # :79 div, :96 max
        self.last_scores = scores
        return scores, val, idx

    def _thompson(self):
        return self.config["score"]["type"] == "thompson_sampling"

    def _ts_nominate(self, q, cand):
        """q nominees by Thompson sampling (b7_ts_nominate): the hyper samples as eval's fused branch draws them
        (bots/bayesopt.lua:68, :73-75), the call's seed from the bot's own generator."""
        X_obs, Y_obs, model = self.observed, self.responses, self.model
        assert not hasattr(cand, "commit"), "thompson_sampling: one GPU (sharded Thompson sampling is not built)"
        if model.class_() == "bot7.models.dngo":
            # the head's exact weight-space paths (b7_blr_ts_nominate): the point hyp table eval's DNGO branch predicts under
            # (:65-66), or config.model.hyps, a list of them (path j under table j mod S)
            hyps = model.config.get("hyps") or [model.hyp or model.init(X_obs, Y_obs)]
            seed = int(self._rng.integers(0, 2 ** 63))
            idx = self.score.nominate(model.ctx, hyps, q, seed, model=model, observed=X_obs, responses=Y_obs, candidates=cand)
            self.last_scores = None
            return [int(i) for i in idx]
        assert hasattr(model, "stage"), "thompson_sampling: a GP or dngo model"
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
                for _ in range(self.config["bot"]["nSamples"])]   # :73-75
        model.stage(X_obs, Y_obs, cand)
        seed = int(self._rng.integers(0, 2 ** 63))
        idx = self.score.nominate(model.ctx, hyps, q, seed)
        self.last_scores = None
        return [int(i) for i in idx]

    def _ts_refined(self):
        """THE predicate: does this bot refine its Thompson nominees on their sample paths (config.score.refine)."""
        return self._thompson() and bool(self.config["score"].get("refine"))

    def nominate_ts_refine(self, q, cand, lo, hi):
        """q Thompson nominees refined off the grid by descent on their own sample paths inside the box [lo, hi]
        (b7_ts_nominate_refine; no counterpart in the reference) -> (the 1-based grid nominees, distinct, which the caller steals;
        the refined points q x d, which it evaluates and observes).  Sampling and seed as _ts_nominate."""
        X_obs, Y_obs, model = self.observed, self.responses, self.model
        why = ts_refine_refusal(self.config, model.class_(), hasattr(cand, "commit"))
        if why:
            raise NotImplementedError(why)
        assert hasattr(model, "stage"), "config.score.refine: a GP model on one GPU"
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
                for _ in range(self.config["bot"]["nSamples"])]   # :73-75
        model.stage(X_obs, Y_obs, cand)
        seed = int(self._rng.integers(0, 2 ** 63))
        idx, x = self.score.nominate_refine(model.ctx, hyps, q, seed, np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64))
        self.last_scores = None
        return [int(i) for i in idx], np.array(x, dtype=np.float64).reshape(len(idx), -1)

    def _run_trial_ts_refined(self):
        """bots/abstract.lua:112-152 with config.bot.batch Thompson nominees refined on their sample paths: the q GRID NOMINEES' rows
        are stolen in one stable pass (:118; distinct by construction, whichever start won), the objective is evaluated at the
        refined points (:124) and those points are observed (:143-144).  The box is the grid's (config.grid.mins / maxes)."""
        self.nTrials += 1
        q, grid = int(self.config["bot"]["batch"]), self.config["grid"]
        cand = self.candidates
        idx, rows = self.nominate_ts_refine(q, cand, grid["mins"], grid["maxes"])       # :117
        host = T.remove(np.asarray(cand), idx)                     # :118
        if isinstance(cand, DeviceGrid) and cand.ctx is not None and cand.version == cand.ctx.grid_version:
            cand.ctx.grid_remove_rows(idx)                         # the same stable deletion on the resident copy
            self.candidates = None if host is None else DeviceGrid(host, cand.ctx, cand.ctx.grid_version)
        else:
            self.candidates = host
        self.last_ts_refine = {"index": idx, "x": rows.copy()}
        ys = np.concatenate([np.asarray(self.objective(r), dtype=np.float64).reshape(1, -1) for r in rows], 0)   # :124
        self.responses = ys if self.responses is None else np.concatenate([self.responses, ys], 0)
        self.observed = rows if self.observed is None else np.concatenate([self.observed, rows], 0)            # :143-144
        best = int(ys[:, 0].argmin())
        return rows[best], ys[best:best + 1]

    def _kg(self):
        return self.config["score"]["type"] == "knowledge_gradient"

    def _kg_nominate(self, cand):
        """(value, 1-based nominee) by the knowledge gradient (b7_kg_nominate): the hyper samples as eval's fused branch draws them
        (bots/bayesopt.lua:68, :73-75); under discretisation = 'thompson' the rows of A are the minimisers of `points` sample paths
        under those same hyper samples.  self.last_kg keeps what the call used."""
        X_obs, Y_obs, model = self.observed, self.responses, self.model
        why = kg_refusal(self.config, model.class_(), hasattr(cand, "commit"))
        if why:
            raise NotImplementedError(why)
        hyps = self._sample_hyps(model, X_obs, Y_obs)
        model.stage(X_obs, Y_obs, cand)
        points = min(int(self.score.config["points"]), cand.shape[0])
        rows, seed = None, None
        if self.score.config["discretisation"] == "thompson":
            seed = int(self._rng.integers(0, 2 ** 63))
            rows = [int(i) for i in model.ctx.ts_nominate(hyps, points, n_features=int(self.score.config["nFeatures"]), seed=seed)[1]]
        val, idx = self.score.nominate(model.ctx, hyps, points, rows)
        self.last_scores = None
        self.last_kg = {"hyps": hyps, "points": points, "rows": rows, "seed": seed, "value": val, "index": int(idx)}
        return val, int(idx)

    def nominate(self, candidates=None):
        """bots/bayesopt.lua:85-99."""
        cand = self.candidates if candidates is None else candidates
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91 floor(rand*M)+1
            return int(np.floor(self._rng.random() * cand.shape[0])) + 1
        _, _, idx = self.eval(cand, want_scores=False)            # :95-96
        return idx

    def nominate_batch(self, q=None, candidates=None):
        """q nominees from ONE library call (b7_eval_nominate_batch; no counterpart in the reference): nominate's pick, then
        q - 1 more by kriging-believer variance downdates.  Returns q 1-based indices into the candidates as they stand; the
        caller commits them.  Sampling as eval's fused branch (bots/bayesopt.lua:68, :73-75); q = 1 is nominate."""
        cand = self.candidates if candidates is None else candidates
        q = int(self.config["bot"]["batch"] if q is None else q)
        if q == 1:
            return [int(self.nominate(cand))]
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91, q distinct rows
            return [int(i) + 1 for i in self._rng.choice(cand.shape[0], size=q, replace=False)]
        if self._thompson():
            return self._ts_nominate(q, cand)
        if self._kg():
            raise NotImplementedError(kg_refusal(dict(self.config, bot=dict(self.config["bot"], batch=q))))
        X_obs, Y_obs, model = self.observed, self.responses, self.model
        spec = getattr(self.score, "device_spec", None)
        assert spec is not None and hasattr(model, "stage") and not hasattr(cand, "commit"), \
            "nominate_batch: a GP model with a device score on one GPU (sharded batches are not built)"
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
                for _ in range(self.config["bot"]["nSamples"])]   # :73-75
        model.stage(X_obs, Y_obs, cand)
        _, idx = model.ctx.eval_nominate_batch(hyps, q, **spec(Y_obs))
        self.last_scores = None
        return [int(i) for i in idx]

    def nominate_refine(self, candidates=None):
        """The nominee refined off the grid (b7_eval_nominate_refine; no counterpart in the reference) -> (refined point x[d], the
        1-based grid row its start came from).  Sampling as eval's fused branch (bots/bayesopt.lua:68, :73-75); the box is the
        grid's (config.grid.mins / maxes)."""
        cand = self.candidates if candidates is None else candidates
        X_obs, Y_obs, model = self.observed, self.responses, self.model
        why = refine_refusal(self.config, model.class_(), hasattr(cand, "commit"))
        if why:
            raise NotImplementedError(why)
        spec = getattr(self.score, "device_spec", None)
        assert spec is not None and hasattr(model, "stage"), "config.bot.refine: a GP model with a device score on one GPU"
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        hyps = [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
                for _ in range(self.config["bot"]["nSamples"])]   # :73-75
        model.stage(X_obs, Y_obs, cand)
        grid, ref = self.config["grid"], self.config["bot"]["refine"]
        _, _, x, _, start = model.ctx.eval_nominate_refine(hyps, starts=ref["starts"], iters=ref["iters"], eta0=ref["eta0"],
                                                           lo=np.asarray(grid["mins"], dtype=np.float64),
                                                           hi=np.asarray(grid["maxes"], dtype=np.float64), **spec(Y_obs))
        self.last_scores = None
        return np.array(x, dtype=np.float64), int(start)

    # ---- constrained nomination (config.bot.constraints) ----------------------------------------------------------------------
    def _constrained(self):
        """THE predicate: does this bot nominate under constraints (run_trial, update_best and progress_report all ask here)."""
        return self.config["bot"].get("constraints") is not None

    def _constraint_refusal(self):
        return constraint_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))

    def _constraints_setup(self):
        """One GP model with a context (same device) and sampler state of its own per constraint."""
        if self.constraints is None:
            from bot7_amd import Context
            self.constraints = []
            for con in self.config["bot"]["constraints"]:
                ctx = Context(self.model.ctx.device_id)
                self.constraints.append({"threshold": con["threshold"], "ctx": ctx, "grid": None, "binary": bool(con.get("binary")),
                                         "model": Models.registry[con["model"]["type"]](con["model"], context=ctx)})
        return self.constraints

    def _sample_hyps(self, model, X_obs, Y_obs):
        model.sample_hypers(X_obs, Y_obs)                         # :68 (burn-in call)
        return [model.parse_hypers(model.sample_hypers(X_obs, Y_obs, None, None, True))
                for _ in range(self.config["bot"]["nSamples"])]   # :73-75

    def nominate_constrained(self, candidates=None):
        """The constrained nominee (module docstring) -> 1-based index into the candidates as they stand.  self.last_constrained
        keeps what the call used: every model's hyper samples, fmin (None: feasibility alone) and the value."""
        cand = self.candidates if candidates is None else candidates
        why = self._constraint_refusal()
        if why:
            raise NotImplementedError(why)
        if self._constrained_ts():
            return self.nominate_constrained_ts(None, cand)       # (a list of config.bot.batch indices)
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91 floor(rand*M)+1
            return int(np.floor(self._rng.random() * cand.shape[0])) + 1
        cons = self._constraints_setup()
        thresholds = [c["threshold"] for c in cons]
        X_obs, model = self.observed, self.model
        Y_obs, C_obs = split_columns(self.responses, len(cons))
        host = np.asarray(cand, dtype=np.float64)
        con_hyps = []
        for con, Ck in zip(cons, C_obs):
            hyps = self._sample_hyps(con["model"], X_obs, Ck)
            if con["grid"] is None or con["grid"].version != con["ctx"].grid_version or not np.array_equal(np.asarray(con["grid"]), host):
                con["ctx"].grid_upload(host)
                con["grid"] = DeviceGrid(host, con["ctx"], con["ctx"].grid_version)
            con["model"].stage(X_obs, Ck, con["grid"])
            if con.get("binary"):                                 # the classifier's log Pr[feasible] in the accumulator
                con["ctx"].clf_eval_logfeas(hyps)
            else:
                con["ctx"].eval_nominate(hyps, score="logpi", fmin=[con["threshold"]], tradeoff=0.0)   # log Pr[c_k <= t_k] in the accumulator
            con_hyps.append(hyps)
        rows = objective_rows(Y_obs, cons)                        # (all of them unless a binary constraint is present)
        if not rows.all():
            X_obs, Y_obs = np.ascontiguousarray(X_obs[rows]), np.ascontiguousarray(Y_obs[rows])
        ctx = model.ctx
        if rows.any():
            hyps = self._sample_hyps(model, X_obs, Y_obs)
            model.stage(X_obs, Y_obs, cand)
        else:                                                     # no run has returned an objective yet: feasibility alone, no objective model
            hyps = None
            if not model._is_resident(cand):
                ctx.grid_upload(np.atleast_2d(host))
        ctx.feas_reset()
        for con in cons:
            ctx.feas_add_acc(con["ctx"])
        fmin = best_feasible_fmin(self.responses, thresholds)
        if fmin is None or hyps is None:                          # no feasible observation yet: Gelbart et al. 2014, section 3.2
            fmin = None
            val, idx = ctx.feas_nominate()
        else:
            spec = dict(self.score.device_spec(Y_obs), fmin=fmin)
            val, idx = ctx.eval_nominate_feasible(hyps, **spec)
        self.last_scores = None
        self.last_constrained = {"hyps": hyps, "constraint_hyps": con_hyps, "fmin": fmin, "value": val, "index": int(idx)}
        if not rows.all():
            self.last_constrained["objective_rows"] = rows
        return int(idx)

    # ---- constrained Thompson sampling (config.score.type = 'constrained_thompson_sampling' with config.bot.constraints) ------------
    def _constrained_ts(self):
        return self.config["score"]["type"] == CONSTRAINED_THOMPSON

    def nominate_constrained_ts(self, q=None, candidates=None):
        """q feasible-first nominees by constrained Thompson sampling (SCBO's selection rule) -> q 1-based indices into the candidates
        as they stand.  Per model-based trial the objective's model and every constraint's model sample their hypers and stage their
        column on their own context, every context keeps q sample paths (ts_paths) drawn with a seed of its own from the bot's
        generator, and the objective's context nominates (ts_feas_nominate): path j picks the row of lowest f_j among the rows its
        constraint paths call feasible, or the row of smallest total violation where they call none.  No fmin, no feasibility column.
        self.last_constrained keeps what the call used."""
        cand = self.candidates if candidates is None else candidates
        why = self._constraint_refusal()
        if why:
            raise NotImplementedError(why)
        q = int(self.config["bot"]["batch"] if q is None else q)
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91, q distinct rows
            if q == 1:
                return [int(np.floor(self._rng.random() * cand.shape[0])) + 1]
            return [int(i) + 1 for i in self._rng.choice(cand.shape[0], size=q, replace=False)]
        cons = self._constraints_setup()
        thresholds = [c["threshold"] for c in cons]
        X_obs, model = self.observed, self.model
        Y_obs, C_obs = split_columns(self.responses, len(cons))
        host = np.asarray(cand, dtype=np.float64)
        hyps = [self._sample_hyps(model, X_obs, Y_obs)]
        model.stage(X_obs, Y_obs, cand)
        for con, Ck in zip(cons, C_obs):
            hyps.append(self._sample_hyps(con["model"], X_obs, Ck))
            if con["grid"] is None or con["grid"].version != con["ctx"].grid_version or not np.array_equal(np.asarray(con["grid"]), host):
                con["ctx"].grid_upload(host)
                con["grid"] = DeviceGrid(host, con["ctx"], con["ctx"].grid_version)
            con["model"].stage(X_obs, Ck, con["grid"])
        seeds = []
        while len(seeds) < 1 + len(cons):                         # a seed per model and trial, distinct
            seed = int(self._rng.integers(0, 2 ** 63))
            if seed not in seeds:
                seeds.append(seed)
        out = self.score.nominate_constrained([model.ctx] + [con["ctx"] for con in cons], hyps, q, seeds, thresholds)
        idx = [int(i) for i in out["index"]]
        if min(idx) < 1:
            raise RuntimeError("constrained_thompson_sampling: path %d has a NaN in every row: nothing to nominate" % idx.index(min(idx)))
        self.last_scores = None
        self.last_constrained = {"hyps": hyps[0], "constraint_hyps": hyps[1:], "seeds": seeds, "thresholds": list(thresholds), "index": idx,
                                 "cls": np.array(out["cls"]), "key": np.array(out["key"]), "y": np.array(out["y"]), "reruns": int(out["reruns"])}
        return idx

    def _run_trial_constrained_ts(self):
        """run_trial's batch handling with the constrained Thompson nominees: the q stolen rows leave every context's resident grid in
        one stable pass (:118), the q response rows [y, c_1 .. c_C] are kept whole (:137-141), and at nInitial every model is
        initialised on its own column (:147-149).  Returns the batch's best feasible row, or its best row where none is feasible."""
        self.nTrials += 1
        idx = self.nominate_constrained_ts()                       # :117
        cand = self.candidates
        rows = np.array(np.asarray(cand)[np.asarray(idx) - 1], dtype=np.float64)
        host = T.remove(np.asarray(cand), idx)                     # :118, an index list (utils/tensor.lua:158-193)
        if isinstance(cand, DeviceGrid) and cand.ctx is not None and cand.version == cand.ctx.grid_version:
            assert np.array_equal(cand.ctx.grid_remove_rows(idx), rows)   # the same stable deletion on the resident copy
            self.candidates = None if host is None else DeviceGrid(host, cand.ctx, cand.ctx.grid_version)
        else:
            self.candidates = host
        for con in self.constraints or []:
            if con["grid"] is not None and con["grid"].version == con["ctx"].grid_version:
                con["ctx"].grid_remove_rows(idx)
                con["grid"] = None if host is None else DeviceGrid(host, con["ctx"], con["ctx"].grid_version)
        C = len(self.config["bot"]["constraints"])
        ys = np.concatenate([np.asarray(self.objective(r), dtype=np.float64).reshape(1, -1) for r in rows], 0)   # :124
        split_columns(ys, C)                                       # (the shape check)
        self.responses = ys if self.responses is None else np.concatenate([self.responses, ys], 0)
        self.observed = rows if self.observed is None else np.concatenate([self.observed, rows], 0)            # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            Y_obs, C_obs = split_columns(self.responses, C)
            self.model.init(self.observed, Y_obs)                  # :147-149
            for con, Ck in zip(self._constraints_setup(), C_obs):
                con["model"].init(self.observed, Ck)
        ok = feasible_rows(ys, [c["threshold"] for c in self.config["bot"]["constraints"]])
        best = int(np.where(ok, ys[:, 0], np.inf).argmin()) if ok.any() else int(ys[:, 0].argmin())
        return rows[best], ys[best:best + 1]

    def _run_trial_constrained(self):
        """bots/abstract.lua:112-152 with the constrained nominee: the stolen row (:118) leaves every constraint context's resident
        grid too, the objective's row [y, c_1 .. c_C] is kept whole (:137-141), and at nInitial every model is initialised on its
        own column (:147-149)."""
        why = self._constraint_refusal()
        if why:
            raise NotImplementedError(why)
        if self._constrained_ts():
            return self._run_trial_constrained_ts()
        self.nTrials += 1
        idx = self.nominate_constrained()                          # :117
        self._steal_candidate(idx)                                 # :118
        for con in self.constraints or []:
            if con["grid"] is not None and con["grid"].version == con["ctx"].grid_version:
                con["ctx"].grid_remove(idx)
                con["grid"] = DeviceGrid(np.asarray(self.candidates), con["ctx"], con["ctx"].grid_version)
        k = self.pending.shape[0]
        nominee = self.pending[k - 1]
        C = len(self.config["bot"]["constraints"])
        y = np.asarray(self.objective(nominee), dtype=np.float64).reshape(1, -1)   # :124
        split_columns(y, C)                                        # (the shape check)
        self.responses = y if self.responses is None else np.concatenate([self.responses, y], 0)
        self.observed, self.pending = T.steal(self.observed, self.pending, [k])  # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            Y_obs, C_obs = split_columns(self.responses, C)
            rows = objective_rows(Y_obs, self.config["bot"]["constraints"])
            if rows.any():                                         # (none yet: the model initialises itself at its first sample_hypers)
                self.model.init(self.observed[rows], Y_obs[rows])  # :147-149
            for con, Ck in zip(self._constraints_setup(), C_obs):
                con["model"].init(self.observed, Ck)
        return nominee, y

    # ---- two objectives (config.bot.objectives) --------------------------------------------------------------------------------
    def _objectives(self):
        """THE predicate: does this bot nominate for two objectives (run_trial, update_best and progress_report all ask here)."""
        return self.config["bot"].get("objectives") is not None

    def _objectives_refusal(self):
        return objectives_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))

    def _objectives_setup(self):
        """A GP model with a context (same device) and sampler state of its own for the second objective."""
        if self.objective2 is None:
            from bot7_amd import Context
            ctx = Context(self.model.ctx.device_id)
            mcfg = self.config["bot"]["objectives"]["model"]
            self.objective2 = {"ctx": ctx, "grid": None, "model": Models.registry[mcfg["type"]](mcfg, context=ctx)}
        return self.objective2

    def objectives_ref(self):
        """The reference point of this trial: config.bot.objectives.ref, or default_ref of the observations so far."""
        ref = self.config["bot"]["objectives"]["ref"]
        return default_ref(self.responses) if ref is None else np.asarray(ref, dtype=np.float64)

    def nominate_objectives(self, candidates=None):
        """The two-objective nominee -> 1-based index into the candidates as they stand.  The objective returns rows [y1, y2], both
        minimised; the bot's own model sees column 0, the second objective's model -- a GP with a context and sampler state of its
        own -- column 1.  Per model-based trial both models sample their hypers and both contexts keep their posterior over the
        same grid rows (eval_posterior); the front of the observations under the reference point comes from pareto_front2, and
        the objective's context nominates by the exact expected hypervolume improvement (ehvi_nominate), marginalised over both
        models' samples.  With config.bot.objectives.ref = None the reference point is recomputed EVERY trial as the per-column
        maximum of the observations plus 10 % of the column's range (default_ref): hypervolumes of different trials are then
        measured against different boxes.  self.last_objectives keeps what the call used."""
        from bot7_amd import _lib
        cand = self.candidates if candidates is None else candidates
        why = self._objectives_refusal()
        if why:
            raise NotImplementedError(why)
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91 floor(rand*M)+1
            return int(np.floor(self._rng.random() * cand.shape[0])) + 1
        o2 = self._objectives_setup()
        X_obs, model = self.observed, self.model
        Y1, Y2 = split_objectives(self.responses)
        ref = self.objectives_ref()
        front, rows = _lib.pareto_front2(self.responses, ref)     # P = 0 while nothing observed lies inside the box
        host = np.asarray(cand, dtype=np.float64)
        hyps1 = self._sample_hyps(model, X_obs, Y1)
        hyps2 = self._sample_hyps(o2["model"], X_obs, Y2)
        model.stage(X_obs, Y1, cand)
        model.ctx.eval_posterior(hyps1)
        if o2["grid"] is None or o2["grid"].version != o2["ctx"].grid_version or not np.array_equal(np.asarray(o2["grid"]), host):
            o2["ctx"].grid_upload(host)
            o2["grid"] = DeviceGrid(host, o2["ctx"], o2["ctx"].grid_version)
        o2["model"].stage(X_obs, Y2, o2["grid"])
        o2["ctx"].eval_posterior(hyps2)
        val, idx = self.score.nominate(model.ctx, o2["ctx"], front, ref)
        self.last_scores = None
        self.last_objectives = {"hyps": hyps1, "hyps2": hyps2, "ref": np.array(ref, dtype=np.float64), "front": front, "rows": rows,
                                "value": val, "index": int(idx)}
        return int(idx)

    def _run_trial_objectives(self):
        """bots/abstract.lua:112-152 with the two-objective nominee: the stolen row (:118) leaves the second context's resident
        grid too, the objective's row [y1, y2] is kept whole (:137-141), and at nInitial each model is initialised on its own
        column (:147-149)."""
        why = self._objectives_refusal()
        if why:
            raise NotImplementedError(why)
        if self._thompson():
            return self._run_trial_objectives_ts()
        if self._objectives3():
            return self._run_trial_objectives3()
        self.nTrials += 1
        idx = self.nominate_objectives()                           # :117
        self._steal_candidate(idx)                                 # :118
        o2 = self.objective2
        if o2 is not None and o2["grid"] is not None and o2["grid"].version == o2["ctx"].grid_version:
            o2["ctx"].grid_remove(idx)
            o2["grid"] = DeviceGrid(np.asarray(self.candidates), o2["ctx"], o2["ctx"].grid_version)
        k = self.pending.shape[0]
        nominee = self.pending[k - 1]
        y = np.asarray(self.objective(nominee), dtype=np.float64).reshape(1, -1)   # :124
        split_objectives(y)                                        # (the shape check)
        self.responses = y if self.responses is None else np.concatenate([self.responses, y], 0)
        self.observed, self.pending = T.steal(self.observed, self.pending, [k])  # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            Y1, Y2 = split_objectives(self.responses)
            self.model.init(self.observed, Y1)                     # :147-149
            self._objectives_setup()["model"].init(self.observed, Y2)
        return nominee, y

    # ---- three objectives (config.bot.objectives = {"ref", "models": [m2, m3]}) ------------------------------------------------
    def _objectives3(self):
        """Does this bot nominate for THREE objectives: config.bot.objectives carries "models" (two of them) in place of "model"."""
        return self._objectives() and "models" in self.config["bot"]["objectives"]

    def _objectives3_setup(self):
        """For the second and the third objective each a GP model with a context (same device) and sampler state of its own."""
        if self.objectives23 is None:
            from bot7_amd import Context
            self.objectives23 = []
            for mcfg in self.config["bot"]["objectives"]["models"]:
                ctx = Context(self.model.ctx.device_id)
                self.objectives23.append({"ctx": ctx, "grid": None, "model": Models.registry[mcfg["type"]](mcfg, context=ctx)})
        return self.objectives23

    def nominate_objectives3(self, candidates=None):
        """The three-objective nominee -> 1-based index into the candidates as they stand: nominate_objectives with a third column,
        a third model and context, the front from pareto_front3 and the nomination by ehvi3_nominate (the exact expected
        hypervolume improvement over the boxes of the non-dominated region, marginalised over the three models' samples).
        self.last_objectives keeps what the call used ("hyps" a list of three)."""
        from bot7_amd import _lib
        cand = self.candidates if candidates is None else candidates
        why = self._objectives_refusal()
        if why:
            raise NotImplementedError(why)
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91 floor(rand*M)+1
            return int(np.floor(self._rng.random() * cand.shape[0])) + 1
        others = self._objectives3_setup()
        X_obs, model = self.observed, self.model
        Ys = split_objectives3(self.responses)
        ref = self.objectives_ref()
        front, rows = _lib.pareto_front3(self.responses, ref)     # P = 0 while nothing observed lies inside the box
        host = np.asarray(cand, dtype=np.float64)
        hyps = [self._sample_hyps(model, X_obs, Ys[0])] + [self._sample_hyps(o["model"], X_obs, Y) for o, Y in zip(others, Ys[1:])]
        model.stage(X_obs, Ys[0], cand)
        model.ctx.eval_posterior(hyps[0])
        for o, Y, h in zip(others, Ys[1:], hyps[1:]):
            if o["grid"] is None or o["grid"].version != o["ctx"].grid_version or not np.array_equal(np.asarray(o["grid"]), host):
                o["ctx"].grid_upload(host)
                o["grid"] = DeviceGrid(host, o["ctx"], o["ctx"].grid_version)
            o["model"].stage(X_obs, Y, o["grid"])
            o["ctx"].eval_posterior(h)
        val, idx = self.score.nominate(model.ctx, (others[0]["ctx"], others[1]["ctx"]), front, ref)
        self.last_scores = None
        self.last_objectives = {"hyps": hyps, "ref": np.array(ref, dtype=np.float64), "front": front, "rows": rows,
                                "value": val, "index": int(idx)}
        return int(idx)

    def _run_trial_objectives3(self):
        """_run_trial_objectives with three columns: the stolen row leaves the second and the third context's resident grid too."""
        self.nTrials += 1
        idx = self.nominate_objectives3()                          # :117
        self._steal_candidate(idx)                                 # :118
        for o in self.objectives23 or ():
            if o["grid"] is not None and o["grid"].version == o["ctx"].grid_version:
                o["ctx"].grid_remove(idx)
                o["grid"] = DeviceGrid(np.asarray(self.candidates), o["ctx"], o["ctx"].grid_version)
        k = self.pending.shape[0]
        nominee = self.pending[k - 1]
        y = np.asarray(self.objective(nominee), dtype=np.float64).reshape(1, -1)   # :124
        split_objectives3(y)                                       # (the shape check)
        self.responses = y if self.responses is None else np.concatenate([self.responses, y], 0)
        self.observed, self.pending = T.steal(self.observed, self.pending, [k])  # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            Ys = split_objectives3(self.responses)
            self.model.init(self.observed, Ys[0])                  # :147-149
            for o, Y in zip(self._objectives3_setup(), Ys[1:]):
                o["model"].init(self.observed, Y)
        return nominee, y

    # ---- two or three objectives by Thompson sampling (config.score.type = 'thompson_sampling' with config.bot.objectives) -----------
    def _objectives_ts(self):
        return self._objectives() and self._thompson()

    def nominate_objectives_ts(self, q=None, candidates=None):
        """q nominees for two or three objectives by Thompson sampling (TSEMO) -> q 1-based indices into the candidates as they
        stand.  Per model-based trial every objective's model samples its hypers and stages its column on its own context, every
        context keeps q sample paths (ts_paths) drawn with a seed from the bot's generator, in objective order, and the first context
        nominates (ts_hvi_nominate): path j picks the row whose sampled values improve the hypervolume of the observations' front
        plus the earlier picks under path j the most.  self.last_objectives keeps what the call used."""
        from bot7_amd import _lib
        cand = self.candidates if candidates is None else candidates
        why = self._objectives_refusal()
        if why:
            raise NotImplementedError(why)
        q = int(self.config["bot"]["batch"] if q is None else q)
        if self.nTrials <= self.config["bot"]["nInitial"]:        # :90-91, q distinct rows
            if q == 1:
                return [int(np.floor(self._rng.random() * cand.shape[0])) + 1]
            return [int(i) + 1 for i in self._rng.choice(cand.shape[0], size=q, replace=False)]
        three = self._objectives3()
        others = self._objectives3_setup() if three else [self._objectives_setup()]
        X_obs, model = self.observed, self.model
        Ys = split_objectives3(self.responses) if three else split_objectives(self.responses)
        ref = self.objectives_ref()
        front, rows = (_lib.pareto_front3 if three else _lib.pareto_front2)(self.responses, ref)
        host = np.asarray(cand, dtype=np.float64)
        hyps = [self._sample_hyps(model, X_obs, Ys[0])] + [self._sample_hyps(o["model"], X_obs, Y) for o, Y in zip(others, Ys[1:])]
        model.stage(X_obs, Ys[0], cand)
        for o, Y in zip(others, Ys[1:]):
            if o["grid"] is None or o["grid"].version != o["ctx"].grid_version or not np.array_equal(np.asarray(o["grid"]), host):
                o["ctx"].grid_upload(host)
                o["grid"] = DeviceGrid(host, o["ctx"], o["ctx"].grid_version)
            o["model"].stage(X_obs, Y, o["grid"])
        seeds = [int(self._rng.integers(0, 2 ** 63)) for _ in range(1 + len(others))]
        hvi, idx, y = self.score.nominate_objectives([model.ctx] + [o["ctx"] for o in others], hyps, q, seeds, front, ref)
        self.last_scores = None
        self.last_objectives = {"hyps": hyps, "seeds": seeds, "ref": np.array(ref, dtype=np.float64), "front": front, "rows": rows,
                                "index": [int(i) for i in idx], "hvi": np.array(hvi), "y": np.array(y)}
        return [int(i) for i in idx]

    def _run_trial_objectives_ts(self):
        """run_trial's batch handling with the Thompson nominees of two or three objectives: the q stolen rows leave every
        objective's resident grid in one stable pass (:118), the objective's rows are kept whole (:137-141), and at nInitial each
        model is initialised on its own column (:147-149)."""
        why = self._objectives_refusal()
        if why:
            raise NotImplementedError(why)
        three = self._objectives3()
        split = split_objectives3 if three else split_objectives
        self.nTrials += 1
        idx = self.nominate_objectives_ts()                        # :117
        cand = self.candidates
        rows = np.array(np.asarray(cand)[np.asarray(idx) - 1], dtype=np.float64)
        host = T.remove(np.asarray(cand), idx)                     # :118, an index list (utils/tensor.lua:158-193)
        if isinstance(cand, DeviceGrid) and cand.ctx is not None and cand.version == cand.ctx.grid_version:
            assert np.array_equal(cand.ctx.grid_remove_rows(idx), rows)   # the same stable deletion on the resident copy
            self.candidates = None if host is None else DeviceGrid(host, cand.ctx, cand.ctx.grid_version)
        else:
            self.candidates = host
        for o in (self.objectives23 or ()) if three else ([self.objective2] if self.objective2 else ()):
            if o["grid"] is not None and o["grid"].version == o["ctx"].grid_version:
                o["ctx"].grid_remove_rows(idx)
                o["grid"] = None if host is None else DeviceGrid(host, o["ctx"], o["ctx"].grid_version)
        ys = np.concatenate([np.asarray(self.objective(r), dtype=np.float64).reshape(1, -1) for r in rows], 0)   # :124
        split(ys)                                                  # (the shape check)
        self.responses = ys if self.responses is None else np.concatenate([self.responses, ys], 0)
        self.observed = rows if self.observed is None else np.concatenate([self.observed, rows], 0)            # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            Ys = split(self.responses)
            self.model.init(self.observed, Ys[0])                  # :147-149
            for o, Y in zip(self._objectives3_setup() if three else [self._objectives_setup()], Ys[1:]):
                o["model"].init(self.observed, Y)
        best = int(ys[:, 0].argmin())
        return rows[best], ys[best:best + 1]

    def _entered_front(self, rows):
        """Did a row of the last trial enter the front (rows: the front's 1-based response rows)."""
        q = int(self.config["bot"]["batch"]) if self._objectives_ts() else 1
        n = self.responses.shape[0] if q > 1 else self.nTrials    # one response row per trial unless the trial was a batch
        return any(r in rows for r in range(n - q + 1, n + 1))

    def update_best(self, x, y):
        """bots/abstract.lua:171-177; under constraints the best is the best FEASIBLE trial (column 0 among the rows with c_k <= t_k);
        under two objectives there is no single best: best["front"] / ["rows"] are the front of all trials so far under this
        trial's reference point, best["hv"] the area it dominates, best["t"] the last trial that entered the front; under three
        objectives the same with pareto_front3 and hypervolume3 (best["hv"] a volume)."""
        if self._objectives3():
            from bot7_amd import _lib
            ref = self.objectives_ref()
            front, rows = _lib.pareto_front3(self.responses, ref)
            self.best["ref"], self.best["front"], self.best["rows"] = ref, front, rows
            self.best["hv"] = _lib.hypervolume3(front, ref)
            if self._entered_front(rows):
                self.best["t"], self.best["x"], self.best["y"] = self.nTrials, x, np.asarray(y, dtype=np.float64).reshape(1, -1)
            return
        if self._objectives():
            from bot7_amd import _lib
            ref = self.objectives_ref()
            front, rows = _lib.pareto_front2(self.responses, ref)
            self.best["ref"], self.best["front"], self.best["rows"] = ref, front, rows
            self.best["hv"] = _lib.hypervolume2(front, ref)
            if self._entered_front(rows):
                self.best["t"], self.best["x"], self.best["y"] = self.nTrials, x, np.asarray(y, dtype=np.float64).reshape(1, -1)
            return
        if not self._constrained():
            return super().update_best(x, y)
        y = np.asarray(y, dtype=np.float64).reshape(1, -1)
        if feasible_rows(y, [c["threshold"] for c in self.config["bot"]["constraints"]])[0] and (
                self.best.get("y") is None or float(np.ravel(self.best["y"])[0]) > y[0, 0]):
            self.best["t"], self.best["x"], self.best["y"] = self.nTrials, x, y

    def progress_report(self, t, x, y):
        if self._objectives3():
            if self.config["bot"]["verbose"] > 0 and t % self.config["bot"]["msg_freq"] == 0:
                yy = np.ravel(y)
                print("trial %4d  y = (%.8g, %.8g, %.8g)  hypervolume3 = %-14.8g front of %d (last entry: trial %d)" %
                      (t, float(yy[0]), float(yy[1]), float(yy[2]), self.best.get("hv", 0.0), len(self.best.get("front", ())), self.best["t"]))
            return
        if self._objectives():
            if self.config["bot"]["verbose"] > 0 and t % self.config["bot"]["msg_freq"] == 0:
                yy = np.ravel(y)
                print("trial %4d  y = (%.8g, %.8g)  hypervolume = %-14.8g front of %d (last entry: trial %d)" %
                      (t, float(yy[0]), float(yy[1]), self.best.get("hv", 0.0), len(self.best.get("front", ())), self.best["t"]))
            return
        if self._constrained() and self.best.get("y") is None:
            if self.config["bot"]["verbose"] > 0 and t % self.config["bot"]["msg_freq"] == 0:
                print("trial %4d  y = %-14.8g (no feasible trial yet)" % (t, float(np.ravel(y)[0])))
            return
        super().progress_report(t, x, y)

    def _run_trial_refined(self):
        """bots/abstract.lua:112-152 with the nominee refined off the grid: the grid row the winner started from is stolen (:118),
        so the grid stops offering that neighbourhood; the objective is evaluated at the refined point (:124) and that point is
        observed (:143-144)."""
        why = refine_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))
        if why:
            raise NotImplementedError(why)
        if self.nTrials + 1 <= self.config["bot"]["nInitial"]:     # :90-91: the initial picks are grid rows
            return super().run_trial()
        self.nTrials += 1
        x, start = self.nominate_refine()                          # :117
        self._steal_candidate(start)                               # :118
        idx = self.pending.shape[0]
        self.pending[idx - 1] = x
        y = self.objective(x)                                      # :124
        y = np.asarray(y, dtype=np.float64).reshape(1, -1) if np.ndim(y) < 2 else np.asarray(y, dtype=np.float64)
        self.responses = y if self.responses is None else np.concatenate([self.responses, y], 0)
        self.observed, self.pending = T.steal(self.observed, self.pending, [idx])  # :143-144
        return x, y

    # ---- trust-region nomination (config.bot.trust_region) -------------------------------------------------------------------
    def _trust_region(self):
        """THE predicate: does this bot nominate inside a trust region."""
        return self.config["bot"].get("trust_region") is not None

    def _tr_base_grid(self, ctx, base, mins=None, maxes=None):
        """A fresh base grid of config.grid.size rows, resident only -> what it takes to make it again.  Sobol: the sequence from
        point 1 (the caller rotates it); random: a seed from the bot's generator."""
        M, d = int(self.config["grid"]["size"]), int(self.config["grid"]["dims"])
        if base == "sobol":
            made = {"base": "sobol", "skip": 1}
            ctx.grid_sobol(M, d, 1, mins, maxes, download=False)
        else:
            made = {"base": "random", "base_seed": int(self._rng.integers(0, 2 ** 63))}
            ctx.grid_random(M, d, made["base_seed"], 0, mins, maxes, download=False)
        return made

    def nominate_trust_region(self):
        """One trust-region trial's nominees (TuRBO-1: Eriksson et al., NeurIPS 2019) -> (rows q x d, the trial's trace record).
        The first nInitial trials of a run and after a restart: random rows of a fresh global base grid.  Afterwards: the hyper
        samples as _sample_hyps draws them, on the observations since the last restart; the box around the best of those
        (tr_box); a fresh base grid mapped into it on the device (grid_trust_region); the nomination through the branch the
        configuration names, on the ResidentGrid; the nominees' rows downloaded.  No row is removed: the grid is discarded."""
        from bot7_amd import _lib
        cfg, tr = self.config, self.config["bot"]["trust_region"]
        q, d, M = int(cfg["bot"]["batch"]), int(cfg["grid"]["dims"]), int(cfg["grid"]["size"])
        mins, maxes = np.asarray(cfg["grid"]["mins"], dtype=np.float64), np.asarray(cfg["grid"]["maxes"], dtype=np.float64)
        ctx = self.model.ctx
        if self.tr_state is None:
            self.tr_state = _lib.TrustRegionState(d, q, tr["length_init"], tr["length_min"], tr["length_max"], tr["success_tolerance"],
                                                  tr["failure_tolerance"])
        rec = {"trial": self.nTrials, "length_before": self.tr_state.length, "center": None, "lo": None, "hi": None, "shift": None,
               "map_seed": None, "prob": float(tr["perturb"]), "restart": False}
        if self.tr_since < cfg["bot"]["nInitial"]:
            made = self._tr_base_grid(ctx, tr["base"], mins, maxes)
            grid = ResidentGrid(ctx, ctx.grid_version, (M, d))
            if q == 1:
                idx = [int(np.floor(self._rng.random() * grid.shape[0])) + 1]      # bots/bayesopt.lua:90-91 floor(rand*M)+1
            else:
                idx = [int(i) + 1 for i in self._rng.choice(grid.shape[0], size=q, replace=False)]
            rec.update(made, kind="initial", index=idx)
            return grid.rows(idx), rec
        X_win, Y_win = self.observed[self.tr_start:], self.responses[self.tr_start:]
        hyps = self._sample_hyps(self.model, X_win, Y_win)
        col = np.where(np.isnan(Y_win[:, 0]), np.inf, Y_win[:, 0])                 # a NaN response never is the best
        center = np.array(X_win[int(np.argmin(col))], dtype=np.float64)            # the best row since the restart (the first of equals)
        lo, hi = _lib.tr_box(hyps, center, self.tr_state.length, mins, maxes)
        made = self._tr_base_grid(ctx, tr["base"])
        shift = self._rng.random(d) if tr["base"] == "sobol" else None             # a fresh Cranley-Patterson rotation per trial
        seed = int(self._rng.integers(0, 2 ** 63))
        ctx.grid_trust_region(center, lo, hi, tr["perturb"], shift=shift, seed=seed)
        grid = ResidentGrid(ctx, ctx.grid_version, (M, d))
        # the existing branches, unchanged: they see the window as the observations and the trial's hyper samples as their draws
        kept = (self.observed, self.responses, self.model)
        self.observed, self.responses, self.model = X_win, Y_win, _KeptHypers(self.model, hyps)
        refined = None
        try:
            if self._ts_refined():
                idx, refined = self.nominate_ts_refine(q, grid, lo, hi)   # the box handed to the library is the trial's trust region
            elif q > 1:
                idx = self.nominate_batch(q, grid)
            else:
                idx = [int(self.eval(grid, want_scores=False)[2])]
        finally:
            self.observed, self.responses, self.model = kept
        rec.update(made, kind="model", index=[int(i) for i in idx], center=center, lo=lo, hi=hi, shift=shift, map_seed=seed,
                   hyps=hyps)
        if refined is not None:
            rec.update(grid_rows=grid.rows(idx))
            return refined, rec
        return grid.rows(idx), rec

    def _run_trial_trust_region(self):
        """bots/abstract.lua:112-152 with the candidates made per trial inside a trust region: nothing is stolen (the grid is
        discarded), the q nominees are evaluated and observed (:124-144), the q responses resize the region (tr_update), and a
        restart moves the model's window -- observed / responses / best stay the run's record."""
        why = trust_region_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))
        if why:
            raise NotImplementedError(why)
        self.nTrials += 1
        rows, rec = self.nominate_trust_region()                   # :117
        ys = np.concatenate([np.asarray(self.objective(r), dtype=np.float64).reshape(1, -1) for r in rows], 0)   # :124
        self.responses = ys if self.responses is None else np.concatenate([self.responses, ys], 0)
        self.observed = rows if self.observed is None else np.concatenate([self.observed, rows], 0)            # :143-144
        self.tr_since += 1
        if self.model is not None and self.tr_since == self.config["bot"]["nInitial"]:
            self.model.init(self.observed[self.tr_start:], self.responses[self.tr_start:])   # :147-149, on the window
        restart = self.tr_state.update(ys[:, 0])
        if restart:
            self.tr_start, self.tr_since = self.observed.shape[0], 0
        rec.update(length_after=self.tr_state.length, restart=restart, x=rows.copy(), y=ys.copy())
        self.tr_trace.append(rec)
        best = int(np.nanargmin(ys[:, 0])) if not np.isnan(ys[:, 0]).all() else 0
        return rows[best], ys[best:best + 1]

    def run_trial(self):
        """bots/abstract.lua:112-152 with config.bot.batch nominees per trial: all of them are stolen from the candidates in one
        stable pass (:118), evaluated and observed (:124-144).  batch = 1 is the parent's loop, untouched."""
        if self._kg():
            why = kg_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))
            if why:
                raise NotImplementedError(why)
        if self.config["score"].get("refine"):
            why = ts_refine_refusal(self.config, self.model.class_() if self.model is not None else "", hasattr(self.candidates, "commit"))
            if why:
                raise NotImplementedError(why)
        if self._constrained_ts():
            return self._run_trial_constrained()                  # (every refusal of the policy, a missing constraint's included)
        if self._trust_region():
            return self._run_trial_trust_region()
        if self._objectives() or self.config["score"]["type"] in EHVI_KINDS:
            return self._run_trial_objectives()
        if self._constrained():
            return self._run_trial_constrained()
        if self.config["bot"]["refine"]:
            return self._run_trial_refined()
        if self._ts_refined() and self.nTrials + 1 > self.config["bot"]["nInitial"]:   # (:90-91: the initial picks are grid rows)
            return self._run_trial_ts_refined()
        q = int(self.config["bot"]["batch"])
        if q == 1:
            return super().run_trial()
        self.nTrials += 1
        idx = self.nominate_batch(q)                               # :117
        cand = self.candidates
        rows = np.array(np.asarray(cand)[np.asarray(idx) - 1], dtype=np.float64)
        host = T.remove(np.asarray(cand), idx)                     # :118, an index list (utils/tensor.lua:158-193)
        if isinstance(cand, DeviceGrid) and cand.ctx is not None and cand.version == cand.ctx.grid_version:
            assert np.array_equal(cand.ctx.grid_remove_rows(idx), rows)   # the same stable deletion on the resident copy
            self.candidates = None if host is None else DeviceGrid(host, cand.ctx, cand.ctx.grid_version)
        else:
            self.candidates = host
        ys = np.concatenate([np.asarray(self.objective(r), dtype=np.float64).reshape(1, -1) for r in rows], 0)   # :124
        self.responses = ys if self.responses is None else np.concatenate([self.responses, ys], 0)
        self.observed = rows if self.observed is None else np.concatenate([self.observed, rows], 0)            # :143-144
        if self.model is not None and self.nTrials == self.config["bot"]["nInitial"]:
            self.model.init(self.observed, self.responses)         # :147-149
        best = int(ys[:, 0].argmin())
        return rows[best], ys[best:best + 1]
