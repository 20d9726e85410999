"""bot7.scores registry (scores/init.lua:15-20)."""
from .abstract import abstract  # noqa: F401
from .expected_improvement import expected_improvement  # noqa: F401
from .confidence_bound import confidence_bound  # noqa: F401
from .log_expected_improvement import log_expected_improvement  # noqa: F401
from .log_probability_of_improvement import log_probability_of_improvement  # noqa: F401
from .max_value_entropy_search import max_value_entropy_search  # noqa: F401
from .thompson_sampling import thompson_sampling  # noqa: F401
from .constrained_thompson_sampling import constrained_thompson_sampling  # noqa: F401
from .knowledge_gradient import knowledge_gradient  # noqa: F401
from .expected_hypervolume_improvement import expected_hypervolume_improvement  # noqa: F401
from .log_expected_hypervolume_improvement import log_expected_hypervolume_improvement  # noqa: F401

registry = {"expected_improvement": expected_improvement, "confidence_bound": confidence_bound,
            "log_expected_improvement": log_expected_improvement,
            "log_probability_of_improvement": log_probability_of_improvement,
            "max_value_entropy_search": max_value_entropy_search, "thompson_sampling": thompson_sampling,
            "constrained_thompson_sampling": constrained_thompson_sampling,
            "knowledge_gradient": knowledge_gradient,
            "expected_hypervolume_improvement": expected_hypervolume_improvement,
            "log_expected_hypervolume_improvement": log_expected_hypervolume_improvement}
