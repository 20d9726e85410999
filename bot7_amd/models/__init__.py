"""bot7.models registry.  In the reference this table IS ``require('gp.models')`` plus ``abstract`` and ``dngo``
(models/init.lua:15-17); here ``gp_regressor`` is the HIP-backed drop-in for gp.models.gp_regressor, and ``gp_classifier`` has no counterpart there."""
from .abstract import abstract  # noqa: F401
from .gp_regressor import gp_regressor  # noqa: F401
from .dngo import dngo  # noqa: F401
from .gp_classifier import gp_classifier  # noqa: F401  (ours: the probit classifier of a binary constraint)

registry = {"gp_regressor": gp_regressor, "dngo": dngo, "gp_classifier": gp_classifier}
