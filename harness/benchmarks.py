"""Synthetic objectives on [0,1]^d (benchmarks/*.lua), vectorised over rows.  Host-side data generators for
the harness (the objective is the user's black box, evaluated on one point per trial: bots/abstract.lua:124);
nothing here is on the accelerated path."""
import numpy as np


def _rows(X, d=None):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim == 1:
        X = X.reshape(1, -1)
    if d is not None:
        assert X.shape[1] == d
    return X


def braninhoo(X):
    """benchmarks/braninhoo.lua:24-44; minima ~0.397887 at (0.124,0.818), (0.543,0.152), (0.962,0.165) (:12-14)."""
    X = _rows(X, 2)
    c1, c2, c3 = -5.1 / (4.0 * np.pi * np.pi), 5.0 / np.pi, 10.0 - 10.0 / (8.0 * np.pi)
    z1, z2 = X[:, 0] * 15.0 - 5.0, X[:, 1] * 15.0
    return ((z2 + z1 ** 2 * c1 + z1 * c2 - 6.0) ** 2 + (np.cos(z1) * c3 + 10.0)).reshape(-1, 1)


_H6_A = np.array([[10.0, 3.00, 17.0, 3.50, 1.70, 8.00], [0.05, 10.0, 17.0, 0.10, 8.00, 14.0],
                  [3.00, 3.50, 1.70, 10.0, 17.0, 8.00], [17.0, 8.00, 0.05, 10.0, 0.10, 14.0]])
_H6_P = np.array([[.1312, .1696, .5569, .0124, .8283, .5886], [.2329, .4135, .8307, .3736, .1004, .9991],
                  [.2348, .1451, .3522, .2883, .3047, .6650], [.4047, .8828, .8732, .5743, .1091, .0381]])
_H6_a = np.array([1.0, 1.2, 3.0, 3.2])


def hartmann6(X):
    """benchmarks/hartmann6.lua:36-63; f* = -3.32237 at (.201690,.150011,.476874,.275332,.311652,.657300) (:24-26)."""
    X = _rows(X, 6)
    inner = -np.einsum("kj,nkj->nk", _H6_A, (X[:, None, :] - _H6_P[None]) ** 2)
    return (-(np.exp(inner) @ _H6_a)).reshape(-1, 1)


def ackley(X):
    """benchmarks/ackley.lua:28-49; 0 at x = 0.5 (:16-17)."""
    Z = (_rows(X) - 0.5) * 65.536
    a, b, c, d = 20.0, -0.2, 2.0 * np.pi, np.exp(1.0)
    return (np.exp(np.sqrt((Z ** 2).mean(1)) * b) * -a - np.exp(np.cos(Z * c).mean(1)) + (a + d)).reshape(-1, 1)


def rastrigin(X):
    """benchmarks/rastrigin.lua:26-45."""
    Z = (_rows(X) - 0.5) * 10.24
    a, b = 10.0, 2.0 * np.pi
    return ((Z ** 2 + np.cos(Z * b) * -a).sum(1) + a * Z.shape[1]).reshape(-1, 1)


GARDNER1_THRESHOLD = 0.5


def gardner1(X):
    """A CONSTRAINED toy (no counterpart in benchmarks/): the first simulation of Gardner et al., "Bayesian Optimization with
    Inequality Constraints", ICML 2014.  With x = 6 X over [0, 6]^2: minimise cos(2 x1) cos(x2) + sin(x1) subject to
    cos(x1) cos(x2) - sin(x1) sin(x2) <= 0.5.  Returns rows [y, c]: the objective and the constraint function, whose threshold is
    GARDNER1_THRESHOLD (config.bot.constraints = [{"threshold": 0.5, "model": {...}}])."""
    Z = _rows(X, 2) * 6.0
    x1, x2 = Z[:, 0], Z[:, 1]
    y = np.cos(2.0 * x1) * np.cos(x2) + np.sin(x1)
    c = np.cos(x1) * np.cos(x2) - np.sin(x1) * np.sin(x2)
    return np.stack([y, c], axis=1)


def gardner1_hidden(X):
    """gardner1 with the constraint HIDDEN behind an outcome (no counterpart in benchmarks/): rows [y, v] with v = 1 where gardner1's
    constraint is violated (c > GARDNER1_THRESHOLD) and 0 where it holds, and y = NaN wherever v = 1 -- the run failed, there is no
    objective value (config.bot.constraints = [{"threshold": 0.5, "binary": True, "model": {"type": "gp_classifier", ...}}])."""
    R = gardner1(X)
    bad = R[:, 1] > GARDNER1_THRESHOLD
    return np.stack([np.where(bad, np.nan, R[:, 0]), bad.astype(np.float64)], axis=1)


def two_spheres(X):
    """A TWO-OBJECTIVE toy (no counterpart in benchmarks/), any dims: rows [y1, y2] = (|x - a|^2, |x - b|^2) with a = 0.25 * 1 and
    b = 0.75 * 1, both minimised.  Its Pareto set is the segment between a and b (config.bot.objectives = {"ref": ..., "model": ...})."""
    X = _rows(X)
    return np.stack([((X - 0.25) ** 2).sum(1), ((X - 0.75) ** 2).sum(1)], axis=1)


def three_spheres(X):
    """A THREE-OBJECTIVE toy (no counterpart in benchmarks/), any dims: rows [y1, y2, y3] = (|x - a|^2, |x - b|^2, |x - c|^2) with
    a = 0.25 * 1, b = 0.5 * 1 and c = 0.75 * 1, all minimised.  The three centres lie on one line, so the Pareto set is their convex
    hull, the segment between a and c: off the diagonal every distance shrinks under projection onto it, and beyond either end moving
    to the end lowers all three (config.bot.objectives = {"ref": ..., "models": [..., ...]})."""
    X = _rows(X)
    return np.stack([((X - 0.25) ** 2).sum(1), ((X - 0.5) ** 2).sum(1), ((X - 0.75) ** 2).sum(1)], axis=1)


registry = {"braninhoo": braninhoo, "hartmann6": hartmann6, "ackley": ackley, "rastrigin": rastrigin, "gardner1": gardner1, "gardner1_hidden": gardner1_hidden,
            "two_spheres": two_spheres, "three_spheres": three_spheres}
