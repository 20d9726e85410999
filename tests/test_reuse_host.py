"""The context-reuse catalogue (tests/_reuse_calls.py) without a GPU: it names every public method of bot7_amd.Context, and its
walk-and-compare machinery -- the one tests/test_gpu_reuse.py runs on the device -- passes an honest host context and catches two
deliberately leaky ones, naming the step and the call."""
import numpy as np
import pytest

import _reuse_calls as R
from bot7_amd import _lib
from oracle.hostctx import OracleContext

# the entries OracleContext can answer; the ones that change the grid first, so that a step ends on an accumulator of M rows
HOST_CALLS = ["gp_set_data", "nominate_commit", "grid_upload", "gp_nll_batch", "score_ei", "eval_nominate[cb,S]"]


class HostCtx(OracleContext):
    """OracleContext behind the few more spellings the catalogue's entries use (options the oracle has no use for, the fit and
    the prediction as two calls, the report of eval_nominate)."""

    def gp_set_opts(self, **kw):
        assert not kw

    def mes_set_levels(self, K):
        pass

    def gp_set_kernel(self, kernel):
        assert kernel == "ardse"

    def gp_fit_hyp(self, lenscale_sq, amp, noise, mean, want_nll=False):
        self.f = self.gp.fit(self.X_obs, self.Y, lenscale_sq, amp, noise, mean)
        return {"nll": np.asarray(self.f.nll, dtype=np.float64), "jitter": self.f.jitter, "info": self.f.info}

    def gp_predict(self, download=True):
        self.mu, self.var = self.gp.predict(self.f, self.X)
        return (self.mu, self.var) if download else (None, None)

    def score_cb(self, tradeoff=1.0, upper=False, sign=-1.0):
        OracleContext.score_cb(self, tradeoff, upper, sign)

    def eval_nominate(self, hyps, score="ei", fmin=None, want_report=False, levels=None, **kw):
        v, i = OracleContext.eval_nominate(self, hyps, score=score, fmin=fmin, **kw)
        if want_report:
            return v, i, {"jitter": np.zeros(len(hyps)), "info": np.zeros(len(hyps), dtype=np.int32)}
        return v, i

    def nominate_commit(self, idx1_global, global_row_offset=0):
        return OracleContext.nominate_commit(self, idx1_global, global_row_offset)


class KeepsTrailingRows(HostCtx):
    """The leak of a grow-only observation buffer: when N shrinks, the old data set's trailing rows stay behind the new ones."""

    def gp_set_data(self, X_obs, Y):
        X_obs, Y = np.asarray(X_obs, dtype=np.float64), np.asarray(Y, dtype=np.float64).reshape(len(X_obs), -1)
        old = getattr(self, "_buf", None)
        if old is not None and old[0].shape[0] > X_obs.shape[0] and old[0].shape[1] == X_obs.shape[1]:
            X_obs, Y = np.concatenate([X_obs, old[0][X_obs.shape[0]:]]), np.concatenate([Y, old[1][Y.shape[0]:]])
        self._buf = (X_obs, Y)
        HostCtx.gp_set_data(self, X_obs, Y)


class KeepsAccumulator(HostCtx):
    """The leak of a flag: a grid change that leaves M as it was does not forget the accumulator, so the reset behind it finds it
    `still valid` and leaves the old sums in place."""

    def grid_upload(self, X):
        X = np.array(X, dtype=np.float64)
        self._stale = getattr(self, "_stale", False) or (self.X is not None and self.X.shape == X.shape and not np.array_equal(self.X, X))
        HostCtx.grid_upload(self, X)

    def score_reset(self):
        stale, self._stale = getattr(self, "_stale", False), False
        if stale and self.acc is not None and self.acc.shape[0] == self.X.shape[0]:
            return
        HostCtx.score_reset(self)


# small on purpose: the oracle's fits are host work, and the two leaks show at any size
STEPS = [("big", R.problem(16, 2, 40, 2, seed=10, name="big")), ("small", R.problem(10, 2, 30, 2, seed=11, name="small")),
         ("same-M", R.problem(10, 2, 30, 2, seed=12, name="same-M"))]


def _walk(cls, cache):
    w = R.Walker(lambda: (cls(), None, None), lambda partners: (HostCtx(), None, None, lambda: None), names=HOST_CALLS, cache=cache)
    w.fill(STEPS[0][1])
    for step, P in STEPS[1:]:
        w.step(step, P)
    return w


@pytest.fixture(scope="module")
def cache():
    return {}


def test_every_public_method_is_named_by_an_entry_or_exempt():
    public = R.public_methods(_lib.Context)
    assert len(public) > 90, public
    named = R.covered()
    assert [m for m in public if m not in named] == [], "add a CALLS entry (or an EXEMPT reason) to tests/_reuse_calls.py"
    assert sorted(named - set(public)) == [], "the catalogue names methods bot7_amd.Context does not have"
    both = [m for m in R.EXEMPT if any(m in c.methods for c in R.CALLS.values())]
    assert both == []
    assert all(isinstance(r, str) and r for r in R.EXEMPT.values())


def test_the_problem_generator_is_deterministic_and_well_conditioned():
    P, Q = R.problem(25, 3, 130, 2, seed=1), R.problem(25, 3, 130, 2, seed=1)
    assert P.key == Q.key and all(np.array_equal(getattr(P, k), getattr(Q, k)) for k in ("X", "Y", "Y2", "Y3", "G", "pend", "logw"))
    assert P.X.min() >= 0.0 and P.X.max() < 1.0 and P.Y.shape == (25, 1) and len(P.hyps) == 2
    for s, h in enumerate(P.hyps):
        assert np.allclose(h["lenscale_sq"], 3 / 8.0 * (1 + 0.25 * s)) and h["noise"] == 1e-3 * h["amp"]
    assert not np.array_equal(R.problem(25, 3, 130, 2, seed=2).X, P.X)
    big = R.problem(25, 3, 130, 2, seed=1, scale=1e6)
    assert np.array_equal(big.Y, 1e6 * P.Y)
    J = R.problem(40, 3, 130, 1, seed=3, dup_rows=8, zero_noise=True)
    assert np.array_equal(J.X[8:16], J.X[:8]) and np.array_equal(J.Y[8:16], J.Y[:8]) and J.hyps[0]["noise"] == 0.0


def test_an_honest_host_context_passes_the_walk(cache):
    w = _walk(HostCtx, cache)
    assert w.compared == 2 * len(HOST_CALLS) and w.refused == set()


def test_a_refusal_is_a_result_and_must_be_the_same_on_both_sides():
    ok = {"x": b"\0" * 8}
    ref = ("refused", -4, "B7_ERR_STATE (-4): no fit")
    assert R.first_difference(ref, ref) is None and R.first_difference(ok, dict(ok)) is None
    assert "refusal differs" in R.first_difference(ref, ok)
    assert "refusal differs" in R.first_difference(ref, ("refused", -5, ref[2]))
    nan = {"x": np.array([np.nan]).tobytes()}
    assert R.first_difference(nan, nan) is None and R.all_finite(nan) == ["x"]   # equal NaNs compare equal: all_finite is what refuses them
    assert R.all_finite({"x": np.array([-np.inf, 1.0]).tobytes(), "idx": 3}) == []
    one_bit = {"x": (np.array([1.0]).view(np.uint64) + 1).tobytes()}
    assert "1 of 1 words differ" in R.first_difference(one_bit, {"x": np.array([1.0]).tobytes()})


def test_trailing_observation_rows_kept_when_n_shrinks_are_caught(cache):
    with pytest.raises(R.Mismatch) as e:
        _walk(KeepsTrailingRows, cache)
    assert "step 'small'" in str(e.value) and "call 'gp_set_data'" in str(e.value), str(e.value)


def test_an_accumulator_kept_across_a_grid_change_of_the_same_m_is_caught(cache):
    with pytest.raises(R.Mismatch) as e:
        _walk(KeepsAccumulator, cache)
    assert "step 'same-M'" in str(e.value) and "call 'nominate_commit'" in str(e.value), str(e.value)


def test_expected_refusals_follow_the_shape():
    A, B, E = R.problem(25, 3, 130, 2, seed=1), R.problem(129, 6, 300, 3, seed=2), R.problem(70, 4, 150, 1, seed=3, ycols=7)
    assert [n for n in R.CALLS if R.expected_refusal(n, A)] == ["blr_eval_nominate[mes]", "blr_eval_nominate_marg[mes]", "head_then_kg",
                                                                "head_then_mes", "head_then_batch"]
    assert R.expected_refusal("gp_slice_sample", B) == R.UNSUPPORTED and R.expected_refusal("gp_slice_sample", A) is None
    assert R.expected_refusal("kg_nominate", E) == R.UNSUPPORTED and R.expected_refusal("eval_nominate[ei,S]", E) is None
