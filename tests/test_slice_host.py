"""The device slice sampler's host side (no GPU): tests/_slice_ref.py -- the restatement the GPU replay holds the kernel to -- is
pinned to harness/samplers/slice.py, the line-cited mirror of samplers/slice.lua; the counter layout; the exports; the model's
pool logic on a stand-in context."""
import math
import types

import numpy as np
import pytest

import bot7_amd
from bot7_amd import _lib
from harness.samplers import slice as H

import _slice_ref as R


# ---- 1. same sequence as the harness sampler ---------------------------------------------------------------------------------------
class RngAdapter(object):
    """One numpy Generator behind both samplers' draws: the restatement asks for them in the order the harness sampler
    consumes them (direction normals, u_Y, the `right` uniforms, then one uniform per shrink step)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def normals(self, g, D):
        return list(self.rng.standard_normal((1, D))[0])

    def log_u_Y(self, g):
        return float(np.log(self.rng.random()))

    def u_right(self, g, D):
        return list(self.rng.random((1, D))[0])

    def u_shrink(self, g, i):
        return float(self.rng.random())


def gaussian_density(D, seed):
    """A correlated Gaussian log-density, as plain Python arithmetic on lists (both samplers call the same function)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(D, D)) / math.sqrt(D)
    P = A @ A.T + 0.5 * np.eye(D)   # precision
    Pl = [[float(v) for v in row] for row in P]

    def f(t):
        q = 0.0
        for i in range(D):
            s = 0.0
            for j in range(D):
                s += Pl[i][j] * t[j]
            q += t[i] * s
        return -0.5 * q
    return f


def sequential_norm(x):
    """sqrt of the ascending sum of squares: the kernel's (and the restatement's) norm."""
    ss = 0.0
    for v in np.asarray(x, dtype=np.float64).ravel():
        ss = ss + float(v) * float(v)
    return math.sqrt(ss)


def harness_chain(f, theta0, lo, hi, widths, U, seed, exact_norm, max_step=1000):
    """U updates of harness/samplers/slice.py over the bounded density, every request recorded.  exact_norm: the sampler's
    np.linalg.norm replaced by the sequential one (numpy's may sum in another order: the last bit of the direction)."""
    requests = []

    def density(t, _args):
        t = [float(v) for v in np.asarray(t).ravel()]
        inb = all(t[k] >= lo[k] and t[k] <= hi[k] for k in range(len(t)))
        v = f(t) if inb else -math.inf
        requests.append((t, v))
        return v

    opt = H.slice_sampler.configure({"widths": np.asarray(widths), "max_step": max_step, "rng": np.random.default_rng(seed)})
    saved = H.np
    if exact_norm:
        shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
        shim.linalg = types.SimpleNamespace(norm=sequential_norm)
        H.np = shim
    try:
        theta, out = np.asarray(theta0, dtype=np.float64), []
        for _ in range(U):
            theta = H.slice_sampler.sample(density, theta.reshape(1, -1), dict(opt, nSamples=1), None)[0]
            out.append(theta.copy())
    finally:
        H.np = saved
    return out, requests


@pytest.mark.parametrize("D,seed", [(4, 3), (9, 8)])
def test_restatement_is_the_harness_sampler(D, seed):
    f = gaussian_density(D, seed)
    lo, hi, widths = [-1.2] * D, [1.2] * D, [1.0 + 0.1 * k for k in range(D)]
    theta0, U = [0.1 * (k - D / 2) for k in range(D)], 25
    ref = R.slice_chain(f, RngAdapter(seed), theta0, lo, hi, widths, U)
    # the same draws, the sampler's own norm replaced by the sequential one: the same requests and samples, exactly
    out, requests = harness_chain(f, theta0, lo, hi, widths, U, seed, exact_norm=True)
    assert len(requests) == len(ref["requests"])
    for (t, v), r in zip(requests, ref["requests"]):
        assert np.array_equal(t, r["theta"]) and (v == r["value"])
    assert all(np.array_equal(a, b) for a, b in zip(out, ref["theta"]))
    assert ref["status"] == [0] * U
    assert any(not r["in_bounds"] for r in ref["requests"]), "the bounds were never hit: the case does not test them"
    assert sum(r["reused"] for r in ref["requests"]) == U - 1 and ref["nevals"] == sum(
        r["in_bounds"] and not r["reused"] for r in ref["requests"])
    # ... and with numpy's own norm: the same decisions, the points within a few ulp of the direction's last bit
    out2, requests2 = harness_chain(f, theta0, lo, hi, widths, U, seed, exact_norm=False)
    assert len(requests2) == len(requests)
    assert all(np.allclose(a, b, rtol=0, atol=1e-13) for a, b in zip(out2, out))


def test_evaluation_cap_returns_x0():
    D, seed = 4, 3
    f = gaussian_density(D, seed)
    lo, hi, widths, theta0 = [-1.2] * D, [1.2] * D, [1.0] * D, [0.05] * D
    full = R.slice_chain(f, RngAdapter(seed), theta0, lo, hi, widths, 6)
    per_update = [sum(r["g"] == g for r in full["requests"]) for g in range(6)]
    assert min(per_update) >= 4 and max(per_update) > 4
    capped = R.slice_chain(f, RngAdapter(seed), theta0, lo, hi, widths, 1, max_evals=3)
    assert capped["status"] == [R.ST_CAP] and capped["theta"][0] == theta0 and capped["value"][0] == f(theta0)
    assert [r["theta"] for r in capped["requests"]] == [r["theta"] for r in full["requests"][:3]]   # a prefix of the uncapped run
    # the next update proceeds from x0, its start value reused
    two = R.slice_chain(f, RngAdapter(seed), theta0, lo, hi, widths, 2, max_evals=per_update[0])
    assert two["status"][0] == 0 and two["requests"][per_update[0]]["reused"]


class Scripted(object):
    """Draws that drive an update into the shrank-to-zero branch: u_Y = 1 (log 0: the level is f(x0) itself), right uniforms
    1/2 (left = -right) and a first shrink uniform of 1/2 (dx = 0 exactly)."""

    def __init__(self, D):
        self.D = D

    def normals(self, g, D):
        return [1.0] + [0.5] * (D - 1)

    def log_u_Y(self, g):
        return 0.0

    def u_right(self, g, D):
        return [0.5] * D

    def u_shrink(self, g, i):
        return 0.5

    # the harness sampler's Generator interface, the same numbers: its first scalar uniform is u_Y, the later ones shrink steps
    def standard_normal(self, shape):
        return np.asarray(self.normals(0, self.D)).reshape(shape)

    def random(self, shape=None):
        if shape is not None:
            return np.full(shape, 0.5)
        self.scalars = getattr(self, "scalars", 0) + 1
        return 1.0 if self.scalars == 1 else 0.5


def test_shrank_to_zero_branch(capsys):
    D = 4
    f = gaussian_density(D, 1)
    lo, hi, widths, theta0 = [-9.0] * D, [9.0] * D, [0.25] * D, [0.0] * D   # the mode: no step-out, and f(x0 + 0) is not above f(x0)
    ref = R.slice_chain(f, Scripted(D), theta0, lo, hi, widths, 1)
    assert ref["status"] == [R.ST_ZERO] and ref["theta"][0] == theta0 and ref["value"][0] == f(theta0)
    opt = H.slice_sampler.configure({"widths": np.asarray(widths), "rng": Scripted(D)})
    got = H.slice_sampler.sample(lambda t, _a: f([float(v) for v in np.asarray(t).ravel()]), np.asarray(theta0).reshape(1, -1),
                                 dict(opt, nSamples=1), None)[0]
    assert "shrank to zero" in capsys.readouterr().out and np.array_equal(got, theta0)


def test_nan_density_takes_the_point():
    D = 4
    calls = []

    def f(t):
        calls.append(t)
        # (a peak far narrower than the widths: no step-out) start, right, left, then the first shrink: NaN
        return math.nan if len(calls) == 4 else -1e6 * sum(v * v for v in t)
    ref = R.slice_chain(f, RngAdapter(11), [0.0] * D, [-50.0] * D, [50.0] * D, [1.0] * D, 1)
    assert ref["status"] == [R.ST_NAN] and ref["value"][0] != ref["value"][0] and ref["theta"][0] == calls[3]


def test_failed_pivot_stops_the_chain():
    D = 4
    n = [0]

    def f(t):
        n[0] += 1
        return (0.0, True) if n[0] == 6 else -0.5 * sum(v * v for v in t)
    ref = R.slice_chain(f, RngAdapter(5), [0.1] * D, [-5.0] * D, [5.0] * D, [1.0] * D, 4)
    first = next(u for u in range(4) if ref["status"][u] & R.ST_PIVOT)
    assert all(s == R.ST_NOT_RUN for s in ref["status"][first + 1:]) and first < 3
    last_good = [0.1] * D if first == 0 else ref["theta"][first - 1]
    assert all(ref["theta"][u] == last_good for u in range(first, 4)) and ref["nevals"] == 6


# ---- 2. the counter layout ----------------------------------------------------------------------------------------------------------
def test_counter_generator_known_values():
    """splitmix64's published outputs for seed 0 (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F) are the words of
    counters 0 and 1 under key 0; a uniform is the word's top 53 bits, an exact integer times 2^-53."""
    assert R.counter_bits(0, 0) == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
    assert R.counter_bits(0, 1)[0] == 0x06C45D188009454F
    u = R.counter_uniform(0, 0)
    assert u * 2.0 ** 53 == float(0xE220A8397B1DCDAF >> 11) and 0.0 <= u < 1.0
    assert R.counter_uniform(0, 1) * 2.0 ** 53 == float(0x06C45D188009454F >> 11)
    assert R.counter_key(7, 0) == R.splitmix64(R.splitmix64(7)) and R.counter_key(7, 3) == R.splitmix64(R.splitmix64(7) ^ 3)
    for key, ctr in ((R.counter_key(1234, 2), 4096 * 5 + 64), (R.counter_key(99, 0), 4096 * 77 + 256 + 3839)):
        v = R.counter_uniform(key, ctr) * 2.0 ** 53
        assert v == math.floor(v) and 0 <= v < 2 ** 53


def test_counter_streams_do_not_overlap():
    """d + 3 = 35 components and 3 840 shrink steps: an update's four streams are disjoint and stay inside its 4 096 counters."""
    D, shrinks = 35, _lib_caps()["max_evals"]
    z = {R.CTR_Z + k for k in range(D)}
    uy = {R.CTR_UY}
    right = {R.CTR_RIGHT + k for k in range(D)}
    shrink = {R.CTR_SHRINK + i for i in range(shrinks)}
    every = [z, uy, right, shrink]
    assert sum(len(s) for s in every) == len(set().union(*every))
    assert max(set().union(*every)) < R.CTR_STRIDE and min(set().union(*every)) >= 0
    # and the draws behind them differ: no two counters of an update share a word
    key = R.counter_key(5, 1)
    words = [R.counter_bits(key, R.CTR_STRIDE * 9 + c)[0] for c in sorted(set().union(*every))]
    assert len(set(words)) == len(words)
    d = R.CounterDraws(5, 1)
    assert d.u_shrink(9, 0) == R.counter_uniform(key, R.CTR_STRIDE * 9 + 256) and d.u_Y(9) == R.counter_uniform(key, R.CTR_STRIDE * 9 + 64)
    assert d.normals(9, 3)[2] == R.counter_normal(key, R.CTR_STRIDE * 9 + 2)


def _lib_caps():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bot7hip.h")).read()
    g = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1))   # noqa: E731
    return {"max_evals": g("B7_SLICE_MAX_EVALS"), "chains": g("B7_SLICE_MAX_CHAINS"), "work": g("B7_SLICE_MAX_WORK"),
            "width": g("B7_SLICE_TRACE_WIDTH")}


# ---- 3. exports ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_constants():
    for name in ("b7_gp_slice_sample", "b7_gp_slice_trace_enable", "b7_gp_slice_trace"):
        assert name in _lib.SYMBOLS
    caps = _lib_caps()
    assert caps == {"max_evals": 3840, "chains": 256, "work": 65536, "width": _lib.SLICE_TRACE_WIDTH}
    assert (_lib.SLICE_NAN, _lib.SLICE_ZERO, _lib.SLICE_CAP, _lib.SLICE_PIVOT, _lib.SLICE_NOT_RUN) == (
        R.ST_NAN, R.ST_ZERO, R.ST_CAP, R.ST_PIVOT, R.ST_NOT_RUN)
    assert hasattr(bot7_amd.Context, "gp_slice_sample") and hasattr(bot7_amd.Context, "gp_slice_trace")


# ---- 4. the model's pool logic on a stand-in context ----------------------------------------------------------------------------------
class StandIn(object):
    """A context that answers gp_slice_sample with recognisable numbers: theta[c][u] = start[c] + (update0 + u + 1) * 1e-3."""

    def __init__(self, stop_chain=None):
        self.fit_token, self.calls, self.stop_chain, self.nll_calls = 0, [], stop_chain, 0

    def gp_set_data(self, X, Y):
        self.fit_token += 1

    def gp_slice_sample(self, theta0, lo, hi, widths, U, seed, update0=0, max_step=1000, max_evals=512, gibbs=False, logspace=True):
        if gibbs:
            raise bot7_amd.Bot7HipError(-5, "gp_slice_sample: Gibbs updates are not built on the device")
        t0 = np.atleast_2d(theta0)
        self.calls.append({"C": t0.shape[0], "U": U, "update0": update0, "seed": seed, "widths": np.asarray(widths).copy()})
        theta = np.stack([[t0[c] + (update0 + u + 1) * 1e-3 for u in range(U)] for c in range(t0.shape[0])])
        status = np.zeros((t0.shape[0], U), dtype=np.int32)
        if self.stop_chain is not None and len(self.calls) == 1:
            status[self.stop_chain, 1], status[self.stop_chain, 2:] = 8, 16
            theta[self.stop_chain, 1:] = theta[self.stop_chain, 0]
        return {"theta": theta, "value": np.zeros((t0.shape[0], U)), "status": status, "nevals": np.full(t0.shape[0], 7 * U, dtype=np.int32)}

    def gp_nll1(self, ls, amp, noise, mean):
        self.nll_calls += 1
        return 0.5 * float(np.sum(np.log(ls) ** 2)), 1e-9, 0   # a jittered evaluation


def data(n=12, d=2, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, d)), rng.normal(size=(n, 1))


def test_pool_is_served_update_by_update_and_keyed_on_the_data():
    ctx = StandIn()
    m = bot7_amd.models.gp_regressor({"sample": True, "sampler": "slice_device", "chains": 2, "prefetch": 3, "nBurnin": 4, "seed": 9},
                                     context=ctx)
    X, Y = data()
    m.sample_hypers(X, Y)                                   # burn-in: ONE call of nBurnin updates of both chains
    assert [(c["C"], c["U"], c["update0"]) for c in ctx.calls] == [(2, 4, 0)]
    assert np.array_equal(ctx.calls[0]["widths"], np.full(5, 0.5))
    start = m._dev["thetas"].copy()
    got = [m._to_theta(m.parse_hypers(m.sample_hypers(X, Y, None, None, True))) for _ in range(6)]
    assert [(c["C"], c["U"], c["update0"]) for c in ctx.calls[1:]] == [(2, 3, 4)]          # one refill served six samples
    want = [start[c] + (4 + u + 1) * 1e-3 for u in range(3) for c in range(2)]             # update by update, chain after chain
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    m.sample_hypers(X, Y, None, None, True)                 # the pool is empty: the next launch, update numbers move on
    assert (ctx.calls[-1]["U"], ctx.calls[-1]["update0"]) == (3, 7) and len(m._dev["pool"]) == 5
    X2, Y2 = data(13)
    m.sample_hypers(X2, Y2, None, None, True)               # new data: the pool is dropped, not served
    assert (ctx.calls[-1]["update0"], len(ctx.calls)) == (10, 4) and len(m._dev["pool"]) == 5
    assert m.nDeviceCalls == 4 and m.nEvals == 7 * 2 * (4 + 3 + 3 + 3)


def test_stopped_chain_finishes_on_the_host_sampler():
    import harness.samplers  # noqa: F401  (registers 'slice')
    ctx = StandIn(stop_chain=1)
    m = bot7_amd.models.gp_regressor({"sample": True, "sampler": "slice_device", "chains": 2, "nBurnin": 4, "seed": 2}, context=ctx)
    X, Y = data()
    m.sample_hypers(X, Y)
    lo, hi = m._bounds(X, Y)
    assert m._dev["host_calls"] == 1 and ctx.nll_calls > 0 and m.last_fit["jitter"] > 0.0
    assert ((m._dev["thetas"] >= lo) & (m._dev["thetas"] <= hi)).all()
    assert not np.array_equal(m._dev["thetas"][1], m._dev["thetas"][0])


def test_limits_are_named():
    rng = np.random.default_rng(0)
    for shape, cols, word in (((129, 2), 1, "N <= 128"), ((5, 33), 1, "d <= 32"), ((5, 2), 2, "one response column")):
        m = bot7_amd.models.gp_regressor({"sample": True, "sampler": "slice_device"}, context=StandIn())
        with pytest.raises(NotImplementedError) as e:
            m.sample_hypers(rng.random(shape), rng.normal(size=(shape[0], cols)), None, None, True)
        assert word in str(e.value)
    g = bot7_amd.models.gp_regressor({"sample": True, "sampler": "slice_device", "sampler_opt": {"gibbs": True}}, context=StandIn())
    with pytest.raises(bot7_amd.Bot7HipError) as e:
        g.sample_hypers(*data(), None, None, True)
    assert e.value.code == -5 and "Gibbs" in str(e.value)


def test_bot_sets_prefetch_to_nsamples():
    """The bot's configure step (its constructor goes on to build a grid on the device): prefetch := nSamples for slice_device only."""
    from harness import bots
    bot = object.__new__(bots.bayesopt)
    bot.hypers = []
    cfg = bot.configure({"bot": {"verbose": 0, "budget": 5, "nInitial": 2, "nSamples": 7, "seed": 1},
                         "grid": {"type": "sobol", "size": 64, "dims": 6},
                         "model": {"type": "gp_regressor", "sample": True, "sampler": "slice_device"}})
    assert cfg["model"]["prefetch"] == 7 and cfg["model"]["sampler"] == "slice_device"
    cfg = bot.configure({"bot": {"verbose": 0, "budget": 5, "nInitial": 2, "nSamples": 7, "seed": 1},
                         "grid": {"type": "sobol", "size": 64, "dims": 6}, "model": {"type": "gp_regressor", "sample": True}})
    assert "prefetch" not in cfg["model"] and cfg["model"]["sampler"] == "slice"
