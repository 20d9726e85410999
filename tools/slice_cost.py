"""What the device slice sampler saves, or does not: hartmann6, d = 6, N in {25, 64, 100} observations, ten hyper vectors per trial
(the `default` workload's sampling), three arms timed in the same run:
  host     config.sampler = 'slice': the host sampler, one b7_gp_nll_batch (B = 1) per density evaluation,
  dev_1x10 'slice_device', C = 1 chain of U = 10 updates in one launch,
  dev_10x1 'slice_device', C = 10 chains of U = 1 update in one launch.
Per arm and N: likelihood evaluations per trial, wall time of a trial's sampling (median, min .. max over the rounds), and for
the device arms the in-kernel time per evaluation from the trace's wall-clock ticks (100 MHz), the first evaluation of a launch
(cold instruction cache) against the later ones.  Also: the b7_gp_nll_batch (B = 1) call time at each N as medians of repeats
(their spread is the margin a comparison with another build of the library has), and the `default` workload's trials per
second through the harness bot (harness/default_regime.py) under each sampler.  The script runs on a tree without
b7_gp_slice_sample as well (the arms that need it are left out): run it there for the figures to set beside these.
Prints one JSON object.
usage (GPU box): python tools/slice_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402
from harness import benchmarks, default_regime  # noqa: E402
import harness.samplers  # noqa: E402,F401

NS, S, ROUNDS, WARM = (25, 64, 100), 10, 15, 3
HAVE = hasattr(bot7_amd.Context, "gp_slice_sample")


def stats(ts, scale=1e3, unit="ms"):
    ts = np.asarray(ts) * scale
    return {"median_" + unit: round(float(np.median(ts)), 4), "min_" + unit: round(float(ts.min()), 4), "max_" + unit: round(float(ts.max()), 4)}


def trial(model, X, Y):
    """One trial's sampling as the bot does it: the burn-in call, then S per-sample calls."""
    model.sample_hypers(X, Y)
    for _ in range(S):
        model.sample_hypers(X, Y, None, None, True)


def arm(c, X, Y, cfg):
    model = bot7_amd.models.gp_regressor(dict({"sample": True, "nBurnin": 0, "seed": 6}, **cfg), context=c)
    for _ in range(WARM):
        trial(model, X, Y)
    ts, ev = [], []
    for _ in range(ROUNDS):
        e0 = getattr(model, "nEvals", 0)
        t0 = time.perf_counter()
        trial(model, X, Y)
        ts.append(time.perf_counter() - t0)
        ev.append(getattr(model, "nEvals", 0) - e0)
    r = stats(ts)
    r["evaluations_per_trial"] = round(float(np.mean(ev)), 1)
    r["us_per_evaluation"] = round(1e6 * float(np.sum(ts)) / max(1, int(np.sum(ev))), 2)
    return r


def in_kernel(c, X, Y, C, U):
    """Ticks of every evaluation of a traced launch: the first of each chain against the rest."""
    model = bot7_amd.models.gp_regressor({}, context=c)
    X = np.asarray(X, dtype=np.float64)
    model.init(X, Y)
    lo, hi = model._bounds_compute(X, Y)
    t0 = np.tile(model._to_theta(model.hyp), (C, 1))
    c.gp_set_data(X, Y)
    first, later = [], []
    c.gp_slice_trace_enable(4096)
    for rep in range(5):
        c.gp_slice_sample(t0, lo, hi, np.full(lo.size, 0.5), U, 100 + rep)
        for ch in range(C):
            tk = [r["ticks"] for r in c.gp_slice_trace(ch) if r["type"] == "request" and r["ticks"] > 0]
            first += tk[:1]
            later += tk[1:]
    c.gp_slice_trace_enable(0)
    out = {"first_us": round(float(np.median(first)) / 100.0, 2)}
    if later:
        out["later_us"] = round(float(np.median(later)) / 100.0, 2)
    return out


out = {"have_slice_device": HAVE, "samples_per_trial": S}
c = bot7_amd.Context(0)
pool = c.grid_sobol(256, 6, 1)
for N in NS:
    X = pool[:N].copy()
    Y = benchmarks.hartmann6(X).reshape(N, 1)
    r = {"host": arm(c, X, Y, {})}
    if HAVE:
        r["dev_1x10"] = arm(c, X, Y, {"sampler": "slice_device", "chains": 1, "prefetch": S})
        r["dev_10x1"] = arm(c, X, Y, {"sampler": "slice_device", "chains": S, "prefetch": 1})
        r["dev_1x10"]["in_kernel"] = in_kernel(c, X, Y, 1, S)
        r["dev_10x1"]["in_kernel"] = in_kernel(c, X, Y, S, 1)
    # b7_gp_nll_batch, B = 1: medians of 7 repeats of 2000 calls
    c.gp_set_data(X, Y)
    ls, amp = np.full(6, 0.75), float(np.var(Y))
    for _ in range(500):
        c.gp_nll1(ls, amp, 1e-4 * amp, float(Y.mean()))
    reps = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(2000):
            c.gp_nll1(ls, amp, 1e-4 * amp, float(Y.mean()))
        reps.append((time.perf_counter() - t0) / 2000)
    r["nll_batch_b1_call"] = dict(stats(reps, 1e6, "us"), repeats_us=[round(1e6 * t, 3) for t in reps])
    out["N%d" % N] = r
samplers = [("slice", {})] + ([("slice_device", {"sampler": "slice_device"})] if HAVE else [])
out["default_workload"] = {}
for name, over in samplers:
    default_regime.run(c, trials=20, **over)   # warm-up
    rates = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = default_regime.run(c, **over)
        rates.append(len(res["nominees"]) / (time.perf_counter() - t0))
    out["default_workload"][name] = {"trials_per_s_wall": [round(v, 1) for v in rates], "median": round(float(np.median(rates)), 1)}
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
