"""What max-value entropy search costs: a B7_SCORE_MES nomination against the EI nomination on the same inputs (the EI / CB / LogEI
kernels and their host path are instruction for instruction the parent commit's, so the EI figure is the parent's), at the
default-regime shape (N = 100, d = 6, 2e4 candidates, S = 10) and the headline shape (N = 2048, d = 32, 2^20 candidates, S = 1),
K = 8 levels.  Per shape: wall time per b7_eval_nominate call (median and min .. max over the rounds, after warm-up), the extra
milliseconds, the y* search's GPU time from the "mes" phase events of a profiled call (eleven launches per search: the bracket,
ten rounds) and its share of the extra cost, and the launches the search adds per nomination.  Prints one JSON object.
usage (GPU box): python tools/mes_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, warm=5, rounds=30),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=2, rounds=5)}


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4)}


def timed(fn, warm, rounds):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats(ts)


out = {"levels": 8}
c = bot7_amd.Context(0)
rng = np.random.default_rng(0)
for name, sh in SHAPES.items():
    N, d, M, S = sh["N"], sh["d"], sh["M"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    fmin = [float(Y.min())]
    c.grid_sobol(M, d, 1, download=False)
    c.gp_set_data(X, Y)
    r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
    r["ei"] = timed(lambda: c.eval_nominate(hyps, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    r["mes"] = timed(lambda: c.eval_nominate(hyps, score="mes", levels=8), sh["warm"], sh["rounds"])
    r["extra_ms"] = round(r["mes"]["median_ms"] - r["ei"]["median_ms"], 4)
    c.profile_enable(True)
    search = []
    for _ in range(5):   # the search's own GPU time: events around each of its launches (profiling serialises the phases)
        c.profile_reset()
        c.eval_nominate(hyps, score="mes", levels=8)
        ms, launches = c.profile_get("mes")
        search.append(ms)
    c.profile_enable(False)
    r["search_gpu_ms"] = round(float(np.median(search)), 4)
    r["search_launches_per_nomination"] = int(launches)
    r["search_share_of_extra"] = round(r["search_gpu_ms"] / r["extra_ms"], 3) if r["extra_ms"] > 0 else None
    r["mes_over_ei"] = round(r["mes"]["median_ms"] / r["ei"]["median_ms"], 2)
    out[name] = r
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
