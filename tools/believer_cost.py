"""What a batch member costs: b7_eval_nominate_batch (kriging-believer downdates) against b7_eval_nominate and against the
refit-and-renominate an extra pick replaces, at the headline shape (N = 2048, d = 32, 2^20 Sobol candidates, S = 1, EI) and the
default-regime shape (N = 100, d = 6, 2e4 candidates, S = 10).  Per shape: wall time per call of b7_eval_nominate and of the
batch at q = 1, 4, 8 (median and min .. max over the rounds, after warm-up), the per-extra-pick time (q = 8 minus q = 1, over 7)
and the alternative: one more b7_eval_nominate on N + 1 observations (data upload and refit included), same card, same session.
Prints one JSON object.
usage (GPU box): python tools/believer_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

SHAPES = {"headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=2, rounds=5),
          "default": dict(N=100, d=6, M=20000, S=10, warm=5, rounds=30)}


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


out = {}
c = bot7_amd.Context(0)
rng = np.random.default_rng(0)
for name, sh in SHAPES.items():
    N, d, M, S = sh["N"], sh["d"], sh["M"], sh["S"]
    X = rng.random((N + 1, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N + 1, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    fmin = [float(Y.min())]
    c.grid_sobol(M, d, 1, download=False)
    c.gp_set_data(X[:N], Y[:N])
    r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
    r["eval_nominate"] = timed(lambda: c.eval_nominate(hyps, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    for q in (1, 4, 8):
        r["batch_q%d" % q] = timed(lambda: c.eval_nominate_batch(hyps, q, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    r["per_extra_pick_ms"] = round((r["batch_q8"]["median_ms"] - r["batch_q1"]["median_ms"]) / 7.0, 4)
    r["per_extra_pick_over_first"] = round(r["per_extra_pick_ms"] / r["batch_q1"]["median_ms"], 4)

    def refit():   # what an extra pick replaces: the believed point joins the data, everything is refitted and re-scored
        c.gp_set_data(X, Y)
        c.eval_nominate(hyps, score="ei", fmin=fmin)
    r["refit_and_renominate"] = timed(refit, sh["warm"], sh["rounds"])
    out[name] = r
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
