"""What the off-grid refinement costs: b7_eval_nominate_refine (16 starts, 16 iterations) beside the b7_eval_nominate it follows,
on the same inputs, timed in the same run, at the headline shape (N = 2048, d = 32, 2^20 candidates, S = 1) and the default
regime's shape (N = 100, d = 6, 2e4 candidates, S = 10), for EI and LogEI.  Per shape and score: wall time per call (median and
min .. max over the rounds, after warm-up) of both entry points and their difference = the refinement; the GPU time of a profiled
call split by phase events into
  starts   the 15 arg-max pairs over the accumulator and the state's first fill (refine:starts),
  k        k and g of the 64 query columns (refine:k),
  v        V = inv(L) k* (refine:v),
  w        W = inv(L)' V and the contractions over the observations (refine:w),
  gather   the block partials summed (refine:gather),
  step     score value / gradient, marginal, ladder (refine:step)
(profiling serialises the phases, so the split adds up to more than an unprofiled call), the same per iteration (17 launch sets:
iteration 0 and the 16 steps); the bytes of L^-1 an iteration reads (2 products x 8 Npad^2 / 2 per sample) against the rate the v
and w phases reached; and the gain in score over the grid's best on these runs.  Prints one JSON object.
usage (GPU box): python tools/refine_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

STARTS, ITERS = 16, 16
SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, warm=5, rounds=30),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=2, rounds=5)}
PHASES = {"starts": "refine:starts", "k": "refine:k", "v": "refine:v", "w": "refine:w", "gather": "refine:gather", "step": "refine:step"}


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


out = {"starts": STARTS, "iters": ITERS}
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
    npad = 64 if N <= 64 else (N + 127) // 128 * 128
    r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}, "npad": npad}
    for score in ("ei", "logei"):
        e = {"nominate": timed(lambda: c.eval_nominate(hyps, score=score, fmin=fmin), sh["warm"], sh["rounds"]),
             "nominate_refine": timed(lambda: c.eval_nominate_refine(hyps, score=score, fmin=fmin, starts=STARTS, iters=ITERS),
                                      sh["warm"], sh["rounds"])}
        e["refinement_ms"] = round(e["nominate_refine"]["median_ms"] - e["nominate"]["median_ms"], 4)
        e["refinement_over_nominate"] = round(e["refinement_ms"] / e["nominate"]["median_ms"], 4)
        e["refinement_per_iteration_ms"] = round(e["refinement_ms"] / (ITERS + 1), 4)
        c.profile_enable(True)
        split = {k: [] for k in PHASES}
        for _ in range(5):
            c.profile_reset()
            c.eval_nominate_refine(hyps, score=score, fmin=fmin, starts=STARTS, iters=ITERS)
            for k, ph in PHASES.items():
                split[k].append(c.profile_get(ph)[0])
        c.profile_enable(False)
        e["split_gpu_ms"] = {k: round(float(np.median(v)), 4) for k, v in split.items()}
        e["split_gpu_ms_per_iteration"] = {k: round(float(np.median(v)) / (ITERS + 1), 5) for k, v in split.items() if k != "starts"}
        linv_bytes = 2 * 8 * npad * npad // 2 * S
        vw_ms = (e["split_gpu_ms"]["v"] + e["split_gpu_ms"]["w"]) / (ITERS + 1)
        e["linv_bytes_per_iteration"] = linv_bytes
        e["linv_rate_gb_s"] = round(linv_bytes / (vw_ms * 1e-3) / 1e9, 2) if vw_ms > 0 else None
        v, i, x, rv, ri = c.eval_nominate_refine(hyps, score=score, fmin=fmin, starts=STARTS, iters=ITERS)
        last = c.refine_last()
        e["grid_best"], e["refined"], e["gain"] = v, rv, rv - v
        e["winner_is_nominee"] = bool(ri == i)
        e["starts_moved"] = int(np.sum((last["status"] & 8) != 0))
        r[score] = e
    out[name] = r
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
