"""What constrained nomination costs: b7_eval_nominate_feasible (LogEI) with C = 0, 1, 2 constraint contexts against the plain
b7_eval_nominate on the same inputs, at the default-regime shape (N = 100, d = 6, 2e4 candidates, S = 10) and the headline shape
(N = 2048, d = 32, 2^20 candidates, S = 1).  A constraint is one LogPI b7_eval_nominate on a context of its own (same data sizes,
another response, same grid) plus b7_feas_add_acc; a constrained call is timed WITH its constraints' nominations, b7_feas_reset
and the adds.  Per shape: wall time per call (median and min .. max over the rounds, after warm-up), and the extra milliseconds
per constraint.  --parent TREE: the same plain nomination timed in a child process on another built checkout of the project (the
parent commit's), in the same visit.  Prints one JSON object.
usage (GPU box): python tools/feas_cost.py [out.json] [--parent path/to/built/checkout]"""
import json
import os
import subprocess
import sys
import time

import numpy as np
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(TREE))
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


def problem(sh, rng):
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    Cs = [np.cos(2.0 * X[:, k:k + 3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1)) for k in range(2)]

    def hyps(R):
        amp = float(np.var(R))
        return [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(R.mean())} for s in range(S)]
    return X, Y, Cs, hyps


parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (parent, TREE)]
plain_only = "--plain-only" in sys.argv
out = {"score": "logei"}
c = bot7_amd.Context(0)
cons = [] if plain_only else [bot7_amd.Context(0), bot7_amd.Context(0)]
rng = np.random.default_rng(0)
for name, sh in SHAPES.items():
    X, Y, Cs, hyps = problem(sh, rng)
    hy, fmin = hyps(Y), [float(Y.min())]
    c.grid_sobol(sh["M"], sh["d"], 1, download=False)
    c.gp_set_data(X, Y)
    r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
    r["plain"] = timed(lambda: c.eval_nominate(hy, score="logei", fmin=fmin), sh["warm"], sh["rounds"])
    if not plain_only:
        hc = [hyps(Ck) for Ck in Cs]
        for k, cc in enumerate(cons):
            cc.grid_sobol(sh["M"], sh["d"], 1, download=False)
            cc.gp_set_data(X, Cs[k])

        def constrained(C):
            for k in range(C):
                cons[k].eval_nominate(hc[k], score="logpi", fmin=[0.5], tradeoff=0.0)
            c.feas_reset()
            for k in range(C):
                c.feas_add_acc(cons[k])
            return c.eval_nominate_feasible(hy, score="logei", fmin=fmin)
        for C in (0, 1, 2):
            r["feasible_C%d" % C] = timed(lambda: constrained(C), sh["warm"], sh["rounds"])
        r["C0_minus_plain_ms"] = round(r["feasible_C0"]["median_ms"] - r["plain"]["median_ms"], 4)
        r["per_constraint_ms"] = round((r["feasible_C2"]["median_ms"] - r["feasible_C0"]["median_ms"]) / 2.0, 4)
        r["per_constraint_over_plain"] = round(r["per_constraint_ms"] / r["plain"]["median_ms"], 3)
    out[name] = r
c.close()
for cc in cons:
    cc.close()
if parent and not plain_only:   # the parent's nomination, same inputs, a fresh process on the other checkout's package and library
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only", "--tree", parent], capture_output=True, text=True, check=True)
    theirs = json.loads(res.stdout.strip().splitlines()[-1])
    for name in SHAPES:
        out[name]["parent_plain"] = theirs[name]["plain"]
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
