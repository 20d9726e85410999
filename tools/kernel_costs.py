"""What the covariance kernel costs: ARD-SE against ARD Matern-5/2 (b7_gp_set_kernel) on the same inputs -- K(X*,X) assembly
rate at d = 6, 32, 64 (N = 2048, 262144 candidates, the ksx phase of b7_gp_predict), per-call latency of one small-set
likelihood (b7_gp_nll_batch, B = 1) and of one small nomination (b7_eval_nominate, S = 10, 2e4 candidates, d = 6) at N = 25
and 100, and trials/s of the default-regime loop (harness/default_regime.py, 30 trials).  Prints one JSON object.
usage (GPU box): python tools/kernel_costs.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402
from harness import default_regime as dr  # noqa: E402

KERNELS = ("ardse", "ardmatern52")
out = {"ksx": {}, "nll_us": {}, "nominate_us": {}, "default_loop": {}}
c = bot7_amd.Context(0)
N, M = 2048, 262144
for d in (6, 32, 64):
    X = c.grid_random(N, d, seed=3, row_offset=10 * M)
    Y = np.sin(X.sum(1, keepdims=True))
    c.grid_random(M, d, seed=3, download=False)
    for k in KERNELS:
        c.gp_set_kernel(k)
        c.gp_fit(X, Y, np.full(d, d / 8.0), 1.0, 1e-4, 0.0)
        c.gp_predict(download=False)
        c.profile_enable(True)
        ts = []
        for _ in range(7):
            c.profile_reset()
            c.gp_predict(download=False)
            c.sync()
            ts.append(c.profile_get("ksx")[0])
        c.profile_enable(False)
        ms = float(np.median(ts))
        out["ksx"]["%s d%d" % (k, d)] = {"ms": round(ms, 4), "GB_per_s": round(M * 8.0 * N / (ms * 1e-3) / 1e9, 1)}
rng = np.random.default_rng(0)
c.grid_sobol(20000, 6, 1, download=False)
for n in (25, 100):
    X = rng.random((n, 6))
    Y = np.sin(3 * X.sum(1, keepdims=True))
    hyps = [{"lenscale_sq": np.full(6, 0.75 * (1 + 0.05 * s)), "amp": 1.0, "noise": 1e-4, "mean": 0.0} for s in range(10)]
    for k in KERNELS:
        c.gp_set_kernel(k)
        c.gp_set_data(X, Y)
        for _ in range(50):
            c.gp_nll1(np.full(6, 0.75), 1.0, 1e-4, 0.0)
        t0 = time.perf_counter()
        for i in range(500):
            c.gp_nll1(np.full(6, 0.75 + 1e-4 * i), 1.0, 1e-4, 0.0)
        out["nll_us"]["%s N%d" % (k, n)] = round((time.perf_counter() - t0) / 500 * 1e6, 2)
        for _ in range(5):
            c.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
        t0 = time.perf_counter()
        for _ in range(50):
            c.eval_nominate(hyps, score="ei", fmin=[float(Y.min())])
        out["nominate_us"]["%s N%d" % (k, n)] = round((time.perf_counter() - t0) / 50 * 1e6, 1)
c.close()
for k in KERNELS:
    ctx = bot7_amd.Context(0)
    t0 = time.perf_counter()
    r = dr.run(ctx, trials=30, kernel=k)
    wall = time.perf_counter() - t0
    ctx.close()
    out["default_loop"][k] = {"trials": 30, "trials_per_s": round(30 / wall, 2), "nll_calls": int(sum(t["nll_calls"] for t in r["per_trial"]))}
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
