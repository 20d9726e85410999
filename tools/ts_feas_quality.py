"""The quality run of constrained Thompson sampling, recorded and not asserted: gardner1 (harness/benchmarks.py; c <= 0.5), 2000 Sobol
candidates, a budget of 60 evaluations, five seeds.  config.score.type = 'constrained_thompson_sampling' at batch 4 (15 trials, the
first of them random) against constrained LogEI at batch 1 (60 trials, the first four random), nSamples 4, the slice sampler.  Per
seed and policy: the best feasible value after 20, 40 and 60 evaluations (null: no feasible row yet), the number of feasible rows and
the wall time.  Prints one JSON object.
usage (GPU box): python tools/ts_feas_quality.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402
from harness import benchmarks as B, bots  # noqa: E402

BUDGET, SEEDS, GRID = 60, (1, 2, 3, 4, 5), 2000
POLICIES = {"constrained_thompson_sampling_batch4": dict(kind="constrained_thompson_sampling", batch=4, nInitial=1),
            "constrained_logei_batch1": dict(kind="log_expected_improvement", batch=1, nInitial=4)}


class H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def run(policy, seed):
    ctx = bot7_amd.Context(0)
    mcfg = {"type": "gp_regressor", "sample": True, "sampler": "slice", "nBurnin": 2, "seed": 10 * seed}
    cfg = {"bot": {"verbose": 0, "budget": BUDGET // policy["batch"], "nInitial": policy["nInitial"], "nSamples": 4, "seed": seed,
                   "batch": policy["batch"], "constraints": [{"threshold": B.GARDNER1_THRESHOLD, "model": dict(mcfg, seed=10 * seed + 1)}]},
           "grid": {"type": "sobol", "size": GRID, "dims": 2}, "score": {"type": policy["kind"], "nFeatures": 256}, "model": mcfg}
    grid = bot7_amd.grids.sobol({"size": GRID, "dims": 2, "mins": np.zeros(2), "maxes": np.ones(2)}, context=ctx)()
    model = bot7_amd.models.gp_regressor(dict(mcfg), context=ctx)
    bot = bots.bayesopt(B.gardner1, [H("x1"), H("x2")], cfg, cache={"candidates": grid, "model": model})
    t0 = time.perf_counter()
    try:
        for _ in range(BUDGET // policy["batch"]):
            x, y = bot.run_trial()
            bot.update_best(x, y)
    finally:
        for con in bot.constraints or []:
            con["ctx"].close()
        ctx.close()
    R = bot.responses
    ok = R[:, 1] <= B.GARDNER1_THRESHOLD
    best = lambda n: float(R[:n][ok[:n], 0].min()) if ok[:n].any() else None
    return {"seed": seed, "best_feasible_after": {str(n): best(n) for n in (20, 40, 60)}, "feasible_rows": int(ok.sum()),
            "wall_s": round(time.perf_counter() - t0, 2)}


def main():
    res = {"benchmark": "gardner1", "threshold": B.GARDNER1_THRESHOLD, "budget": BUDGET, "grid": GRID, "policies": {}}
    for name, policy in POLICIES.items():
        runs = [run(policy, seed) for seed in SEEDS]
        finals = [r["best_feasible_after"]["60"] for r in runs]
        vals = [v for v in finals if v is not None]
        res["policies"][name] = {"runs": runs, "final_median": float(np.median(vals)) if vals else None,
                                 "final_mean": float(np.mean(vals)) if vals else None, "final_worst": max(vals) if vals else None}
        print(name, res["policies"][name]["final_median"], finals, file=sys.stderr, flush=True)
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
