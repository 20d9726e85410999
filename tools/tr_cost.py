"""What trust-region nomination costs and what it buys.  Three parts, each written into one JSON object:
  (a) b7_grid_trust_region alone at 2e4 x 6 and 2^20 x 32: GPU time of the call's phase (HIP events around the launch; warm-up,
      then the median over the rounds) against its traffic bound, one read and one write of M d doubles at the 6.29 TB/s a
      device-to-device copy reaches on this part; and the wall time of the whole synchronous call.
  (b) a whole model-based trial of the harness bot with config.bot.trust_region against the same script with trust_region = None
      (the fixed grid, thinned by a row per trial), both shapes, EI and Thompson sampling: wall time per trial, median over the
      model-based trials after the first.
  (c) optimisation quality, recorded and never asserted: ackley in 32 dimensions, 2e4 candidates, budget 200, nInitial 64, five
      seeds; the best value after the budget for trust region + Thompson sampling, trust region + EI and fixed-grid EI.  The model
      is the harness default (config.model.sample = False: the point initialisation of gp_regressor.init, lenscale_sq = d / 8), so
      the box is a cube; nSamples = 1.
  (d) on request only: (c) again with slice-sampled hypers (config.model.sample = True, nSamples = 4), where the lengthscales
      differ by column and the box is no cube.
usage (GPU box): python tools/tr_cost.py out.json [a] [b] [c] [d]      (no letters: a b c; an existing out.json is extended)"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402
from harness import benchmarks, bots  # noqa: E402

COPY_BYTES_PER_S = 6.29e12
SHAPES = {"default": dict(M=20000, d=6, warm=5, rounds=30), "headline": dict(M=1 << 20, d=32, warm=3, rounds=15)}


class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def med(ts):
    ts = np.asarray(ts, dtype=np.float64)
    return {"median_ms": round(float(np.median(ts)), 5), "min_ms": round(float(ts.min()), 5), "max_ms": round(float(ts.max()), 5), "n": int(ts.size)}


def part_a(c):
    out = {}
    for name, sh in SHAPES.items():
        M, d = sh["M"], sh["d"]
        rng = np.random.default_rng(d)
        lo = rng.uniform(0.0, 0.4, d)
        hi = lo + rng.uniform(0.1, 0.5, d)
        center, shift = 0.5 * (lo + hi), rng.random(d)
        r = {"shape": {"M": M, "d": d}, "bytes": 2 * M * d * 8, "bound_ms": round(2 * M * d * 8 / COPY_BYTES_PER_S * 1e3, 5)}
        for label, sft in (("rotated", shift), ("plain", None)):
            c.grid_random(M, d, 1, download=False)
            gpu, wall = [], []
            c.profile_enable(True)
            for k in range(sh["warm"] + sh["rounds"]):
                c.profile_reset()
                t0 = time.perf_counter()
                c.grid_trust_region(center, lo, hi, min(1.0, 20.0 / d), shift=sft, seed=k)
                wall.append((time.perf_counter() - t0) * 1e3)
                gpu.append(c.profile_get("trust_region")[0])
            c.profile_enable(False)
            e = {"gpu": med(gpu[sh["warm"]:]), "wall_profiled": med(wall[sh["warm"]:])}
            e["fraction_of_bound"] = round(r["bound_ms"] / e["gpu"]["median_ms"], 4) if e["gpu"]["median_ms"] > 0 else None
            wall = []
            for k in range(sh["warm"] + sh["rounds"]):
                t0 = time.perf_counter()
                c.grid_trust_region(center, lo, hi, min(1.0, 20.0 / d), shift=sft, seed=k)
                wall.append((time.perf_counter() - t0) * 1e3)
            e["wall"] = med(wall[sh["warm"]:])
            r[label] = e
        out[name] = r
    return out


def make_bot(c, d, M, score, tr, seed, budget, n_initial, n_samples, batch=1, model=None):
    cfg = {"bot": {"verbose": 0, "budget": budget, "nInitial": n_initial, "nSamples": n_samples, "seed": seed, "batch": batch, "trust_region": tr},
           "grid": {"type": "sobol", "size": M, "dims": d},
           "score": dict({"type": score}, **({"nFeatures": 1024} if score == "thompson_sampling" else {}))}
    cache = {"model": bot7_amd.models.gp_regressor(dict(model or {}), context=c)}
    if tr is None:
        cache["candidates"] = bot7_amd.grids.sobol({"size": M, "dims": d, "mins": np.zeros(d), "maxes": np.ones(d)}, context=c)()
    return bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(d)], cfg, cache=cache)


def part_b(c):
    out = {}
    for name, sh in SHAPES.items():
        M, d = sh["M"], sh["d"]
        n_initial, trials = 16, (12 if name == "default" else 6)
        r = {"shape": {"M": M, "d": d, "nInitial": n_initial, "nSamples": 2, "model_trials": trials}}
        for score in ("expected_improvement", "thompson_sampling"):
            e = {}
            for label, tr in (("trust_region", {}), ("fixed_grid", None)):
                bot = make_bot(c, d, M, score, tr, 3, n_initial + trials, n_initial, 2)
                ts = []
                for t in range(n_initial + trials):
                    t0 = time.perf_counter()
                    bot.run_trial()
                    ts.append((time.perf_counter() - t0) * 1e3)
                e[label] = med(ts[n_initial + 1:])
                e[label]["initial_trial"] = med(ts[1:n_initial])
                del bot
            e["trust_region_over_fixed_grid"] = round(e["trust_region"]["median_ms"] / e["fixed_grid"]["median_ms"], 3)
            r[score] = e
        out[name] = r
    return out


def part_c(c, model=None, n_samples=1):
    d, M, budget, n_initial = 32, 20000, 200, 64
    out = {"objective": "ackley", "d": d, "candidates": M, "budget": budget, "nInitial": n_initial, "nSamples": n_samples, "seeds": [1, 2, 3, 4, 5],
           "model": "gp_regressor, sample = False (lenscale_sq = d / 8)" if model is None else "gp_regressor, %r" % (model,)}
    arms = {"trust_region_thompson": ("thompson_sampling", {}), "trust_region_ei": ("expected_improvement", {}),
            "fixed_grid_ei": ("expected_improvement", None)}
    for label, (score, tr) in arms.items():
        best, restarts, secs = [], [], []
        for seed in out["seeds"]:
            bot = make_bot(c, d, M, score, tr, seed, budget, n_initial, n_samples, model=model)
            t0 = time.perf_counter()
            bot.run_experiment()
            secs.append(round(time.perf_counter() - t0, 2))
            best.append(round(float(bot.responses.min()), 5))
            restarts.append(int(bot.tr_state.restarts) if bot.tr_state is not None else 0)
            del bot
        out[label] = {"best": best, "median_best": round(float(np.median(best)), 5), "restarts": restarts, "seconds": secs}
    return out


if __name__ == "__main__":
    path = sys.argv[1]
    parts = [p for p in sys.argv[2:] if p in ("a", "b", "c", "d")] or ["a", "b", "c"]
    out = json.load(open(path)) if os.path.exists(path) else {}
    c = bot7_amd.Context(0)
    out["device"] = c.device_info()["name"]

    def part_d(ctx):   # (c) again with slice-sampled hypers, four per trial: the box takes its shape from the lengthscales
        return part_c(ctx, model={"sample": True}, n_samples=4)

    for p, fn, key in (("a", part_a, "map_alone"), ("b", part_b, "trial"), ("c", part_c, "quality"), ("d", part_d, "quality_sampled_hypers")):
        if p in parts:
            out[key] = fn(c)
            with open(path, "w") as f:
                json.dump(out, f, indent=1)
            print(key, json.dumps(out[key]))
    c.close()
