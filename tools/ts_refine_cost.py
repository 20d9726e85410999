"""What refining Thompson nominees on their sample paths costs, and what it buys.  One visit, one JSON object:

  (a) b7_ts_nominate_refine (16 starts, 16 iterations) against b7_ts_nominate on the same inputs, at the headline shape (N = 2048,
      d = 32, 2^20 candidates, F = 1024, S = 1; q = 1 and 16) and at the default regime's shape (N = 100, d = 6, 2e4 candidates,
      S = 10; q = 1 and 8): wall time per call (median, min .. max) and the GPU time of a profiled call by phase (ts_refine: the one
      launch that holds every iteration; ts_refine:pack, the operands into fragment order; ts_refine:starts, the start selection);
  (b) the refinement kernel against its own issue bound.  The fp64 MFMA and the fp64 VALU share the same units (gemm_f64.h), so
      a chunk of 16 features or 16 observations costs its MFMAs (dpad / 4 for the product + 4 ceil(dpad / 16) for the gradient
      tile, 64 cycles each) PLUS its vector instructions (4 cycles each at wave64).  One wave owns four starts for all iterations and
      nothing crosses waves, so the launch lasts as long as one wave's iters + 1 evaluations: (F + Npad16) / 16 chunks each.  The
      MFMA part of the bound is exact; VALU_PER_CHUNK is an ESTIMATE from the source (four sine / cosine pairs of ~45 instructions
      per feature chunk, four covariance-and-gradient entries of ~30 per observation chunk), not a count from the ISA;
  (c) b7_ts_nominate itself against the parent commit (--parent-tree DIR: a tree that holds a build of it), alternating, the same
      script: its path is meant to be untouched, so the two must sit inside each other's run-to-run spread;
  (d) quality, recorded and never asserted: the harness bot on ackley, d = 32, trust region + Thompson sampling, refined and
      unrefined, over the seeds tools/tr_cost.py uses.
usage (GPU box): python tools/ts_refine_cost.py out.json [--parent-tree DIR] [a] [c] [d]
                 python tools/ts_refine_cost.py --time-ts TREE        (part (c)'s child: TREE's own package times b7_ts_nominate)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 1024
SHAPES = {"headline": dict(N=2048, d=32, M=1 << 20, S=1, qs=(1, 16), warm=2, rounds=7),
          "default": dict(N=100, d=6, M=20000, S=10, qs=(1, 8), warm=5, rounds=30)}
STARTS, ITERS = 16, 16
VALU_PER_CHUNK = {"features": 4 * 45, "observations": 4 * 30}     # estimates, see (b)
CLOCK_HZ = 2.4e9


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


def stage(c, sh, rng):
    N, d, M, S = sh["N"], sh["d"], sh["M"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    c.grid_sobol(M, d, 1, download=False)
    c.gp_set_data(X, Y)
    return hyps


def time_ts(tree):
    """b7_ts_nominate alone at both shapes, by the package of `tree`."""
    sys.path.insert(0, tree)
    import bot7_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(bot7_amd.__file__))) == os.path.abspath(tree)
    c = bot7_amd.Context(0)
    rng = np.random.default_rng(0)
    out = {}
    for name, sh in SHAPES.items():
        hyps = stage(c, sh, rng)
        out[name] = {"q%d" % q: timed(lambda: c.ts_nominate(hyps, q, n_features=F, seed=1), sh["warm"], sh["rounds"]) for q in sh["qs"]}
    c.close()
    print(json.dumps(out))


def issue_bound_ms(N, d, iters):
    dpad = 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64 if d <= 64 else 96
    mfmas = dpad // 4 + 4 * ((dpad + 15) // 16)
    fch, och = F // 16, (N + 15) // 16
    mf = (fch + och) * mfmas * 64
    va = (fch * VALU_PER_CHUNK["features"] + och * VALU_PER_CHUNK["observations"]) * 4
    return {"mfmas_per_chunk": mfmas, "chunks_per_evaluation": fch + och, "evaluations": iters + 1,
            "mfma_bound_ms": round((iters + 1) * mf / CLOCK_HZ * 1e3, 4),
            "mfma_plus_estimated_valu_ms": round((iters + 1) * (mf + va) / CLOCK_HZ * 1e3, 4)}


def part_a(c):
    rng = np.random.default_rng(0)
    out = {"features": F, "starts": STARTS, "iters": ITERS}
    for name, sh in SHAPES.items():
        hyps = stage(c, sh, rng)
        r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
        for q in sh["qs"]:
            e = {"ts_nominate": timed(lambda: c.ts_nominate(hyps, q, n_features=F, seed=1), sh["warm"], sh["rounds"]),
                 "ts_nominate_refine": timed(lambda: c.ts_nominate_refine(hyps, q, n_features=F, seed=1, starts=STARTS, iters=ITERS),
                                             sh["warm"], sh["rounds"])}
            e["refine_over_plain"] = round(e["ts_nominate_refine"]["median_ms"] / e["ts_nominate"]["median_ms"], 3)
            c.profile_enable(True)
            split = {k: [] for k in ("ts_refine", "ts_refine:pack", "ts_refine:starts")}
            for _ in range(5):
                c.profile_reset()
                pm, idx, x, val, start = c.ts_nominate_refine(hyps, q, n_features=F, seed=1, starts=STARTS, iters=ITERS)
                for k in split:
                    split[k].append(c.profile_get(k)[0])
            c.profile_enable(False)
            e["split_gpu_ms"] = {k: round(float(np.median(v)), 4) for k, v in split.items()}
            e["path_value_gain"] = [round(float(v), 6) for v in (pm - val)]       # f_j at the grid nominee minus f_j at the refined point
            b = issue_bound_ms(sh["N"], sh["d"], ITERS)
            b["fraction_of_mfma_bound"] = round(b["mfma_bound_ms"] / e["split_gpu_ms"]["ts_refine"], 3) if e["split_gpu_ms"]["ts_refine"] > 0 else None
            e["refine_kernel"] = b
            r["q%d" % q] = e
        out[name] = r
    return out


def part_c(parent_tree):
    runs = {"this": [], "parent": []}
    for _ in range(3):
        for label, tree in (("parent", parent_tree), ("this", ROOT)):
            got = subprocess.run([sys.executable, os.path.abspath(__file__), "--time-ts", tree], capture_output=True, text=True, check=True)
            runs[label].append(json.loads(got.stdout.strip().splitlines()[-1]))
    out = {"what": "b7_ts_nominate, three alternating processes per tree; per process the median of its rounds"}
    for name, sh in SHAPES.items():
        for q in sh["qs"]:
            key = "q%d" % q
            a = [r[name][key]["median_ms"] for r in runs["this"]]
            b = [r[name][key]["median_ms"] for r in runs["parent"]]
            out["%s_%s" % (name, key)] = {"this_ms": a, "parent_ms": b, "this_over_parent": round(float(np.median(a) / np.median(b)), 4),
                                          "inside_parent_spread": bool(min(b) <= np.median(a) <= max(b))}
    return out


class _H(object):
    def __init__(self, name):
        self.name, self.min, self.max, self.size = name, 0.0, 1.0, 1


def part_d(c):
    import bot7_amd
    from harness import benchmarks, bots
    d, M, budget, n_initial = 32, 20000, 200, 64
    out = {"objective": "ackley", "d": d, "candidates": M, "budget": budget, "nInitial": n_initial, "nSamples": 1, "seeds": [1, 2, 3, 4, 5],
           "model": "gp_regressor, sample = False (lenscale_sq = d / 8)", "refine": {"starts": STARTS, "iters": ITERS}}
    for label, refine in (("trust_region_thompson", None), ("trust_region_thompson_refined", {"starts": STARTS, "iters": ITERS})):
        best, secs = [], []
        for seed in out["seeds"]:
            score = {"type": "thompson_sampling", "nFeatures": 1024}
            if refine:
                score["refine"] = dict(refine)
            cfg = {"bot": {"verbose": 0, "budget": budget, "nInitial": n_initial, "nSamples": 1, "seed": seed, "batch": 1, "trust_region": {}},
                   "grid": {"type": "sobol", "size": M, "dims": d}, "score": score}
            bot = bots.bayesopt(benchmarks.ackley, [_H("x%d" % k) for k in range(d)], cfg,
                                cache={"model": bot7_amd.models.gp_regressor({}, context=c)})
            t0 = time.perf_counter()
            for _ in range(budget):
                x, y = bot.run_trial()
                bot.update_best(x, y)
            secs.append(round(time.perf_counter() - t0, 2))
            best.append(round(float(bot.responses.min()), 5))
            del bot
        out[label] = {"best": best, "median_best": round(float(np.median(best)), 5), "seconds": secs}
    return out


if __name__ == "__main__":
    if sys.argv[1] == "--time-ts":
        time_ts(sys.argv[2])
        sys.exit(0)
    sys.path.insert(0, ROOT)
    import bot7_amd
    path, args = sys.argv[1], sys.argv[2:]
    parent = args[args.index("--parent-tree") + 1] if "--parent-tree" in args else None
    parts = [p for p in args if p in ("a", "c", "d")] or ["a", "c", "d"]
    out = json.load(open(path)) if os.path.exists(path) else {}
    if "c" in parts and parent:           # before this process opens the GPU: the children time alone
        out["ts_nominate_against_parent"] = part_c(parent)
        print("ts_nominate_against_parent", json.dumps(out["ts_nominate_against_parent"]))
    c = bot7_amd.Context(0)
    out["device"] = c.device_info()["name"]
    for p, fn, key in (("a", part_a, "cost"), ("d", part_d, "quality")):
        if p in parts:
            out[key] = fn(c)
            print(key, json.dumps(out[key]))
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    c.close()
