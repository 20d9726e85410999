"""The kernels of the slab walk (ksx_kernel, believer_kernel) and kg_kernel under this build against a checkout of the parent commit
with its library built, in child processes of ONE run, alternating parent / this, ROUNDS rounds each.  Per round and build:
  headline  (N = 2048, d = 32, 2^20 candidates, S = 1): the GPU time of the phases `ksx` (b7_eval_nominate), `believer`
            (b7_eval_nominate_batch, q = 8) and `kg` (b7_kg_nominate, 16 points), each the median of three profiled calls after a
            warm-up, and bench.py's ms/step (--steps 5 --warmup 2, no CPU baseline, no extras)
  wide      (N = 2048, d = 64, 2^18 candidates, S = 1): the phase `kg` again, in a 32-row slab class (dpad >= 48)
  default   (N = 100, d = 6, 2e4 candidates, S = 10): wall time per call of the batch (q = 8) and KG nominations, the median of 30
            calls after 5
  first     wall time of a fresh context's first nomination (default shape), library load excluded
A figure passes when this build's median over the rounds is no higher than the parent's median plus the parent's own min-to-max
spread over its rounds -- the only noise estimate the run itself provides.  Writes both builds' medians and spreads.
usage (GPU box): python tools/cov_walk_ab.py --parent-tree DIR [--this-tree DIR] [out.json]      (exit status 1 when a figure is
outside its margin; --this-tree with the parent's tree again shows what running second costs: nothing, 24.280 -> 24.281 ms)"""
import json
import os
import subprocess
import sys
import time

import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("B7_COST_TREE") or HERE   # (the child's tree)
sys.path.insert(0, ROOT)

ROUNDS = 5
HEAD = dict(N=2048, d=32, M=1 << 20, S=1)
WIDE = dict(N=2048, d=64, M=1 << 18, S=1)
DEFAULT = dict(N=100, d=6, M=20000, S=10)
Q, POINTS = 8, 16


def inputs(sh, rng):
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    return X, Y, hyps, [float(Y.min())]


def wall_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def child():
    import bot7_amd
    rng = np.random.default_rng(0)
    out = {}
    c = bot7_amd.Context(0)
    X, Y, hyps, fmin = inputs(DEFAULT, rng)
    c.grid_sobol(DEFAULT["M"], DEFAULT["d"], 1, download=False)
    c.gp_set_data(X, Y)
    t0 = time.perf_counter()
    c.eval_nominate(hyps, score="ei", fmin=fmin)
    out["first_nomination_ms"] = (time.perf_counter() - t0) * 1e3
    out["default_batch_call_ms"] = wall_ms(lambda: c.eval_nominate_batch(hyps, Q, score="ei", fmin=fmin), 5, 30)
    out["default_kg_call_ms"] = wall_ms(lambda: c.kg_nominate(hyps, points=POINTS), 5, 30)
    X, Y, hyps, fmin = inputs(HEAD, rng)
    c.grid_sobol(HEAD["M"], HEAD["d"], 1, download=False)
    c.gp_set_data(X, Y)
    calls = {"ksx": lambda: c.eval_nominate(hyps, score="ei", fmin=fmin),
             "believer": lambda: c.eval_nominate_batch(hyps, Q, score="ei", fmin=fmin),
             "kg": lambda: c.kg_nominate(hyps, points=POINTS)}
    for fn in calls.values():
        fn()
    c.profile_enable(True)
    for phase, fn in calls.items():
        ms = []
        for _ in range(3):
            c.profile_reset()
            fn()
            ms.append(c.profile_get(phase)[0])
        out["headline_%s_phase_ms" % phase] = float(np.median(ms))
    c.profile_enable(False)
    X, Y, hyps, fmin = inputs(WIDE, rng)
    c.grid_random(WIDE["M"], WIDE["d"], seed=0, download=False)   # (the Sobol grid ends at 39 dimensions)
    c.gp_set_data(X, Y)
    c.kg_nominate(hyps, points=POINTS)
    c.profile_enable(True)
    ms = []
    for _ in range(3):
        c.profile_reset()
        c.kg_nominate(hyps, points=POINTS)
        ms.append(c.profile_get("kg")[0])
    out["wide_kg_phase_ms"] = float(np.median(ms))
    c.profile_enable(False)
    c.close()
    print(json.dumps(out))


def run_child(tree):
    env = dict(os.environ)
    env["B7_COST_TREE"] = os.path.abspath(tree)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise RuntimeError("child (%s) failed with status %d: %s" % (tree, res.returncode, res.stderr[-2000:]))
    out = json.loads(res.stdout.strip().splitlines()[-1])
    res = subprocess.run([sys.executable, os.path.join(os.path.abspath(tree), "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                          "--no-cpu-baseline", "--no-extras"], cwd=os.path.abspath(tree), capture_output=True, text=True, timeout=300)
    if res.returncode != 0:
        raise RuntimeError("bench.py (%s) failed with status %d: %s" % (tree, res.returncode, res.stderr[-2000:]))
    out["bench_ms_per_step"] = json.loads(res.stdout.strip().splitlines()[-1])["ms_per_step"]
    return out


def main(argv):
    if "--child" in argv:
        return child()
    parent = argv[argv.index("--parent-tree") + 1]
    this = argv[argv.index("--this-tree") + 1] if "--this-tree" in argv else HERE   # (the parent's tree again: what the second place costs)
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--parent-tree", "--this-tree"))]
    runs = {"parent": [], "this": []}
    for r in range(ROUNDS):
        for which, tree in (("parent", parent), ("this", this)):
            runs[which].append(run_child(tree))
            print(which, r, json.dumps(runs[which][-1]), flush=True)
    out, bad = {"rounds": ROUNDS, "headline": HEAD, "wide": WIDE, "default": DEFAULT, "q": Q, "points": POINTS, "figures": {}}, []
    for key in runs["parent"][0]:
        p, t = [x[key] for x in runs["parent"]], [x[key] for x in runs["this"]]
        f = {"parent_median": round(float(np.median(p)), 4), "parent_spread": round(max(p) - min(p), 4),
             "this_median": round(float(np.median(t)), 4), "this_spread": round(max(t) - min(t), 4)}
        f["inside"] = f["this_median"] <= f["parent_median"] + f["parent_spread"]
        if not f["inside"] and key != "first_nomination_ms":   # the first launch is reported, not judged
            bad.append(key)
        out["figures"][key] = f
    out["outside_margin"] = bad
    print(json.dumps(out, indent=1))
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
