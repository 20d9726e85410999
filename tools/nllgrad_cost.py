"""What the likelihood gradient and the bounded fit cost, measured on the GPU box.  Recorded, not gated.

  fit       b7_gp_fit_hyp_grad beside b7_gp_fit_hyp at the default regime's shape (N = 100, d = 6) and the headline's (N = 2048,
            d = 32): wall time per call around the call's own synchronisation, median of 200 after 20 warm-ups, both in one process
  kernel    the two gradient launches alone (phase events around them, profiling on) against the MFMA issue bound of what the
            algorithm needs: 2 N^3 / 3 flops of the triangular product plus 2 N^2 dpad / 2 of the epilogue's distance products,
            at the fp64 matrix peak of 78.6 TFLOP/s (csrc/gemm_f64.h), as a fraction
  map       a whole b7_gp_fit_map at both shapes from init's heuristic inside the model's bounds: wall time, iterations, evaluations
  parent    b7_gp_fit_hyp, b7_gp_nll_batch (B = 16) and b7_eval_nominate of this tree's library and of the parent commit's, each
            in processes of its own, alternating; the ratio of the medians beside the parent's own process-to-process spread.
            The parent's library is built beforehand, where there is a git history, by `--build-parent REV` (git archive of the
            named revision into tools/_build/parent, its own build.py; the hash goes into the JSON); without it the section says
            "not measured"
  quality   hartmann6, the default workload's grid and budget, five seeds: median best with the heuristic point estimate, with
            fit = 'map' and with ten slice samples, and trials per second of each.  Recorded, not asserted.
usage:  python tools/nllgrad_cost.py --build-parent REV        (where the history is; no GPU; REV: the commit this change sits on)
        python tools/nllgrad_cost.py [out.json] [--no-quality]  (GPU box)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("NLLGRAD_COST_TREE") or ROOT)   # a child measuring the parent commit imports the parent's package
PARENT = os.path.join(ROOT, "tools", "_build", "parent")
PARENT_SO = os.path.join(PARENT, "bot7_amd", "libbot7hip.so")
PARENT_REV = os.path.join(PARENT, "PARENT_REV")
SHAPES = {"default": dict(N=100, d=6, M=20000), "headline": dict(N=2048, d=32, M=1 << 18)}
PEAK = 78.6e12


def problem(N, d, seed=1):
    rng = np.random.default_rng([seed, N, d])
    X = rng.random((N, d))
    y = np.sin(3.0 * X.sum(axis=1) / np.sqrt(d)) + 0.1 * rng.standard_normal(N)
    amp = float(np.var(y))
    return X, y, (np.full(d, d / 8.0), amp, 1e-4 * amp, float(np.mean(y)))


def med(fn, warm, n):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 5), "min_ms": round(float(ts.min()), 5), "p90_ms": round(float(np.percentile(ts, 90)), 5)}


def child():
    """One process's medians of the three calls this change must not slow down (the package and library are NLLGRAD_COST_TREE's, or
    this tree's)."""
    import bot7_amd
    out = {}
    c = bot7_amd.Context(0)
    for name, s in SHAPES.items():
        X, y, h = problem(s["N"], s["d"])
        c.gp_set_data(X, y)
        c.grid_sobol(s["M"], s["d"], 1, download=False)
        hyps = [dict(lenscale_sq=h[0], amp=h[1], noise=h[2], mean=h[3])]
        n = 200 if s["N"] <= 128 else 40
        out[name] = {"gp_fit_hyp": med(lambda: c.gp_fit_hyp(*h), 20, n),
                     "gp_nll_batch16": med(lambda: c.gp_nll_batch(np.tile(h[0], (16, 1)), np.full(16, h[1]), np.full(16, h[2]), np.full(16, h[3])), 5, n // 2),
                     "eval_nominate": med(lambda: c.eval_nominate(hyps, score="ei", fmin=[float(y.min())]), 5, n // 2)}
    c.close()
    print(json.dumps(out))


def build_parent(rev):
    """The library of revision `rev` (the commit this change sits on: name it, HEAD is not it once the change is committed) under
    tools/_build/parent, built by its own build.py; the revision's hash is kept beside it and recorded with the measurements."""
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--verify", rev + "^{commit}"], check=True, capture_output=True, text=True).stdout.strip()
    os.makedirs(PARENT, exist_ok=True)
    tar = subprocess.run(["git", "-C", ROOT, "archive", sha], check=True, capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", PARENT], input=tar, check=True)
    subprocess.check_call([sys.executable, "-m", "bot7_amd.build"], cwd=PARENT)
    open(PARENT_REV, "w").write(sha + "\n")
    print("built", PARENT_SO, "of", sha)


def main():
    import bot7_amd
    from bot7_amd import _lib
    res = {"device": None, "fit": {}, "kernel": {}, "map": {}}
    c = bot7_amd.Context(0)
    res["device"] = c.device_info()
    G = bot7_amd.models.gp_regressor
    for name, s in SHAPES.items():
        N, d = s["N"], s["d"]
        X, y, h = problem(N, d)
        c.gp_set_data(X, y)
        a = med(lambda: c.gp_fit_hyp(*h, want_nll=True), 20, 200)
        b = med(lambda: c.gp_fit_hyp_grad(*h), 20, 200)
        g = med(lambda: c.gp_nll_grad(), 20, 200)
        res["fit"][name] = {"N": N, "d": d, "gp_fit_hyp": a, "gp_fit_hyp_grad": b, "gp_nll_grad_alone": g,
                            "added_ms": round(b["median_ms"] - a["median_ms"], 5), "ratio": round(b["median_ms"] / a["median_ms"], 4)}
        L = c._L
        L.b7_profile_enable(c._h, 1)
        L.b7_profile_reset(c._h)
        for _ in range(50):
            c.gp_nll_grad()
        import ctypes as C
        ms, n = C.c_double(), C.c_int64()
        L.b7_profile_get(c._h, b"nll_grad", C.byref(ms), C.byref(n))
        L.b7_profile_enable(c._h, 0)
        dpad = 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 48 if d <= 48 else 64 if d <= 64 else 96
        flops = 2.0 * N ** 3 / 3.0 + 2.0 * N * N * dpad / 2.0
        t = ms.value / max(1, n.value) * 1e-3
        res["kernel"][name] = {"both_launches_ms": round(t * 1e3, 5), "flops_needed": flops, "issue_bound_ms": round(flops / PEAK * 1e3, 6),
                               "fraction_of_issue_bound": round(flops / PEAK / t, 4) if t > 0 else None, "bound": "fp64 MFMA issue, 78.6 TFLOP/s"}
        m = G({})
        h0 = m.init(X, y)
        lo, hi = m._bounds(X, y.reshape(-1, 1))
        t0 = np.clip(m._to_theta(h0), lo, hi)
        runs = []
        for _ in range(3):
            w0 = time.perf_counter()
            r = c.gp_fit_map(t0, lo, hi)
            runs.append(time.perf_counter() - w0)
        res["map"][name] = {"wall_ms_median_of_3": round(float(np.median(runs)) * 1e3, 3), "iters": r["iters"], "evals": r["evals"],
                            "status": r["status"], "nll_start": float(c.gp_fit_map(t0, lo, hi, max_iters=0)["nll"]), "nll_end": r["nll"]}
    c.close()
    outs = [a for a in sys.argv[1:] if not a.startswith("--")]

    def dump():   # after every section: a later one that fails does not take the earlier ones with it
        if outs:
            os.makedirs(os.path.dirname(os.path.abspath(outs[0])), exist_ok=True)
            open(outs[0], "w").write(json.dumps(res, indent=1) + "\n")
    dump()

    # this tree's library against the parent commit's, alternating processes
    if os.path.exists(PARENT_SO) and os.path.exists(PARENT_REV):
        rounds = {"parent": [], "this": []}
        for _ in range(3):
            for which in ("parent", "this"):
                env = dict(os.environ)
                if which == "parent":
                    env["NLLGRAD_COST_TREE"] = PARENT
                o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
                if o.returncode != 0:
                    raise RuntimeError(o.stderr[-2000:])
                rounds[which].append(json.loads(o.stdout.strip().splitlines()[-1]))
        cmp = {"parent_rev": open(PARENT_REV).read().strip()}
        for shape in SHAPES:
            for call in ("gp_fit_hyp", "gp_nll_batch16", "eval_nominate"):
                p = [r[shape][call]["median_ms"] for r in rounds["parent"]]
                t = [r[shape][call]["median_ms"] for r in rounds["this"]]
                cmp["%s/%s" % (shape, call)] = {"parent_ms": p, "this_ms": t, "ratio_of_medians": round(float(np.median(t) / np.median(p)), 4),
                                                "parent_spread": round(float(max(p) / min(p)), 4),
                                                "inside_parent_spread": bool(min(p) / max(p) <= np.median(t) / np.median(p) <= max(p) / min(p))}
        res["parent"] = cmp
    else:
        res["parent"] = "not measured: tools/_build/parent is not built (python tools/nllgrad_cost.py --build-parent REV)"

    dump()
    if "--no-quality" not in sys.argv:
        from harness import default_regime as dr
        arms = {"heuristic": dict(sample=False, nSamples=1), "map": dict(fit="map", nSamples=1), "slice10": dict(nSamples=10)}
        q = {}
        for arm, over in arms.items():
            bests, rates = [], []
            for seed in range(5):
                cc = bot7_amd.Context(0)
                w0 = time.perf_counter()
                out = dr.run(cc, bot_seed=4 + seed, model_seed=6 + seed, **over)
                rates.append(len(out["nominees"]) / (time.perf_counter() - w0))
                bests.append(out["best"]["y"])
                cc.close()
            q[arm] = {"best_per_seed": [round(float(v), 6) for v in bests], "median_best": round(float(np.median(bests)), 6),
                      "trials_per_s_median": round(float(np.median(rates)), 2)}
        res["quality_hartmann6"] = q
    else:
        res["quality_hartmann6"] = "not measured"
    dump()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--build-parent" in sys.argv:
        i = sys.argv.index("--build-parent")
        if i + 1 >= len(sys.argv):
            sys.exit("usage: nllgrad_cost.py --build-parent REV   (the commit this change sits on, e.g. HEAD~1 once it is committed)")
        build_parent(sys.argv[i + 1])
    else:
        main()
