"""What the log-space EHVI costs beside the linear one: b7_logehvi_nominate against b7_ehvi_nominate and b7_logehvi3_nominate against
b7_ehvi3_nominate over the same kept posteriors, in the same run, at the shapes of tools/ehvi_cost.py and tools/ehvi3_cost.py: the
default regime's (N = 100, d = 6, 2e4 candidates, S = 10 per objective, P = 16) and the headline's (N = 2048, d = 32, 2^20 candidates,
S = 1, P = 32, and P = 128 for three objectives).  Per shape and front: wall time per nomination (median, min .. max after warm-up)
and the GPU time of each kernel alone (the "ehvi" / "logehvi", "ehvi3_tab" / "logehvi3_tab", "ehvi3_box" / "logehvi3_box" phase events
of a profiled call, summed over the chunks), and log over linear for each.
With --parent-tree DIR (a checkout of the parent commit with its library built: DIR/bot7_amd): this build against the parent's, in
fresh child processes of this run, alternating, three times each.  Every child (1) times the six kernels as above and (2) prints a
SHA-256 of the output bytes of the four *_compute calls on the inputs of the tests' KERNEL_CASES / KERNEL_CASES3, and of the
(value, index) pair and the accumulator's bytes of the four *_nominate calls on the tests' small two- and three-objective problems.
The kernels compute what the parent's computed when every digest is equal in all six children ("digests_equal"), and run as fast when
this build's median lies within the min .. max of the parent's own three repeats ("within_parent_range", with the spread and the
difference of the medians beside it).  Exit status 1 if a digest differs.
Prints one JSON object.  usage (GPU box): python tools/logehvi_cost.py [out.json] [--parent-tree DIR]"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("B7_COST_TREE") or HERE   # (the --child's library tree; the inputs are always this tree's tests')
sys.path.insert(0, ROOT)
import bot7_amd  # noqa: E402

SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, P2=(16,), P3=(16,), warm=3, rounds=15),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, P2=(32,), P3=(32, 128), warm=1, rounds=5)}
PHASES2 = {"linear": ("ehvi",), "log": ("logehvi",)}
PHASES3 = {"linear": ("ehvi3_tab", "ehvi3_box"), "log": ("logehvi3_tab", "logehvi3_box")}


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


def inputs(sh, rng):
    """Three response columns over the same points (distances to three centres), S hyper samples per objective."""
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.stack([((X - c) ** 2).sum(1) for c in (0.25, 0.75, 0.5)], axis=1) + 0.01 * rng.standard_normal((N, 3))
    hyps = []
    for col in range(3):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y[:, col].mean())}
                     for s in range(S)])
    return X, Y, hyps


def front2_of(P, Y):
    ref = Y.max(axis=0)[:2] + 0.1 * (Y.max(axis=0) - Y.min(axis=0))[:2]
    t = (np.arange(P) + 0.5) / P
    lo = Y.min(axis=0)
    return np.stack([lo[0] + t * (ref[0] - lo[0]) * 0.9, lo[1] + (1.0 - t) * (ref[1] - lo[1]) * 0.9], axis=1), ref


def front3_of(P, Y):
    """P mutually non-dominated points on a tilted plane across the observed range (tools/ehvi3_cost.py's construction)."""
    ref = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    lo = Y.min(axis=0)
    rng = np.random.default_rng(P)
    ab = rng.uniform(0.2, 0.6, (P, 2))
    unit = np.concatenate([ab, 1.2 - ab.sum(axis=1, keepdims=True)], axis=1)
    front, _ = bot7_amd._lib.pareto_front3(lo + unit * (ref - lo) * 0.9, ref)
    return front, ref


def kernel_ms(c, fn, phases, rounds=5):
    c.profile_enable(True)
    try:
        got = {p: [] for p in phases}
        for _ in range(rounds):
            c.profile_reset()
            fn()
            for p in phases:
                got[p].append(c.profile_get(p)[0])
    finally:
        c.profile_enable(False)
    return {p: round(float(np.median(v)), 4) for p, v in got.items()}


def digests():
    """SHA-256 of what the eight entry points return on the tests' inputs, under whichever library this process loaded."""
    for p in (HERE, os.path.join(HERE, "tests")):
        if p not in sys.path:
            sys.path.append(p)
    import _ehvi3_ref as R3
    import _ehvi_ref as R2
    import _logehvi_ref as RL
    from test_gpu_ehvi import two_objective_problem
    from test_gpu_ehvi3 import three_objective_problem

    def sha(*arrays):
        return hashlib.sha256(b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)).hexdigest()
    out = {}
    cs = [bot7_amd.Context(0) for _ in range(3)]
    c = cs[0]
    for M, P, S1, S2 in R2.KERNEL_CASES:
        out["ehvi_compute/%d,%d,%d,%d" % (M, P, S1, S2)] = sha(c.ehvi_compute(*R2.make_rows(M, S1, S2), R2.make_front(P), R2.REF))
    for M, P, S1, S2 in RL.KERNEL_CASES:
        out["logehvi_compute/%d,%d,%d,%d" % (M, P, S1, S2)] = sha(c.logehvi_compute(*RL.make_rows_log(M, S1, S2), R2.make_front(P), R2.REF))
    for M, P, S1, S2, S3 in R3.KERNEL_CASES3:
        key = "%d,%d,%d,%d,%d" % (M, P, S1, S2, S3)
        out["ehvi3_compute/" + key] = sha(c.ehvi3_compute(*R3.make_rows3(M, (S1, S2, S3)), R3.make_front3(P), R3.REF3))
        out["logehvi3_compute/" + key] = sha(c.logehvi3_compute(*RL.make_rows3_log(M, (S1, S2, S3)), R3.make_front3(P), R3.REF3))
    for n, prob in ((2, two_objective_problem()), (3, three_objective_problem())):
        X, Y, Xc, hyps = prob[0], prob[1], prob[2], (prob[3:] if n == 2 else prob[3])
        ref = np.full(n, 0.9)
        front = (bot7_amd._lib.pareto_front2 if n == 2 else bot7_amd._lib.pareto_front3)(Y, ref)[0]
        for k in range(n):
            cs[k].gp_set_kernel("ardse")
            cs[k].grid_upload(Xc)
            cs[k].gp_set_data(X, Y[:, k:k + 1])
            cs[k].eval_posterior(hyps[k])
        for name in ("ehvi", "logehvi"):
            call = getattr(c, name + ("3" if n == 3 else "") + "_nominate")
            val, idx = call(*cs[1:n], front, ref)
            out["%s%s_nominate/P%d" % (name, "3" if n == 3 else "", len(front))] = sha([val, float(idx)], c.score_finish(1.0, download=True)[2])
    for c in cs:
        c.close()
    return out


def measure(kinds=("linear", "log")):
    cs = [bot7_amd.Context(0) for _ in range(3)]
    rng = np.random.default_rng(0)
    out = {}
    for name, sh in SHAPES.items():
        X, Y, hyps = inputs(sh, rng)
        for k, c in enumerate(cs):
            c.grid_sobol(sh["M"], sh["d"], 1, download=False)
            c.gp_set_data(X, Y[:, k:k + 1])
            c.eval_posterior(hyps[k])
        r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
        for P in sh["P2"]:
            front, ref = front2_of(P, Y)
            calls = {"linear": lambda: cs[0].ehvi_nominate(cs[1], front, ref), "log": lambda: cs[0].logehvi_nominate(cs[1], front, ref)}
            e = {}
            for kind in kinds:
                e[kind] = {"nominate": timed(calls[kind], sh["warm"], sh["rounds"]), "kernel_ms": kernel_ms(cs[0], calls[kind], PHASES2[kind])}
            if "log" in e:
                e["log_over_linear"] = {"nominate": round(e["log"]["nominate"]["median_ms"] / e["linear"]["nominate"]["median_ms"], 3),
                                        "kernel": round(e["log"]["kernel_ms"]["logehvi"] / e["linear"]["kernel_ms"]["ehvi"], 3)}
            r["two_objectives_P%d" % P] = e
        for P in sh["P3"]:
            front, ref = front3_of(P, Y)
            calls = {"linear": lambda: cs[0].ehvi3_nominate(cs[1], cs[2], front, ref),
                     "log": lambda: cs[0].logehvi3_nominate(cs[1], cs[2], front, ref)}
            e = {"front": len(front)}
            for kind in kinds:
                e[kind] = {"nominate": timed(calls[kind], sh["warm"], sh["rounds"]), "kernel_ms": kernel_ms(cs[0], calls[kind], PHASES3[kind])}
            if "log" in e:
                e["log_over_linear"] = {"nominate": round(e["log"]["nominate"]["median_ms"] / e["linear"]["nominate"]["median_ms"], 3),
                                        "table_kernel": round(e["log"]["kernel_ms"]["logehvi3_tab"] / e["linear"]["kernel_ms"]["ehvi3_tab"], 3),
                                        "box_kernel": round(e["log"]["kernel_ms"]["logehvi3_box"] / e["linear"]["kernel_ms"]["ehvi3_box"], 3)}
            r["three_objectives_P%d" % P] = e
        out[name] = r
    for c in cs:
        c.close()
    return out


def main(argv):
    if "--child" in argv:
        print(json.dumps({"digests": digests(), "times": measure()}))
        return
    parent = argv[argv.index("--parent-tree") + 1] if "--parent-tree" in argv else None
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--parent-tree")]
    out, same = measure(), True
    if parent:
        runs = {"this": [], "parent": []}
        for _ in range(3):
            for which, tree in (("parent", parent), ("this", None)):
                env = dict(os.environ)
                env.pop("B7_COST_TREE", None)
                if tree:
                    env["B7_COST_TREE"] = os.path.abspath(tree)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
                if res.returncode != 0:
                    raise RuntimeError("child (%s) failed: %s" % (which, res.stderr[-2000:]))
                runs[which].append(json.loads(res.stdout.strip().splitlines()[-1]))
                print("child %d of 6 done (%s)" % (len(runs["this"]) + len(runs["parent"]), which), file=sys.stderr, flush=True)
        first = runs["parent"][0]["digests"]
        differing = sorted(k for k in first if any(x["digests"].get(k) != first[k] for w in runs for x in runs[w]))
        same = not differing and all(set(x["digests"]) == set(first) for w in runs for x in runs[w])
        out["digests_against_parent"] = {"digests_equal": same, "compared": len(first), "differing": differing, "sha256": first}
        cmp_ = {}
        for name in SHAPES:
            for key in runs["parent"][0]["times"][name]:
                if key == "shape":
                    continue
                for kind in ("linear", "log"):
                    for phase in runs["parent"][0]["times"][name][key][kind]["kernel_ms"]:
                        ms = {w: [x["times"][name][key][kind]["kernel_ms"][phase] for x in runs[w]] for w in runs}
                        med = float(np.median(ms["this"]))
                        cmp_["%s/%s/%s" % (name, key, phase)] = {
                            "this_ms": ms["this"], "parent_ms": ms["parent"], "parent_spread_ms": round(max(ms["parent"]) - min(ms["parent"]), 4),
                            "this_minus_parent_ms": round(med - float(np.median(ms["parent"])), 4),
                            "within_parent_range": bool(min(ms["parent"]) <= med <= max(ms["parent"]))}
        out["kernels_against_parent"] = cmp_
    print(json.dumps(out))
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main(sys.argv[1:])
