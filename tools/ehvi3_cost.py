"""What three-objective nomination costs: three b7_eval_posterior calls (one per objective's context) + b7_ehvi3_nominate against
three plain b7_eval_nominate (EI) calls on the same inputs, timed in the same run, at the headline shape (N = 2048, d = 32, 2^20
candidates, S = 1 each, P = 32 and P = 128) and the default regime's shape (N = 100, d = 6, 2e4 candidates, S = 10 each, P = 16).
Per case: wall time per call (median and min .. max over the rounds, after warm-up) of the pieces and of the whole; the GPU time of
the two kernels alone (the "ehvi3_tab" / "ehvi3_box" phase events of a profiled call, summed over the chunks), each against its own
bound:
  the table kernel against VALU issue: one Psi with its add costs VALU_PER_PSI vector instructions (counted in the ISA that ships:
    148 in the sample loop's body per cut), a candidate sum_m cuts_m S_m of them, a wave64 instruction 4 cycles on one of the 4 SIMDs
    of a CU, at the 2.4 GHz the 78.6 TFLOP/s of gemm_f64.h stands for; the loads, the square root per sample, the divisions and the
    scalar work are not in the bound;
  the box walk against bytes: five table reads of 8 bytes per box and candidate, against HBM_BYTES_PER_S (8 TB/s, the board's
    figure); the rate reached is recorded beside it -- a chunk's table (at most 256 MiB) is read about three times over while the
    caches still hold much of it, so the rate may exceed what memory gives.
With --parent-tree DIR (a checkout of the parent commit with its library built: DIR/bot7_amd): the TWO-objective nomination (two
b7_eval_posterior + b7_ehvi_nominate, tools/ehvi_cost.py's shapes) under this build and under the parent's, in child processes of
this run, alternating, three times each -- nothing of its path changed, so the two should agree within the spread of the parent's
own repeats, which is recorded beside them.  Prints one JSON object.
usage (GPU box): python tools/ehvi3_cost.py [out.json] [--parent-tree DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np
ROOT = os.environ.get("B7_COST_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # (the --ehvi2-only child's tree)
sys.path.insert(0, ROOT)
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402

CASES = [("headline_P32", dict(N=2048, d=32, M=1 << 20, S=1, P=32, warm=2, rounds=5)),
         ("headline_P128", dict(N=2048, d=32, M=1 << 20, S=1, P=128, warm=2, rounds=5)),
         ("default", dict(N=100, d=6, M=20000, S=10, P=16, warm=5, rounds=30))]
TWO = {"default": dict(N=100, d=6, M=20000, S=10, P=16, warm=5, rounds=30),
       "headline": dict(N=2048, d=32, M=1 << 20, S=1, P=32, warm=2, rounds=5)}
VALU_PER_PSI = 148
CLOCK_HZ = 2.4e9
HBM_BYTES_PER_S = 8.0e12


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


def inputs(sh, rng, centres=(0.25, 0.5, 0.75)):
    """Response columns over the same points (three_spheres' shape: distances to centres on the diagonal), S hyper samples each."""
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.stack([((X - c) ** 2).sum(1) for c in centres], axis=1) + 0.01 * rng.standard_normal((N, len(centres)))
    hyps = []
    for col in range(len(centres)):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y[:, col].mean())}
                     for s in range(S)])
    return X, Y, hyps


def front3_of(P, Y):
    """P canonical points on a tilted plane across the observed range (general position: 2P + 1 boxes), under a reference point just
    beyond the observations."""
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    ref = hi + 0.1 * (hi - lo)
    rng = np.random.default_rng(P)
    ab = rng.uniform(0.05, 0.6, (P, 2))
    t = np.concatenate([ab, 0.95 - ab.sum(axis=1, keepdims=True) * 0.75], axis=1)
    front, _ = _lib.pareto_front3(lo + t * (ref - lo) * 0.9, ref)
    return front, ref


def front2_of(P, Y):
    ref = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    t = (np.arange(P) + 0.5) / P
    lo = Y.min(axis=0)
    return np.stack([lo[0] + t * (ref[0] - lo[0]) * 0.9, lo[1] + (1.0 - t) * (ref[1] - lo[1]) * 0.9], axis=1), ref


def ehvi2_only():
    """The child of --parent-tree: two-objective nominations at tools/ehvi_cost.py's shapes with the package of the tree B7_COST_TREE names."""
    c1, c2 = bot7_amd.Context(0), bot7_amd.Context(0)
    rng = np.random.default_rng(0)
    out = {}
    for name, sh in TWO.items():
        X, Y, hyps = inputs(sh, rng, centres=(0.25, 0.75))
        front, ref = front2_of(sh["P"], Y)
        for c, col in ((c1, 0), (c2, 1)):
            c.grid_sobol(sh["M"], sh["d"], 1, download=False)
            c.gp_set_data(X, Y[:, col:col + 1])

        def whole():
            c1.eval_posterior(hyps[0])
            c2.eval_posterior(hyps[1])
            return c1.ehvi_nominate(c2, front, ref)
        out[name] = {"whole": timed(whole, sh["warm"], sh["rounds"]),
                     "ehvi_nominate": timed(lambda: c1.ehvi_nominate(c2, front, ref), sh["warm"], sh["rounds"])}
    c1.close()
    c2.close()
    print(json.dumps(out))


def main(argv):
    if "--ehvi2-only" in argv:
        return ehvi2_only()
    parent = argv[argv.index("--parent-tree") + 1] if "--parent-tree" in argv else None
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--parent-tree")]
    out = {}
    cs = [bot7_amd.Context(0) for _ in range(3)]
    c1 = cs[0]
    cus = c1.device_info()["compute_units"]
    rng = np.random.default_rng(0)
    staged = None
    for name, sh in CASES:
        N, d, M, S, P = sh["N"], sh["d"], sh["M"], sh["S"], sh["P"]
        if staged != (N, d, M, S):
            X, Y, hyps = inputs(sh, rng)
            for col, c in enumerate(cs):
                c.grid_sobol(M, d, 1, download=False)
                c.gp_set_data(X, Y[:, col:col + 1])
            staged = (N, d, M, S)
        front, ref = front3_of(P, Y)
        boxes = _lib.nondominated_boxes3(front, ref)
        cuts = [len(set(front[:, m])) + 1 for m in range(3)]
        fmin = [[float(Y[:, col].min())] for col in range(3)]

        def three_ei():
            for col, c in enumerate(cs):
                c.eval_nominate(hyps[col], score="ei", fmin=fmin[col])

        def whole():
            for col, c in enumerate(cs):
                c.eval_posterior(hyps[col])
            return c1.ehvi3_nominate(cs[1], cs[2], front, ref)

        r = {"shape": dict({k: sh[k] for k in ("N", "d", "M", "S", "P")}, front=len(front), boxes=len(boxes), cuts=cuts)}
        r["ei_nominate"] = timed(lambda: c1.eval_nominate(hyps[0], score="ei", fmin=fmin[0]), sh["warm"], sh["rounds"])
        r["three_ei_nominates"] = timed(three_ei, sh["warm"], sh["rounds"])
        r["eval_posterior"] = timed(lambda: c1.eval_posterior(hyps[0]), sh["warm"], sh["rounds"])
        r["three_posteriors_and_ehvi3_nominate"] = timed(whole, sh["warm"], sh["rounds"])
        r["ehvi3_nominate"] = timed(lambda: c1.ehvi3_nominate(cs[1], cs[2], front, ref), sh["warm"], sh["rounds"])
        r["whole_over_three_ei"] = round(r["three_posteriors_and_ehvi3_nominate"]["median_ms"] / r["three_ei_nominates"]["median_ms"], 3)
        c1.profile_enable(True)
        tab, box, chunks = [], [], 0
        for _ in range(5):
            c1.profile_reset()
            c1.ehvi3_nominate(cs[1], cs[2], front, ref)
            tab.append(c1.profile_get("ehvi3_tab")[0])
            box.append(c1.profile_get("ehvi3_box")[0])
            chunks = c1.profile_get("ehvi3_tab")[1]
        c1.profile_enable(False)
        waves = (M + 63) // 64
        per_candidate = sum(cuts) * S * VALU_PER_PSI
        tb = {"valu_per_psi": VALU_PER_PSI, "valu_per_candidate": per_candidate, "work_items": waves * sum((k + 7) // 8 for k in cuts),
              "bound_ms": round(waves * per_candidate * 4.0 / (4.0 * cus * CLOCK_HZ) * 1e3, 4), "measured_ms": round(float(np.median(tab)), 4)}
        tb["fraction_of_bound"] = round(tb["bound_ms"] / tb["measured_ms"], 3) if tb["measured_ms"] > 0 else None
        nbytes = float(M) * len(boxes) * 40.0
        bb = {"bytes_read": nbytes, "bound_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4), "measured_ms": round(float(np.median(box)), 4)}
        bb["fraction_of_bound"] = round(bb["bound_ms"] / bb["measured_ms"], 3) if bb["measured_ms"] > 0 else None
        bb["bytes_per_s"] = round(nbytes / (bb["measured_ms"] * 1e-3), 0) if bb["measured_ms"] > 0 else None
        r["chunks"], r["table_kernel"], r["box_kernel"] = chunks, tb, bb
        out[name] = r
    for c in cs:
        c.close()
    if parent:
        runs = {"this": [], "parent": []}
        for _ in range(3):
            for which, tree in (("parent", parent), ("this", None)):
                env = dict(os.environ)
                env.pop("B7_COST_TREE", None)
                if tree:
                    env["B7_COST_TREE"] = os.path.abspath(tree)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ehvi2-only"], env=env, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    raise RuntimeError("two-objective child (%s) failed: %s" % (which, res.stderr[-2000:]))
                runs[which].append(json.loads(res.stdout.strip().splitlines()[-1]))
        cmp_ = {}
        for name in TWO:
            cmp_[name] = {}
            for what in ("whole", "ehvi_nominate"):
                med = {w: [x[name][what]["median_ms"] for x in runs[w]] for w in runs}
                cmp_[name][what] = {"this_median_ms": med["this"], "parent_median_ms": med["parent"],
                                    "parent_spread_ms": round(max(med["parent"]) - min(med["parent"]), 4),
                                    "this_minus_parent_ms": round(float(np.median(med["this"]) - np.median(med["parent"])), 4)}
        out["two_objectives_against_parent"] = cmp_
    print(json.dumps(out))
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
