"""What two-objective nomination costs: two b7_eval_posterior calls (one per objective's context) + b7_ehvi_nominate against two
plain b7_eval_nominate (EI) calls on the same inputs, timed in the same run, at the default-regime shape (N = 100, d = 6, 2e4
candidates, S = 10 + 10, P = 16) and the headline shape (N = 2048, d = 32, 2^20 candidates, S = 1 + 1, P = 32).  Per shape: wall time
per call (median and min .. max over the rounds, after warm-up) of the pieces and of the whole, the GPU time of ehvi2_kernel alone
(the "ehvi" phase event of a profiled call), and that time against the kernel's own VALU issue bound: one Psi costs VALU_PER_PSI
vector instructions (counted in the ISA that ships: the 142-instruction body of ocml's erfc and exp around the division, plus the
branch tails and the strip's add; 154 for objective 1, which also keeps Psi(a_k) and clamps the difference, 150 for objective 2),
a candidate (P + 1)(S1 x 154 + S2 x 150) of them, a wave64 instruction 4 cycles on one of the 4 SIMDs of a CU, at the 2.4 GHz the
78.6 TFLOP/s of gemm_f64.h stands for.  The loads, the row-class test and the loop's scalar work are not in the bound.  Beside it:
what one wave alone needs to issue its candidate's instructions back to back (one_wave_ms), the floor of a grid with fewer
waves than the chip has SIMDs -- the default regime's 313 against 1024.
With --parent-tree DIR (a checkout of the parent commit with its library built: DIR/bot7_amd): b7_eval_nominate (EI) under this
build and under the parent's, in child processes of this run, alternating, three times each -- nothing of its path changed, so the
two should agree within the spread of the parent's own repeats, which is recorded beside them; the comparison "two EI nominations
on the parent" is twice the parent's median.  Prints one JSON object.
usage (GPU box): python tools/ehvi_cost.py [out.json] [--parent-tree DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np
ROOT = os.environ.get("B7_COST_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # (the --ei-only child's tree)
sys.path.insert(0, ROOT)
import bot7_amd  # noqa: E402

SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, P=16, warm=5, rounds=30),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, P=32, warm=2, rounds=5)}
VALU_PER_PSI = (154, 150)     # objective 1, objective 2
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


def inputs(sh, rng):
    """Two response columns over the same points (two_spheres' shape: distances to two centres), S hyper samples per objective."""
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.stack([((X - 0.25) ** 2).sum(1), ((X - 0.75) ** 2).sum(1)], axis=1) + 0.01 * rng.standard_normal((N, 2))
    hyps = []
    for col in range(2):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y[:, col].mean())}
                     for s in range(S)])
    return X, Y, hyps


def front_of(P, Y):
    """P canonical points across the observed range, under a reference point just beyond the observations."""
    ref = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    t = (np.arange(P) + 0.5) / P
    lo = Y.min(axis=0)
    front = np.stack([lo[0] + t * (ref[0] - lo[0]) * 0.9, lo[1] + (1.0 - t) * (ref[1] - lo[1]) * 0.9], axis=1)
    return front, ref


def bound_ms(M, S1, S2, P, cus):
    per_candidate = (P + 1) * (S1 * VALU_PER_PSI[0] + S2 * VALU_PER_PSI[1])
    waves = (M + 63) // 64
    return {"valu_per_psi": list(VALU_PER_PSI), "valu_per_candidate": per_candidate, "waves": waves,
            "bound_ms": round(waves * per_candidate * 4.0 / (4.0 * cus * CLOCK_HZ) * 1e3, 4),
            # what ONE wave needs to issue its own instructions back to back: the floor while there are fewer waves than SIMDs
            "one_wave_ms": round(per_candidate * 4.0 / CLOCK_HZ * 1e3, 4)}


def ei_only():
    """The child of --parent-tree: EI nominations at both shapes with the package of the tree B7_COST_TREE names."""
    c = bot7_amd.Context(0)
    rng = np.random.default_rng(0)
    out = {}
    for name, sh in SHAPES.items():
        X, Y, hyps = inputs(sh, rng)
        c.grid_sobol(sh["M"], sh["d"], 1, download=False)
        c.gp_set_data(X, Y[:, :1])
        fmin = [float(Y[:, 0].min())]
        out[name] = timed(lambda: c.eval_nominate(hyps[0], score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    c.close()
    print(json.dumps(out))


def main(argv):
    if "--ei-only" in argv:
        return ei_only()
    parent = argv[argv.index("--parent-tree") + 1] if "--parent-tree" in argv else None
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--parent-tree")]
    out = {}
    c1, c2 = bot7_amd.Context(0), bot7_amd.Context(0)
    cus = c1.device_info()["compute_units"]
    rng = np.random.default_rng(0)
    for name, sh in SHAPES.items():
        N, d, M, S, P = sh["N"], sh["d"], sh["M"], sh["S"], sh["P"]
        X, Y, hyps = inputs(sh, rng)
        front, ref = front_of(P, Y)
        for c, col in ((c1, 0), (c2, 1)):
            c.grid_sobol(M, d, 1, download=False)
            c.gp_set_data(X, Y[:, col:col + 1])
        fmin = [[float(Y[:, 0].min())], [float(Y[:, 1].min())]]

        def two_ei():
            c1.eval_nominate(hyps[0], score="ei", fmin=fmin[0])
            c2.eval_nominate(hyps[1], score="ei", fmin=fmin[1])

        def whole():
            c1.eval_posterior(hyps[0])
            c2.eval_posterior(hyps[1])
            return c1.ehvi_nominate(c2, front, ref)

        r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S", "P")}}
        r["ei_nominate"] = timed(lambda: c1.eval_nominate(hyps[0], score="ei", fmin=fmin[0]), sh["warm"], sh["rounds"])
        r["two_ei_nominates"] = timed(two_ei, sh["warm"], sh["rounds"])
        r["eval_posterior"] = timed(lambda: c1.eval_posterior(hyps[0]), sh["warm"], sh["rounds"])
        r["two_posteriors_and_ehvi_nominate"] = timed(whole, sh["warm"], sh["rounds"])
        r["ehvi_nominate"] = timed(lambda: c1.ehvi_nominate(c2, front, ref), sh["warm"], sh["rounds"])
        r["whole_over_two_ei"] = round(r["two_posteriors_and_ehvi_nominate"]["median_ms"] / r["two_ei_nominates"]["median_ms"], 3)
        c1.profile_enable(True)
        ker = []
        for _ in range(5):
            c1.profile_reset()
            c1.ehvi_nominate(c2, front, ref)
            ker.append(c1.profile_get("ehvi")[0])
        c1.profile_enable(False)
        b = bound_ms(M, S, S, P, cus)
        b["measured_ms"] = round(float(np.median(ker)), 4)
        b["fraction_of_bound"] = round(b["bound_ms"] / b["measured_ms"], 3) if b["measured_ms"] > 0 else None
        b["one_wave_over_measured"] = round(b["one_wave_ms"] / b["measured_ms"], 3) if b["measured_ms"] > 0 else None
        r["ehvi_kernel"] = b
        out[name] = r
    c1.close()
    c2.close()
    if parent:
        runs = {"this": [], "parent": []}
        for _ in range(3):
            for which, tree in (("parent", parent), ("this", None)):
                env = dict(os.environ)
                env.pop("B7_COST_TREE", None)
                if tree:
                    env["B7_COST_TREE"] = os.path.abspath(tree)
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ei-only"], env=env, capture_output=True, text=True, timeout=600)
                if res.returncode != 0:
                    raise RuntimeError("EI child (%s) failed: %s" % (which, res.stderr[-2000:]))
                runs[which].append(json.loads(res.stdout.strip().splitlines()[-1]))
        cmp_ = {}
        for name in SHAPES:
            med = {w: [x[name]["median_ms"] for x in runs[w]] for w in runs}
            pm = float(np.median(med["parent"]))
            cmp_[name] = {"this_median_ms": med["this"], "parent_median_ms": med["parent"],
                          "parent_spread_ms": round(max(med["parent"]) - min(med["parent"]), 4),
                          "this_minus_parent_ms": round(float(np.median(med["this"]) - pm), 4),
                          "two_ei_on_the_parent_ms": round(2.0 * pm, 4),
                          "whole_over_two_ei_on_the_parent": round(out[name]["two_posteriors_and_ehvi_nominate"]["median_ms"] / (2.0 * pm), 3)}
        out["ei_against_parent"] = cmp_
    print(json.dumps(out))
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
