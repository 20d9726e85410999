"""What the knowledge gradient costs: b7_kg_nominate (n = 16 discretisation rows, chosen by the library) against b7_eval_nominate
(EI) on the same inputs, timed in the same run, at the headline shape (N = 2048, d = 32, 2^20 candidates, S = 1) and the
default-regime shape (N = 100, d = 6, 2e4 candidates, S = 10).  Per shape: wall time per call (median and min .. max over the rounds,
after warm-up) and the GPU time of a profiled call split by phase events into
  fits_and_posterior   what b7_eval_nominate itself does (kxx, prep, potrf, trtri, ksx, post, score, argmax),
  rows                 the choice of A on the device, the scaled points and alpha (kg_rows),
  columns              k(X, a_i) over the observations (kg_cols),
  mat_vecs             alpha: the fits' own and the 16 x 2 triangular mat-vecs that make W (the phase event does not tell them apart),
  kg_kernel            the pass over the grid (kg),
  fold                 the accumulator's reset and the fold over the samples (kg_fold)
(profiling serialises the phases, so the split adds up to more than an unprofiled call).  kg_kernel against its own issue bound:
the fp64 MFMA and the fp64 VALU share the same units, so a 16-observation x 16-query tile costs its MFMAs (dpad / 4 for the
distances + 4 against W, 64 cycles each) PLUS its vector instructions (4 cycles each at wave64); VALU_PER_TILE is counted in the
ISA that ships (tools/isa_count.py on kg_kernel's slab loop: 80 per tile under ARD-SE, cov_nonpos4's exponential and the operand
reads).  The bound is tiles x cycles / (4 SIMDs x CUs x clock), at the 2.4 GHz the 78.6 TFLOP/s of gemm_f64.h stands for; the
epilogue (one envelope of 17 lines per query: about 290 fp64 divisions) is not in it and is reported as the remainder.
With --parent-tree DIR (a checkout of the parent commit with its library built: DIR/bot7_amd): b7_eval_nominate (EI) under this
build and under the parent's, in child processes of this run, alternating, three times each -- nothing of its path changed, so the
two should agree within the spread of the parent's own repeats, which is recorded beside them.  Prints one JSON object.
usage (GPU box): python tools/kg_cost.py [out.json] [--parent-tree DIR]"""
import json
import os
import subprocess
import sys
import time

import numpy as np
ROOT = os.environ.get("B7_COST_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # (the --ei-only child's tree)
sys.path.insert(0, ROOT)
import bot7_amd  # noqa: E402

POINTS = 16
SHAPES = {"headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=2, rounds=5),
          "default": dict(N=100, d=6, M=20000, S=10, warm=5, rounds=30)}
PHASES = {"fits_and_posterior": ("kxx", "prep", "potrf", "trtri", "ksx", "post", "score", "argmax"), "rows": ("kg_rows",),
          "columns": ("kg_cols",), "mat_vecs": ("alpha",), "kg_kernel": ("kg",), "fold": ("kg_fold",)}
VALU_PER_TILE = 80     # ARD-SE, every dpad class (318 .. 328 per slab of four tiles; 164 per slab of two at dpad >= 48)
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
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    return X, Y, hyps, [float(Y.min())]


def kg_bound_ms(M, N, d, S, cus):
    dpad = 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 48 if d <= 48 else 64 if d <= 64 else 96
    npad = 64 if N <= 64 else (N + 127) // 128 * 128
    mfmas = dpad // 4 + 4
    cycles = 64 * mfmas + 4 * VALU_PER_TILE
    tiles = ((M + 63) // 64 * 4) * (npad // 16) * S
    return {"mfmas_per_tile": mfmas, "valu_per_tile": VALU_PER_TILE, "cycles_per_tile": cycles, "tiles": tiles,
            "bound_ms": round(tiles * cycles / (4.0 * cus * CLOCK_HZ) * 1e3, 4)}


def ei_only():
    """The child of --parent-tree: EI nominations at both shapes with the package of the tree B7_COST_TREE names."""
    c = bot7_amd.Context(0)
    rng = np.random.default_rng(0)
    out = {}
    for name, sh in SHAPES.items():
        X, Y, hyps, fmin = inputs(sh, rng)
        c.grid_sobol(sh["M"], sh["d"], 1, download=False)
        c.gp_set_data(X, Y)
        out[name] = timed(lambda: c.eval_nominate(hyps, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    c.close()
    print(json.dumps(out))


def main(argv):
    if "--ei-only" in argv:
        return ei_only()
    parent = argv[argv.index("--parent-tree") + 1] if "--parent-tree" in argv else None
    paths = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--parent-tree")]
    out = {"points": POINTS}
    c = bot7_amd.Context(0)
    cus = c.device_info()["compute_units"]
    rng = np.random.default_rng(0)
    for name, sh in SHAPES.items():
        N, d, M, S = sh["N"], sh["d"], sh["M"], sh["S"]
        X, Y, hyps, fmin = inputs(sh, rng)
        c.grid_sobol(M, d, 1, download=False)
        c.gp_set_data(X, Y)
        r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
        r["ei_nominate"] = timed(lambda: c.eval_nominate(hyps, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
        r["kg_nominate"] = timed(lambda: c.kg_nominate(hyps, points=POINTS), sh["warm"], sh["rounds"])
        r["kg_over_ei"] = round(r["kg_nominate"]["median_ms"] / r["ei_nominate"]["median_ms"], 3)
        c.profile_enable(True)
        split, launches = {k: [] for k in PHASES}, {}
        for _ in range(5):
            c.profile_reset()
            c.kg_nominate(hyps, points=POINTS)
            for k, names in PHASES.items():
                got = [c.profile_get(n) for n in names]
                split[k].append(sum(g[0] for g in got))
                launches[k] = int(sum(g[1] for g in got))
        c.profile_enable(False)
        r["split_gpu_ms"] = {k: round(float(np.median(v)), 4) for k, v in split.items()}
        total = sum(r["split_gpu_ms"].values())
        r["split_share"] = {k: round(v / total, 4) for k, v in r["split_gpu_ms"].items()} if total > 0 else None
        r["phase_events"] = launches
        b = kg_bound_ms(M, N, d, S, cus)
        got = r["split_gpu_ms"]["kg_kernel"]
        b["measured_ms"] = got
        b["fraction_of_bound"] = round(b["bound_ms"] / got, 3) if got > 0 else None
        b["remainder_ms"] = round(got - b["bound_ms"], 4)
        r["kg_kernel"] = b
        out[name] = r
    c.close()
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
            cmp_[name] = {"this_median_ms": med["this"], "parent_median_ms": med["parent"],
                          "parent_spread_ms": round(max(med["parent"]) - min(med["parent"]), 4),
                          "this_minus_parent_ms": round(float(np.median(med["this"]) - np.median(med["parent"])), 4)}
        out["ei_against_parent"] = cmp_
    print(json.dumps(out))
    if paths:
        with open(paths[0], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:])
