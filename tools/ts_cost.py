"""What Thompson sampling costs: b7_ts_nominate (F = 1024 features) against b7_eval_nominate (EI) and b7_eval_nominate_batch (EI,
same q) on the same inputs, timed in the same run, at the default-regime shape (N = 100, d = 6, 2e4 candidates, S = 10; q in
{1, 8}) and the headline shape (N = 2048, d = 32, 2^20 candidates, S = 1; q in {1, 16}).  Per shape and q: wall time per call
(median and min .. max over the rounds, after warm-up) and the GPU time of a profiled call split by phase events into
  fits        K(X,X), the factorisations, alpha (kxx, prep, potrf, trtri, alpha) -- min(S, q) of them,
  mean        K(X*,X) and the multi-column posterior mean (ksx, mean),
  features    the random-feature kernel over the observations and over the grid (rff),
  argmins     the 2 q arg-min launches (ts_argmin),
  draws       the generator and the fragment packing (ts_draws)
(profiling serialises the phases, so the split adds up to more than an unprofiled call).  The feature kernel against its own issue
bound: the fp64 MFMA and the fp64 VALU share the same units, so a 16-feature x 16-candidate tile costs its MFMAs (dpad / 4 + 4, 64
cycles each) PLUS its vector instructions (4 cycles each at wave64); VALU_PER_TILE is counted in the ISA that ships -- half of
rff_kernel's loop body, which serves two tiles -- and holds four cosines of 29 instructions (rff_cos with its phase add).  The bound is
tiles x cycles / (4 SIMDs x CUs x clock), at the 2.4 GHz the 78.6 TFLOP/s of gemm_f64.h stands for.  Prints one JSON object.
usage (GPU box): python tools/ts_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

F = 1024
SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, qs=(1, 8), warm=5, rounds=30),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, qs=(1, 16), warm=2, rounds=5)}
PHASES = {"fits": ("kxx", "prep", "potrf", "trtri", "alpha"), "mean": ("ksx", "mean"), "features": ("rff",), "argmins": ("ts_argmin",),
          "draws": ("ts_draws",)}
VALU_PER_TILE = {8: 128, 16: 129, 32: 132, 64: 137, 96: 145}   # vector instructions per 16 x 16 tile of rff_kernel<dpad>, from its ISA
COS_INSTRUCTIONS = 29
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


def rff_bound_ms(rows, d, cus):
    dpad = 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64 if d <= 64 else 96
    mfmas = dpad // 4 + 4
    cycles = 64 * mfmas + 4 * VALU_PER_TILE[dpad]
    tiles = ((rows + 15) // 16) * (F // 16)
    return {"mfmas_per_tile": mfmas, "valu_per_tile": VALU_PER_TILE[dpad], "cycles_per_tile": cycles,
            "bound_ms": round(tiles * cycles / (4.0 * cus * CLOCK_HZ) * 1e3, 4)}


out = {"features": F, "cosine_instructions": COS_INSTRUCTIONS}
c = bot7_amd.Context(0)
cus = c.device_info()["compute_units"]
rng = np.random.default_rng(0)
for name, sh in SHAPES.items():
    N, d, M, S = sh["N"], sh["d"], sh["M"], sh["S"]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    amp = float(np.var(Y))
    hyps = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    fmin = [float(Y.min())]
    c.grid_sobol(M, d, 1, download=False)
    c.gp_set_data(X, Y)
    r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
    r["ei_nominate"] = timed(lambda: c.eval_nominate(hyps, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
    for q in sh["qs"]:
        e = {"ts": timed(lambda: c.ts_nominate(hyps, q, n_features=F, seed=1), sh["warm"], sh["rounds"]),
             "ei_batch": timed(lambda: c.eval_nominate_batch(hyps, q, score="ei", fmin=fmin), sh["warm"], sh["rounds"])}
        e["ts_over_ei_nominate"] = round(e["ts"]["median_ms"] / r["ei_nominate"]["median_ms"], 3)
        e["ts_over_ei_batch"] = round(e["ts"]["median_ms"] / e["ei_batch"]["median_ms"], 3)
        c.profile_enable(True)
        split = {k: [] for k in PHASES}
        launches = {}
        for _ in range(5):
            c.profile_reset()
            c.ts_nominate(hyps, q, n_features=F, seed=1)
            for k, names in PHASES.items():
                got = [c.profile_get(n) for n in names]
                split[k].append(sum(g[0] for g in got))
                launches[k] = int(sum(g[1] for g in got))
        c.profile_enable(False)
        e["split_gpu_ms"] = {k: round(float(np.median(v)), 4) for k, v in split.items()}
        e["phase_events"] = launches
        # the feature kernel runs once over the N observations and once over the M candidates per used hyper sample
        used = min(S, q)
        b = rff_bound_ms(M, d, cus)
        b["bound_ms"] = round(used * (b["bound_ms"] + rff_bound_ms(N, d, cus)["bound_ms"]), 4)
        b["fraction_of_bound"] = round(b["bound_ms"] / e["split_gpu_ms"]["features"], 3) if e["split_gpu_ms"]["features"] > 0 else None
        e["feature_kernel"] = b
        r["q%d" % q] = e
    out[name] = r
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
