"""What Thompson sampling on the DNGO head costs: b7_blr_ts_nominate against b7_blr_eval_nominate (S = 1) / b7_blr_eval_nominate_marg
(S > 1) with EI on the same inputs, timed in the same run, at cfg5's shape (N = 256, d = 5, a 3 x 50 tanh basis, 65 536 candidates) and
with the same network over 2^20 candidates; q in {1, 16}, S in {1, 10}.  Per shape, S and q: wall time per call (median and min ..
max over the rounds, after warm-up) and the GPU time of a profiled call split by phase events into
  basis     the network over the observations and over the grid (basis),
  heads     the S heads (potrf: one launch),
  weights   the q weight draws (blr_ts_weights),
  paths     blr_paths_kernel (blr_paths),
  argmins   the 2 q arg-min launches (ts_argmin)
(profiling serialises the phases, so the split adds up to more than an unprofiled call).  The paths kernel against its byte bound:
it reads the feature buffer once (M zpad 8 bytes, zpad = 64 for 50 features) and writes M q 8 bytes; the rate is what a
device-to-device copy of 512 MiB reaches in this very run (read + written bytes over the median of ten copies).  Prints one JSON
object.
usage (GPU box): python tools/blr_ts_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

SHAPES = {"cfg5": dict(N=256, d=5, M=65536, warm=10, rounds=50), "2^20": dict(N=256, d=5, M=1 << 20, warm=3, rounds=15)}
WIDTHS, ZPAD = [50, 50, 50], 64
QS, SS = (1, 16), (1, 10)
PHASES = {"basis": ("basis",), "heads": ("potrf",), "weights": ("blr_ts_weights",), "paths": ("blr_paths",), "argmins": ("ts_argmin",)}


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


def copy_rate():
    """Bytes read + written per second by a device-to-device copy of 512 MiB (device events, median of ten after two warm-ups)."""
    import torch
    n = (512 << 20) // 8
    src, dst = torch.ones(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    ms = []
    for i in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return 2.0 * n * 8 / (float(np.median(ms)) * 1e-3)


rate = copy_rate()
out = {"copy_rate_TBps": round(rate / 1e12, 3), "zpad": ZPAD}
c = bot7_amd.Context(0)
rng = np.random.default_rng(0)
for name, sh in SHAPES.items():
    N, d, M = sh["N"], sh["d"], sh["M"]
    dims = [d] + WIDTHS
    Wn = [rng.normal(scale=1.0 / np.sqrt(dims[i]), size=(dims[i + 1], dims[i])) for i in range(3)]
    bn = [rng.normal(scale=0.1, size=dims[i + 1]) for i in range(3)]
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    fmin = [float(Y.min())]
    c.grid_sobol(M, d, 1, download=False)
    r = {"shape": {"N": N, "d": d, "M": M, "basis": WIDTHS}}
    for S in SS:
        al, be, mn = [1.0 + 0.1 * s for s in range(S)], [100.0 * (1 + 0.05 * s) for s in range(S)], [float(Y.mean())] * S
        if S == 1:
            ei = timed(lambda: c.blr_eval_nominate(Wn, bn, "Tanh", X, Y, al[0], be[0], mn[0], score="ei", fmin=fmin), sh["warm"], sh["rounds"])
        else:
            ei = timed(lambda: c.blr_eval_nominate_marg(Wn, bn, "Tanh", X, Y, al, be, mn, score="ei", fmin=fmin), sh["warm"], sh["rounds"])
        rs = {"ei_nominate": ei}
        for q in QS:
            e = {"ts": timed(lambda: c.blr_ts_nominate(Wn, bn, "Tanh", X, Y, al, be, mn, q, seed=1), sh["warm"], sh["rounds"])}
            e["ts_over_ei_nominate"] = round(e["ts"]["median_ms"] / ei["median_ms"], 3)
            c.profile_enable(True)
            split = {k: [] for k in PHASES}
            launches = {}
            for _ in range(7):
                c.profile_reset()
                c.blr_ts_nominate(Wn, bn, "Tanh", X, Y, al, be, mn, q, seed=1)
                for k, names in PHASES.items():
                    got = [c.profile_get(n) for n in names]
                    split[k].append(sum(g[0] for g in got))
                    launches[k] = int(sum(g[1] for g in got))
            c.profile_enable(False)
            e["split_gpu_ms"] = {k: round(float(np.median(v)), 4) for k, v in split.items()}
            e["phase_events"] = launches
            nbytes = M * ZPAD * 8 + M * q * 8
            bound = nbytes / rate * 1e3
            e["paths_kernel"] = {"bytes": nbytes, "bound_ms": round(bound, 4),
                                 "fraction_of_bound": round(bound / e["split_gpu_ms"]["paths"], 3) if e["split_gpu_ms"]["paths"] > 0 else None}
            rs["q%d" % q] = e
        r["S%d" % S] = rs
    out[name] = r
c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
