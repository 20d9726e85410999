"""What constrained Thompson sampling costs: b7_ts_paths on 1 + C contexts + b7_ts_feas_nominate, at the headline shape (N = 2048,
d = 32, 2^20 candidates, S = 1 per model, F = 1024) for q in {1, 16} and C in {1, 3}, and at the default regime's shape (N = 100,
d = 6, 2e4 candidates, S = 10) for q = 16.  Per case, timed in the same run on the same paths:
  the pick stage's GPU time (phase events of profiled calls) in the one-pass arm (the diagnostic build under B7_TS_FEAS_ONEPASS = 1:
    "ts_feas" + "ts_feas_rerun") and in the per-path arm (B7_TS_FEAS_ONEPASS = 0, the library's default: "ts_feas_paths"), the picks
    checked equal;
  the one pass alone against its byte bound, (1 + C) M q 8 bytes at the device-copy rate measured in this run (a 256 MiB
    device-to-device copy by torch, read + write counted);
  a whole constrained Thompson nomination (wall time, median and min .. max) against 1 + C plain b7_ts_nominate calls;
  the same against constrained LogEI with C constraints: C b7_eval_nominate(LogPI) + b7_feas_add_acc + b7_eval_nominate_feasible.
Prints one JSON object.
usage (GPU box): python tools/ts_feas_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402

F = 1024
SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, warm=3, rounds=10, cases=[(16, 1), (16, 3)]),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=1, rounds=3, cases=[(1, 1), (16, 1), (1, 3), (16, 3)])}


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
    """Bytes per second of a device-to-device copy (read + write), 256 MiB, the best of 10."""
    import torch
    n = (256 << 20) // 8
    a, b = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    b.copy_(a)
    best = float("inf")
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * n * 8 / best


def inputs(sh, rng):
    N, d, S = sh["N"], sh["d"], sh["S"]
    X = rng.random((N, d))
    Y = np.stack([((X - c) ** 2).sum(1) for c in (0.25, 0.4, 0.6, 0.75)], axis=1) + 0.01 * rng.standard_normal((N, 4))
    hyps = []
    for col in range(4):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y[:, col].mean())}
                     for s in range(S)])
    return X, Y, hyps


def contexts(n, lib=None, onepass=None):
    if onepass is not None:
        os.environ["B7_TS_FEAS_ONEPASS"] = str(onepass)
    try:
        return [bot7_amd.Context(0, lib=lib) for _ in range(n)]
    finally:
        os.environ.pop("B7_TS_FEAS_ONEPASS", None)


def pick_gpu_ms(cs, thr, phases, rounds):
    a = cs[0]
    a.profile_enable(True)
    a.ts_feas_nominate(cs[1:], thr)
    a.profile_reset()
    for _ in range(rounds):
        out = a.ts_feas_nominate(cs[1:], thr)
    ms = {p: a.profile_get(p)[0] / rounds for p in phases}
    a.profile_enable(False)
    return ms, out


def main():
    rate = copy_rate()
    res = {"device_copy_GBps": round(rate / 1e9, 1), "F": F, "shapes": {}}
    rng = np.random.default_rng(0)
    for name, sh in SHAPES.items():
        X, Y, hyps = inputs(sh, rng)
        Xc = rng.random((sh["M"], sh["d"]))
        onep, perp = contexts(4, lib="diag", onepass=1), contexts(4, lib="diag", onepass=0)   # the one-pass arm; the per-path arm, the default
        for k in range(4):
            for c in (onep[k], perp[k]):
                c.grid_upload(Xc)
                c.gp_set_data(X, Y[:, k:k + 1])
        out = {"N": sh["N"], "d": sh["d"], "M": sh["M"], "S": sh["S"], "cases": []}
        for q, C in sh["cases"]:
            thr = [float(np.median(Y[:, k])) for k in range(1, 1 + C)]
            n = 1 + C

            def paths(cs):
                for k in range(n):
                    cs[k].ts_paths(hyps[k], q, n_features=F, seed=100 + k)

            paths(onep)
            paths(perp)
            one, o1 = pick_gpu_ms(onep[:n], thr, ("ts_feas", "ts_feas_rerun"), sh["rounds"])
            per, o2 = pick_gpu_ms(perp[:n], thr, ("ts_feas_paths",), sh["rounds"])
            assert np.array_equal(o1["index"], o2["index"]) and np.array_equal(o1["key"], o2["key"]) and np.array_equal(o1["cls"], o2["cls"])
            bound_ms = n * sh["M"] * q * 8 / rate * 1e3
            whole = timed(lambda: (paths(perp), perp[0].ts_feas_nominate(perp[1:n], thr)), sh["warm"], sh["rounds"])
            pick_wall = timed(lambda: perp[0].ts_feas_nominate(perp[1:n], thr), sh["warm"], sh["rounds"])
            plain = timed(lambda: [perp[k].ts_nominate(hyps[k], q, n_features=F, seed=100 + k) for k in range(n)], sh["warm"], sh["rounds"])

            def logei():
                for k in range(1, n):
                    perp[k].eval_nominate(hyps[k], score="logpi", fmin=[thr[k - 1]], tradeoff=0.0)
                perp[0].feas_reset()
                for k in range(1, n):
                    perp[0].feas_add_acc(perp[k])
                perp[0].eval_nominate_feasible(hyps[0], score="logei", fmin=[float(Y[:, 0].min())], tradeoff=0.0)

            feas = timed(logei, sh["warm"], sh["rounds"])
            out["cases"].append({"q": q, "C": C, "reruns": o1["reruns"], "classes": o1["cls"].tolist(),
                                 "pick_gpu_ms": {"one_pass": round(one["ts_feas"], 4), "reruns": round(one["ts_feas_rerun"], 4),
                                                 "one_pass_arm_total": round(one["ts_feas"] + one["ts_feas_rerun"], 4),
                                                 "per_path_arm": round(per["ts_feas_paths"], 4)},
                                 "byte_bound_ms": round(bound_ms, 4), "one_pass_over_bound": round(one["ts_feas"] / bound_ms, 2),
                                 "pick_wall": pick_wall, "constrained_ts_nomination": whole, "plain_ts_nominate_calls": plain,
                                 "constrained_logei_nomination": feas})
            print(name, out["cases"][-1], file=sys.stderr, flush=True)
        res["shapes"][name] = out
        for c in onep + perp:
            c.close()
    text = json.dumps(res, indent=1)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
