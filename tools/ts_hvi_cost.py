"""What multi-objective Thompson sampling costs: b7_ts_paths per objective + b7_ts_hvi_nominate / b7_ts_hvi3_nominate against the EHVI
nomination of the same shape (two or three b7_eval_posterior + b7_ehvi_nominate / b7_ehvi3_nominate) and against the same number of
plain b7_ts_nominate calls, on the same inputs, timed in the same run, at the headline shape (N = 2048, d = 32, 2^20 candidates,
S = 1 per objective, F = 1024) and the default regime's shape (N = 100, d = 6, 2e4 candidates, S = 10); two objectives at P = 32,
three at P = 32 and P = 128; q = 1 and q = 16.  Per case: wall time per call (median and min .. max over the rounds, after
warm-up) of the pieces and of the whole, and, from the phase events of profiled calls under BOTH layouts of the picks' reads (the
diagnostic build's B7_TS_HVI_LAYOUT: 0 = column j of [M][q] at stride q, 1 = a [q][M] copy made once per call by ts_transpose_kernel):
  per pick the score + arg-max kernel's GPU time over its byte bound, m M 8 bytes at the device-copy rate measured in this run (a
    256 MiB device-to-device copy by torch, read + write counted);
  the transposition's GPU time per call;
  the per-pick host round trip: (the nomination's wall time - the kernels' and the transposition's GPU time) / q.
Prints one JSON object.
usage (GPU box): python tools/ts_hvi_cost.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402

F = 1024
SHAPES = {"default": dict(N=100, d=6, M=20000, S=10, warm=5, rounds=20),
          "headline": dict(N=2048, d=32, M=1 << 20, S=1, warm=2, rounds=5)}
SETTINGS = [(2, 32), (3, 32), (3, 128)]
QS = (1, 16)


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
    Y = np.stack([((X - c) ** 2).sum(1) for c in (0.25, 0.5, 0.75)], axis=1) + 0.01 * rng.standard_normal((N, 3))
    hyps = []
    for col in range(3):
        amp = float(np.var(Y[:, col]))
        hyps.append([{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y[:, col].mean())}
                     for s in range(S)])
    return X, Y, hyps


def front_of(m, P, Y):
    """P canonical points across the observed range under a reference point just beyond the observations: the anti-diagonal for two
    objectives, a tilted plane for three (general position: 2P + 1 boxes)."""
    Y = Y[:, :m]
    lo, hi = Y.min(axis=0), Y.max(axis=0)
    ref = hi + 0.1 * (hi - lo)
    if m == 2:
        t = (np.arange(P) + 0.5) / P
        return np.stack([lo[0] + t * (ref[0] - lo[0]) * 0.9, lo[1] + (1.0 - t) * (ref[1] - lo[1]) * 0.9], axis=1), ref
    ab = np.random.default_rng(P).uniform(0.05, 0.6, (P, 2))
    t = np.concatenate([ab, 0.95 - ab.sum(axis=1, keepdims=True) * 0.75], axis=1)
    return _lib.pareto_front3(lo + t * (ref - lo) * 0.9, ref)[0], ref


def make_contexts(lib, layout):
    if layout is not None:
        os.environ["B7_TS_HVI_LAYOUT"] = str(layout)
    try:
        return [bot7_amd.Context(0, lib=lib) for _ in range(3)]
    finally:
        os.environ.pop("B7_TS_HVI_LAYOUT", None)


def stage_all(cs, sh, X, Y):
    for k, c in enumerate(cs):
        c.grid_sobol(sh["M"], sh["d"], 1, download=False)
        c.gp_set_data(X, Y[:, k:k + 1])


def picks_profile(cs, m, q, front, ref, M, rate):
    """Phase events of profiled nominations on cs (paths kept already) -> the per-pick kernel time, the transposition, the bound."""
    c = cs[0]
    others = cs[1] if m == 2 else cs[1:m]
    c.profile_enable(True)
    kern, tr, wall, launches = [], [], [], 0
    for _ in range(5):
        c.profile_reset()
        t0 = time.perf_counter()
        c.ts_hvi_nominate(others, front, ref)
        wall.append((time.perf_counter() - t0) * 1e3)
        k = c.profile_get("hvi2" if m == 2 else "hvi3")
        kern.append(k[0])
        launches = int(k[1])
        tr.append(c.profile_get("ts_transpose")[0])
    c.profile_enable(False)
    per_pick = float(np.median(kern)) / max(launches, 1)
    bound = m * M * 8 / rate * 1e3
    return {"kernel_ms_per_pick": round(per_pick, 5), "byte_bound_ms_per_pick": round(bound, 5),
            "kernel_over_bound": round(per_pick / bound, 3), "transpose_ms_per_call": round(float(np.median(tr)), 5),
            "kernel_launches": launches, "profiled_wall_ms": round(float(np.median(wall)), 4),
            "host_round_trip_ms_per_pick": round((float(np.median(wall)) - float(np.median(kern)) - float(np.median(tr))) / q, 5)}


def main():
    rate = copy_rate()
    out = {"features": F, "device_copy_bytes_per_s": round(rate, 0)}
    shipped = make_contexts(None, None)
    arms = {"strided": make_contexts("diag", 0), "transposed": make_contexts("diag", 1)}
    rng = np.random.default_rng(0)
    for name, sh in SHAPES.items():
        X, Y, hyps = inputs(sh, rng)
        M = sh["M"]
        for cs in [shipped] + list(arms.values()):
            stage_all(cs, sh, X, Y)
        r = {"shape": {k: sh[k] for k in ("N", "d", "M", "S")}}
        r["eval_posterior"] = timed(lambda: shipped[0].eval_posterior(hyps[0]), sh["warm"], sh["rounds"])
        for m, P in SETTINGS:
            front, ref = front_of(m, P, Y)
            cs = shipped[:m]
            others = cs[1] if m == 2 else cs[1:]

            def ehvi():
                for c, h in zip(cs, hyps):
                    c.eval_posterior(h)
                return cs[0].ehvi_nominate(others, front, ref) if m == 2 else cs[0].ehvi3_nominate(others[0], others[1], front, ref)
            e = {"P": int(len(front)), "ehvi_whole": timed(ehvi, sh["warm"], sh["rounds"])}
            for q in QS:
                def paths():
                    for k, (c, h) in enumerate(zip(cs, hyps)):
                        c.ts_paths(h, q, n_features=F, seed=11 + k)

                def whole():
                    paths()
                    return cs[0].ts_hvi_nominate(others, front, ref)

                def plain():
                    for k, (c, h) in enumerate(zip(cs, hyps)):
                        c.ts_nominate(h, q, n_features=F, seed=11 + k)
                w = {"whole": timed(whole, sh["warm"], sh["rounds"]), "ts_paths_all": timed(paths, sh["warm"], sh["rounds"]),
                     "pick_loop": timed(lambda: cs[0].ts_hvi_nominate(others, front, ref), sh["warm"], sh["rounds"]),
                     "plain_ts_nominate_calls": timed(plain, sh["warm"], sh["rounds"])}
                paths()       # (the plain calls left paths too; these are the timed ones again)
                w["whole_over_ehvi"] = round(w["whole"]["median_ms"] / e["ehvi_whole"]["median_ms"], 4)
                w["whole_over_plain_ts"] = round(w["whole"]["median_ms"] / w["plain_ts_nominate_calls"]["median_ms"], 4)
                w["picks"] = [int(i) for i in cs[0].ts_hvi_nominate(others, front, ref)[1]]
                for arm, acs in arms.items():
                    for k, (c, h) in enumerate(zip(acs[:m], hyps)):
                        c.ts_paths(h, q, n_features=F, seed=11 + k)
                    w[arm] = picks_profile(acs, m, q, front, ref, M, rate)
                    w[arm]["pick_loop"] = timed(lambda: acs[0].ts_hvi_nominate(acs[1] if m == 2 else acs[1:m], front, ref), sh["warm"], sh["rounds"])
                e["q%d" % q] = w
            r["m%d_P%d" % (m, P)] = e
        out[name] = r
    for cs in [shipped] + list(arms.values()):
        for c in cs:
            c.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
