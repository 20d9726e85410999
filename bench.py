#!/usr/bin/env python
"""Headline benchmark: EI candidates scored per second at N = 2048 observations, d = 32 (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--candidates M_PER_GPU] [--workload metric|cfg2|cfg3|cfg4|cfg5|default]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path (bots/bayesopt.lua:56-99) over this rank's shard of the candidate grid, everything
resident in HBM: per GP hyper sample K(X,X) assembly + blocked Cholesky + L^-1 + alpha (the GP fit, redundantly on
every rank; only the d + 3 hypers are uploaded, the data were put on the device once with b7_gp_set_data),
K(X*,X) assembly + posterior mean, posterior variance (the M*N^2 fp64-MFMA GEMM), EI, score:add; then score:div,
arg-max and the single (value, index) exchange -- b7_score_finish_global: RCCL inside libbot7hip.so.  Weak scaling:
every rank owns --candidates rows of one global candidate list.

Inputs (synthetic, deterministic): a Sobol pool of M_total + N points in the unit cube (grids/sobol.lua
semantics, generated on the GPU; the counter-based uniform grid for d >= 40, beyond the reference's Sobol table);
observations = pool rows 1 + k*floor((M_total+N)/N), k = 0..N-1, removed from the pool by stable deletion
(utils/tensor.lua:158-170); candidates = the remaining M_total rows in order.  One departure from 8(d), config.skip = 2
instead of 1 (grids/sobol.lua:70): Sobol point 1 is (0.5, ..., 0.5), the EXACT global minimum of ackley / rastrigin
(benchmarks/ackley.lua:16-17).  As a candidate it wins trivially (round 1: best.index1 = 1); as an observation, which
is where 8(d)'s strided pick puts it, f_min = 0 and EI is identically 0 over the whole grid, so the arg-max is the
first of 2^20 ties.  Starting the pool at point 2 keeps every other property of the recipe and gives a winner in the
interior of the grid that the CPU leg re-derives.  Rank r owns candidate rows [r*M, (r+1)*M): it generates the contiguous pool range that holds them and
deletes the observation rows inside it (b7_grid_remove_rows).  Y = the reference's objective restated on the host
(harness/benchmarks.py); hypers lenscale_sq = d/8, amp = var(Y), mean = mean(Y), noise = 1e-4*amp.

A plain run sets up, warms up, times --steps steps (HIP events around every kernel phase, as the phases and rooflines of the line
are read from them) and prints one JSON line; `value` and `ms_per_step` come from those steps.  --full adds what takes runs of its
own: the same steps without the phase events, the S = 10 leg, GP-fit timings by N, the CPU baseline and the oracle's check of
the winner, and for the metric workload the other BASELINE configurations and the default regime.  --dump-outputs DIR writes
what the last timed step computed: the winner (best_value, best_index1) and the scores score:div left over the candidates
(scores; when they do not fit in 64 MB a fixed, seeded sample, with scores_index1), or for --workload default the last
experiment's nominees, observations, responses and hyper draws.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (d, N, default per-GPU M, objective, score)
    "metric": (32, 2048, 1 << 20, "ackley", "ei"),
    "cfg4": (64, 2048, 262144, "rastrigin", "ei"),   # BASELINE config 4: 2M candidates over 8 GPUs; d = 64 is beyond
                                                     # the reference's Sobol table (dims < 40) -> counter-based grid
    "cfg3": (32, 1024, 262144, "ackley", "ei"),
    "cfg2": (6, 256, 32768, "hartmann6", "cb"),
    "cfg5": (5, 256, 65536, "dngo", "ei"),           # BASELINE config 5: DNGO head (3 x 50 tanh basis), 65536 candidates
    # the reference's OWN default experiment (examples/run_benchmark.lua:30-36, bots/abstract.lua:63-67,79-80): a whole trial
    # loop, not one frozen nomination -- see run_default() below; a step = one experiment of `budget` trials
    "default": (6, 100, 20000, "hartmann6", "ei"),
}
FP64_MFMA_PEAK_TFLOPS = 78.6  # 256 CU x 4 SIMD x 32 flop/clk x 2.4 GHz; measured 74.5-77.3 (profiles/r01_mfma_f64_probe.txt)
GPU_CLOCK_HZ = 2.4e9           # shader clock under load (profiles/r04_post_clock.txt)
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md
SOBOL_SKIP = 2                 # config.skip of the pool: see "Inputs" above
PMC_SUMMARIES = ("r04_pmc_summary.json", "r03_pmc_summary.json", "r02_pmc_summary.json", "r01z_pmc_summary.json")  # newest first
KSX_PMC_BY_CLASS = "r04_ksx_pmc_by_class.json"   # instruction counts of ksx_kernel per width class (tools/ksx_pmc.sh; covar.hip unchanged since round 3)
DUMP_LIMIT_BYTES = 64 * 10 ** 6   # --dump-outputs: all files of all processes together (each process gets its share)
NPY_HEADER_BYTES = 128            # what np.save puts in front of the data of a 1-D or 2-D float64 array


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="metric", choices=sorted(WORKLOADS))
    ap.add_argument("--candidates", type=int, default=0, help="candidates per GPU (default: the workload's)")
    ap.add_argument("--samples", type=int, default=1,
                    help="GP hyper samples marginalised per step (the reference's nSamples is 10, bots/abstract.lua:67); "
                         "the headline metric is quoted for 1, the S = 10 loop is reported beside it ('marginalised')")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the marginalised (S = 10) leg and gp_fit_ms_by_N")
    ap.add_argument("--backend", default="rccl", choices=["rccl", "nccl", "gloo"],
                    help="rccl (= nccl): the exchange is b7_score_finish_global, RCCL inside libbot7hip.so; gloo: ranks "
                         "may share one GPU and exchange through torch.distributed on the CPU (rehearsal of N > 1)")
    ap.add_argument("--cpu-sample", type=int, default=131072, help="candidates in the bounded CPU-baseline sample")
    ap.add_argument("--workspace-mib", type=int, default=0, help="K(X*,X) chunk workspace (default: the library's)")
    ap.add_argument("--layout", default="auto", choices=["auto", "group", "ranks"],
                    help="N > 1: 'ranks' = one process per GPU (torch.distributed.run launches them; b7_comm_*), 'group' = ONE process "
                         "driving N GPUs (b7_group_*: the reference's own layout, bots/abstract.lua:155-169); auto: ranks when a "
                         "launcher set RANK, else group")
    ap.add_argument("--virtual-ranks", action="store_true",
                    help="group layout on fewer than N devices: members share device 0 (rehearsal on a one-GPU box; RCCL refuses "
                         "that, the exchange is merged on the host unless the diagnostic build + test double force the grouped call)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the second timed pass without phase events, the S = 10 leg, the GP-fit "
                         "timings, the CPU baseline and the oracle's check of the winner, the other BASELINE configurations and the "
                         "default regime (--workload default: its per-kernel figures and the oracle-driven loop).  Off: set up, "
                         "warm up, time --steps steps, print the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (float64, 64 MB at most)")
    return ap.parse_args()


# ---- SURVEY 8(d) input construction ------------------------------------------------------------------------------
def pool_index(j, N, s):
    """Pool row (0-based) of candidate j (0-based) once the N observation rows k*s have been deleted."""
    head = N * (s - 1)
    return (j // (s - 1)) * s + 1 + j % (s - 1) if j < head else N * s + (j - head)


def make_inputs(ctx, d, N, M_total, lo, hi):
    """Observations on the host, this rank's candidate rows [lo, hi) resident on the device."""
    s = (M_total + N) // N
    sobol = d < 40
    gen = (lambda size, first: ctx.grid_sobol(size, d, SOBOL_SKIP + first)) if sobol else \
          (lambda size, first: ctx.grid_random(size, d, seed=1, row_offset=first))
    X_obs = np.concatenate([gen(1, k * s) for k in range(N)], axis=0)
    if hi > lo:
        p0, p1 = pool_index(lo, N, s), pool_index(hi - 1, N, s)
        if sobol:
            ctx.grid_sobol(p1 - p0 + 1, d, SOBOL_SKIP + p0, download=False)
        else:
            ctx.grid_random(p1 - p0 + 1, d, seed=1, row_offset=p0, download=False)
        k0 = -(-p0 // s)                                     # first observation index with k*s >= p0
        inside = [k * s - p0 + 1 for k in range(k0, N) if k * s <= p1]
        if inside:
            ctx.grid_remove_rows(inside, want_rows=False)
        assert ctx.grid_shape()[0] == hi - lo
    return X_obs


def usable_cores():
    """Threads this process can actually run at once: the affinity mask, cut down to the cgroup's CPU quota when there is one
    (a container on a 256-core host with cpu.max = 16 CPUs runs 16 threads' worth, whatever the mask says)."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]            # cgroup v2
        if quota != "max":
            cores = max(1, min(cores, int(-(-int(quota) // int(period)))))
    except Exception:
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())              # cgroup v1
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0 and period > 0:
                cores = max(1, min(cores, -(-quota // period)))
        except Exception:
            pass
    return cores


def cpu_baseline(d, N, score, X_obs, Y, hyp, X_hid, window0=0):
    """The oracle (port of the Torch7 CPU path: BLAS dgemm / LAPACK dpotrf / dtrtrs through numpy+scipy) timed on
    this box's host cores on a bounded sample of the same workload: one fit + len(X_hid) candidates, rows
    [window0, window0 + len(X_hid)) of rank 0's shard -- the window that holds the GPU's global winner."""
    from oracle import cport, gp
    cores = usable_cores()
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=cores)
    except Exception:
        limiter = None
    sample = X_hid.shape[0]
    t0 = time.perf_counter()
    f = gp.fit(X_obs, Y, **hyp)
    t_fit = time.perf_counter() - t0
    mu, var = gp.predict(f, X_hid)
    if score == "ei":
        s = cport.ei(mu, var, [float(Y.min())])
    else:
        s = cport.cb(mu, var)
    idx, val = cport.argmax_first(s)
    t = time.perf_counter() - t0
    if limiter is not None and hasattr(limiter, "unregister"):
        limiter.unregister()
    top2 = np.partition(s, -2)[-2:]
    return {"value": sample / t, "unit": "candidates/s", "cores": cores, "kind": "port",
            "sample": "1 GP fit (N=%d, %.3f s) + %d candidates of rank 0's shard (rows %d..%d, the window around the GPU's "
                      "global winner) scored with %s in %.2f s (numpy/scipy OpenBLAS+LAPACK restatement of the Torch7 "
                      "CPU path; not Torch7 itself)" % (N, t_fit, sample, window0 + 1, window0 + sample, score.upper(), t),
            "gp_fit_ms": t_fit * 1e3, "argmax1": int(idx), "best_value": float(val),
            "top2_gap": float(top2[1] - top2[0])}, s


def pmc_traffic(rows_per_launch, N):
    """HBM bytes per post_kernel launch from the committed rocprofv3 --pmc passes (FETCH_SIZE doubled per
    MI355X_MICROARCH.md, + WRITE_SIZE), when they were taken at this launch shape; None otherwise."""
    for name in PMC_SUMMARIES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                p = json.load(f)
            if int(p["rows_per_launch"]) == int(rows_per_launch) and int(p["n_obs"]) == int(N):
                return float(p["kernels"]["post_kernel"]["hbm_bytes_per_launch"]), "profiles/" + name
        except Exception:
            pass
    return None, None


def dump_bytes(arrays):
    """Bytes the .npy files of `arrays` take (data + header)."""
    return sum(np.asarray(a).size * 8 + NPY_HEADER_BYTES for a in arrays.values())


def dump_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: one float64 .npy per array under out_dir, `limit` bytes at most in all (this process's share of
    DUMP_LIMIT_BYTES when several processes write into the same directory)."""
    arrays = {name: np.ascontiguousarray(a, dtype=np.float64) for name, a in arrays.items()}
    total = dump_bytes(arrays)
    if total > limit:
        raise ValueError("--dump-outputs: %d bytes exceed the limit of %d" % (total, limit))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def nomination_outputs(ctx, best, suffix="", limit=DUMP_LIMIT_BYTES):
    """What a nomination step computed: the winner it hands back (value, 1-based global index) and the scores that score:div left
    on the device over this process's candidates (bots/bayesopt.lua's score tensor).  Dividing them by 1.0 again reads them back
    unchanged.  All of them when they fit in `limit` bytes beside the winner; otherwise a fixed, seeded sample of the rows, as
    many as fit together with their 1-based local indices (scores_index1: 16 bytes a row)."""
    out = {"best_value" + suffix: [best[0]], "best_index1" + suffix: [best[1]]}
    room = limit - dump_bytes(out)
    M = ctx.grid_shape()[0]
    if M > 0:
        _, _, scores = ctx.score_finish(1.0, download=True)
        if M * 8 + NPY_HEADER_BYTES > room:
            rows = np.sort(np.random.default_rng(0).choice(M, (room - 2 * NPY_HEADER_BYTES) // 16, replace=False))
            out["scores_index1" + suffix] = rows + 1
            scores = scores[rows]
        out["scores" + suffix] = scores
    return out


def experiment_outputs(g):
    """What one experiment of --workload default hands back: the nominee of every trial, the observations and responses, the
    hyper draws of every model-based trial, the best response."""
    return {"nominees": g["nominees"], "X": g["X"], "Y": g["Y"], "hyper_draws": np.concatenate(g["draws"], axis=0),
            "best_y": [g["best"]["y"]]}


def run_default(args, ctx=None, emit=True, cpu_seconds=None):
    """bench.py --workload default: the reference's own default experiment as a whole trial loop (harness/default_regime.py):
    hartmann6, d = 6, 2e4 Sobol candidates, budget 100 (N <= 100), nInitial 2, nSamples 10 slice-sampled hyper vectors per
    nomination, EI.  One step = one experiment; `value` = trials/s over the whole experiments (objective evaluations, a closed
    form, included).  cpu_baseline = the oracle driving the SAME loop (same host code, seeds and random streams) on the host
    cores: its nominee sequence is the parity check of the GPU run.  One GPU only (the regime is latency-bound; sharding
    2e4 candidates is exercised by the tests, not timed here).  The per-kernel figures and the cpu_baseline leg run with --full."""
    import bot7_amd
    from harness import default_regime as dr
    d, N, M, obj_name, score = WORKLOADS["default"]
    own_ctx = ctx is None
    if own_ctx:
        ctx = bot7_amd.Context(int(os.environ.get("LOCAL_RANK", "0")))
    info = ctx.device_info()
    budget = int(os.environ.get("B7_DEFAULT_BUDGET", "100"))
    for _ in range(args.warmup):
        dr.run(ctx, trials=min(budget, 40), budget=budget)
    runs = []
    gc.collect()
    gc.disable()
    try:
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            runs.append(dr.run(ctx, budget=budget))
        ctx.sync()
        elapsed = time.perf_counter() - t0
    finally:
        gc.enable()
    for r in runs[1:]:
        assert r["nominees"] == runs[0]["nominees"], "two identical experiments nominated different candidates"
    g = runs[-1]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, experiment_outputs(g))
    per_trial = [dict(r) for r in g["per_trial"]]
    for k in ("sampler_ms", "nominate_ms", "commit_ms", "trial_ms"):   # the mean over the timed experiments, trial by trial
        for i, r in enumerate(per_trial):
            r[k] = float(np.mean([run["per_trial"][i][k] for run in runs]))
    split = dr.summarise(per_trial)
    line = {
        "metric": "BO trials/sec at the reference's default regime (hartmann6 d=6, 2e4 Sobol candidates, nSamples=10, budget %d)" % budget,
        "value": args.steps * budget / elapsed, "unit": "trials/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "default: the reference's own default experiment (examples/run_benchmark.lua:30-36, "
                               "bots/abstract.lua:63-67,79-80): hartmann6 d=6, %d Sobol candidates, budget %d (N <= %d), nInitial 2, "
                               "nSamples 10 (slice sampler on the host, every density evaluation one b7_gp_nll_batch call), EI; a step = "
                               "one experiment = %d trials of sample_hypers + b7_eval_nominate + b7_nominate_commit"
                               % (M, budget, budget, budget),
                   "d": d, "budget": budget, "candidates": M, "nSamples": 10, "score": "ei",
                   "parallelism": "one GPU, one context (the regime is latency-bound)", "device": info["name"]},
        "ms_per_trial": split,
        "best": g["best"], "nominees_first_10": g["nominees"][:10],
    }
    if args.full:
        line.update(default_kernel_figures(ctx, g, split))
    if args.full and not args.no_cpu_baseline:
        from oracle.hostctx import OracleContext
        cores = usable_cores()
        try:
            from threadpoolctl import threadpool_limits
            limiter = threadpool_limits(limits=cores)
        except Exception:
            limiter = None
        cap_s = float(cpu_seconds if cpu_seconds is not None else os.environ.get("B7_DEFAULT_CPU_SECONDS", "40"))
        t0 = time.perf_counter()
        stop = {"n": 0}

        class _Stop(Exception):
            pass

        def on_trial(rec):
            stop["n"] += 1
            if time.perf_counter() - t0 > cap_s:
                raise _Stop()
        cpu = {}
        try:
            dr.run(OracleContext(), budget=budget, on_trial=on_trial, out=cpu)
        except _Stop:
            pass
        t_cpu = time.perf_counter() - t0
        if limiter is not None and hasattr(limiter, "unregister"):
            limiter.unregister()
        cpu_recs = cpu["per_trial"]
        n_cpu = len(cpu_recs)
        cpu["nominees"] = cpu["nominees"][:n_cpu]
        # parity: the nominee of every trial the oracle got through (the loop is deterministic given the densities; the slice
        # sampler is continuous in them away from accept / reject ties)
        same, worst = dr.agreement(g, cpu)
        cpu_split = dr.summarise(cpu_recs)
        # crossover: the first N from which the GPU's trial is faster than the CPU's for good
        cross = None
        for i in range(min(n_cpu, len(per_trial)) - 1, -1, -1):
            if per_trial[i]["nll_calls"] and per_trial[i]["trial_ms"] >= cpu_recs[i]["trial_ms"]:
                break
            if per_trial[i]["nll_calls"]:
                cross = per_trial[i]["N"]
        line["cpu_baseline"] = {"value": n_cpu / t_cpu, "unit": "trials/s", "cores": cores, "kind": "port",
                                "sample": "the same experiment driven through the oracle (numpy/scipy OpenBLAS+LAPACK restatement; not Torch7): "
                                          "%d of %d trials in %.1f s" % (n_cpu, budget, t_cpu),
                                "ms_per_trial": cpu_split, "trials": n_cpu}
        line["parity"] = {"trials_compared": n_cpu,
                          "leading_trials_with_the_same_nominee": same, "max_rel_diff_of_hyper_draws": worst,
                          "gpu_faster_per_trial_from_N": cross,
                          "note": "oracle: GP algebra parity unpinned (no reference fixture; DESIGN.md section 2)"}
        if same < min(n_cpu, len(g["nominees"])):
            line["parity"]["failed_at_trial"] = same + 1
            if emit:
                print(json.dumps(line))
                sys.exit("default regime: the GPU's nominee sequence leaves the oracle-driven loop at trial %d" % (same + 1))
    else:
        line["cpu_baseline"] = None
    if emit:
        print(json.dumps(line))
        sys.stdout.flush()
    if own_ctx:
        ctx.close()
    return line


def default_kernel_figures(ctx, g, split):
    """bench.py --workload default --full: kernel durations of the regime, HIP events on the context's stream (the phase timers of the
    library): the likelihood kernel (one launch per density evaluation: what a trial is made of) and the nomination's kernels at
    the last trial's N, each against its roofline.  Runs of their own after the timed experiments."""
    d, M = WORKLOADS["default"][0], WORKLOADS["default"][2]
    Xo, Yo = g["X"], g["Y"]
    hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": float(np.var(Yo)), "noise": 1e-4 * float(np.var(Yo)), "mean": float(np.mean(Yo))}
    ctx.grid_sobol(M, d, 1, download=False)
    kern = {}
    for n_obs in sorted({min(25, len(Xo)), min(64, len(Xo)), len(Xo)}):
        ctx.gp_set_data(Xo[:n_obs], Yo[:n_obs])
        for _ in range(5):
            ctx.gp_nll_batch(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        t0 = time.perf_counter()
        reps = 200
        for _ in range(reps):
            ctx.gp_nll_batch(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        call_us = (time.perf_counter() - t0) / reps * 1e6
        ctx.profile_enable(True)
        ctx.profile_reset()
        for _ in range(50):
            ctx.gp_nll_batch(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
        nll_ms, nll_n = ctx.profile_get("potrf")
        ctx.profile_reset()
        hyps = [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.05 * s_i)) for s_i in range(10)]
        spec = {"score": "ei", "fmin": [float(Yo[:n_obs].min())], "tradeoff": 0.0}
        for _ in range(20):
            ctx.eval_nominate(hyps, **spec)
        ph = {}
        for name in ("prep", "kxx", "potrf", "alpha", "ksx", "post", "kpost", "score", "argmax"):
            ms, cnt = ctx.profile_get(name)
            if cnt:
                ph[name] = round(ms / 20 * 1e3, 2)     # us per nomination
        ctx.profile_enable(False)
        ctx.profile_reset()
        for _ in range(5):
            ctx.eval_nominate(hyps, **spec)
        t0 = time.perf_counter()
        for _ in range(100):
            ctx.eval_nominate(hyps, **spec)
        nom_us = (time.perf_counter() - t0) / 100 * 1e6
        kern[str(n_obs)] = {"nll_call_us": round(call_us, 2), "nll_kernel_us": round(nll_ms / max(1, nll_n) * 1e3, 2),
                            "nominate_call_us": round(nom_us, 1), "nominate_phase_us": ph}
    n_last = str(len(Xo))
    # roofline of the kernel a trial spends most of its time in -- the one-workgroup likelihood (K + Cholesky + solve of one
    # hyper vector): algorithmic flops N^3/3 (factor) + N^2 (2 d + 1) (K, solve) against the fp64-MFMA peak.  It is a dependent
    # chain on ONE CU: the fraction says how far a latency-bound kernel is from a throughput roofline, nothing more.
    nn = float(len(Xo))
    nll_flops = nn ** 3 / 3.0 + nn * nn * (2.0 * d + 1.0)
    nll_t = kern[n_last]["nll_kernel_us"] * 1e-6
    post_us = kern[n_last]["nominate_phase_us"].get("kpost") or kern[n_last]["nominate_phase_us"].get("post")
    post_flops = 10.0 * M * nn * nn
    nt = -(-len(Xo) // 16)
    chain_us = nt * 3925 / GPU_CLOCK_HZ * 1e6
    dpad = 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32
    strip_cycles = 64.0 * (nt * max(1, dpad // 4) + 2 * nt * (nt + 1)) + 64 * nt * 4.8
    pipe_us = 10 * -(-M // 16) * strip_cycles / (1024 * GPU_CLOCK_HZ) * 1e6
    return {
        "kernels_by_N": kern,
        "roofline": {"bound": "dependent chain",
                     "kernel": "gp_small_kernel<0> (one density evaluation of the slice sampler: K + Cholesky + solve in one "
                               "workgroup; ~%d launches per trial)" % round(split.get("nll_calls", 0) / max(1, split.get("model_based_trials", 1))),
                     "floor_us": chain_us, "frac_of_floor": chain_us * 1e-6 / nll_t if nll_t > 0 else None,
                     "achieved": nll_flops / nll_t / 1e12 if nll_t > 0 else None, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": nll_flops / nll_t / 1e12 / FP64_MFMA_PEAK_TFLOPS if nll_t > 0 else None, "traffic": None,
                     "flops_per_launch": nll_flops, "avg_launch_ms": nll_t * 1e3,
                     "note": "one workgroup on one CU; floor_us = the ceil(N/16) pivot chains of the two 64-column factor routines alone "
                             "(3 925 cycles per 16 columns: sixteen dependent {rsqrt, scale, rank-1} steps on one wave; stamps in "
                             "profiles/r04_gp_small_stamps.txt); frac against the MFMA peak is tiny by construction and kept only "
                             "because the contract asks for it"},
        "roofline_nominate": {"bound": "fp64 pipe (MFMA+VALU)",
                              "kernel": "kpost_small_kernel (K*, mean and variance of the S = 10 fits over the grid at N = %s, K* never stored)" % n_last,
                              "achieved": post_flops / (post_us * 1e-6) / 1e12 if post_us else None, "peak": FP64_MFMA_PEAK_TFLOPS,
                              "unit": "TFLOP/s", "frac": post_flops / (post_us * 1e-6) / 1e12 / FP64_MFMA_PEAK_TFLOPS if post_us else None,
                              "pipe_us": pipe_us, "frac_of_pipe": pipe_us / post_us if post_us else None,
                              "traffic": None, "flops_per_launch": post_flops, "avg_launch_ms": post_us * 1e-3 if post_us else None,
                              "note": "pipe_us = what the one fp64 pipe per SIMD needs for the kernel's instructions: per 16-candidate "
                                      "strip NT dpad/4 + 2 NT (NT + 1) MFMAs of 64 cycles (NT = ceil(N/16): distances, then the lower "
                                      "triangle of L^-1 against the K* tile) and 64 NT exponential instructions of 4.8 cycles, over "
                                      "1 024 SIMDs at 2.4 GHz; avg_launch_ms is the library's phase timer (events around the launch)"},
    }


def run_group(args):
    """python bench.py --gpus N with no launcher: ONE process drives N GPUs (b7_group_*), the layout the reference itself has
    (one LuaJIT process, bots/abstract.lua:155-169).  Candidates are sharded over the members by contiguous row ranges, the fit
    is replicated, every member's work is enqueued without a host wait in between, and the winners are combined by ONE grouped
    ncclAllReduce (ncclCommInitAll) when the devices are distinct.  Weak scaling: --candidates rows per GPU.  The K steps are timed
    twice with or without --full (member 0's phase events on, then off): with virtual ranks `value` comes from the second pass."""
    import bot7_amd
    from harness import benchmarks
    d, N, M_default, obj_name, score = WORKLOADS[args.workload]
    if obj_name == "dngo":
        sys.exit("bench.py: the single-process group has no DNGO branch; launch cfg5 with torch.distributed.run (--layout ranks)")
    G = args.gpus
    M = args.candidates or M_default
    M_total = M * G
    import torch
    ndev = torch.cuda.device_count()
    if ndev >= G and not args.virtual_ranks:
        devices = list(range(G))
    elif args.virtual_ranks:
        devices = [0] * G
    else:
        # fewer devices than ranks and no launcher: do not exit -- the group runs with its members sharing device 0 (a rehearsal:
        # they time-share the GPU, so the value is one device's), and the line says so in config.parallelism / config.devices
        sys.stderr.write("bench.py --gpus %d: %d device(s) visible -- running the single-process group as %d VIRTUAL ranks on device 0\n"
                         % (G, ndev, G))
        devices = [0] * G
    lib = "diag" if os.environ.get("B7_GROUP_EXCHANGE") == "rccl" else None   # forcing the grouped call for virtual ranks: diagnostic build
    g = bot7_amd.Group(devices, lib=lib)
    ginfo = g.info()
    if args.workspace_mib:
        g.set_workspace(args.workspace_mib << 20)
    # inputs: the pool on the group, the observation rows deleted from the union; observations via a scratch context
    s_ = (M_total + N) // N
    tmp = bot7_amd.Context(devices[0], lib=lib)
    gen1 = (lambda first: tmp.grid_sobol(1, d, SOBOL_SKIP + first)) if d < 40 else (lambda first: tmp.grid_random(1, d, seed=1, row_offset=first))
    X_obs = np.concatenate([gen1(k * s_) for k in range(N)], axis=0)
    tmp.close()
    if d < 40:
        g.grid_sobol(M_total + N, d, SOBOL_SKIP)
    else:
        g.grid_random(M_total + N, d, seed=1)
    g.grid_remove_rows([k * s_ + 1 for k in range(N)], want_rows=False)
    assert g.grid_shape()[0] == M_total
    Y = benchmarks.registry[obj_name](X_obs)
    amp = float(np.var(Y))
    hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(Y))}
    g.gp_set_data(X_obs, Y)
    spec = {"score": "ei", "fmin": [float(Y.min())], "tradeoff": 0.0} if score == "ei" else {"score": "cb"}
    hyps = [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.05 * s_i)) for s_i in range(args.samples)]

    def fence():
        for m in g.members:
            m.sync()
        torch.cuda.synchronize()

    def timed(steps):
        gc.collect()
        gc.disable()
        try:
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                b = g.eval_nominate(hyps, **spec)
            fence()
            return time.perf_counter() - t0, b
        finally:
            gc.enable()

    for _ in range(args.warmup):
        g.eval_nominate(hyps, **spec)
    m0 = g.members[0]
    m0.profile_enable(True)
    m0.profile_reset()
    elapsed, best = timed(args.steps)
    m0.profile_enable(False)
    if args.dump_outputs:   # what b7_group_eval_nominate hands back: the winner
        dump_outputs(args.dump_outputs, {"best_value": [best[0]], "best_index1": [best[1]]})
    elapsed_plain, best_plain = timed(args.steps)
    assert best_plain == best
    shared = len(set(devices)) < G
    if shared:
        # virtual ranks time-share ONE device: member 0's phase events then wait across the other members' kernels (its "ksx"
        # phase reads 100 ms) and the pass with events on is no measure of anything -- the line's value is the plain pass
        elapsed, elapsed_events = elapsed_plain, elapsed
    phases = {}
    for ph in ("prep", "kxx", "potrf", "trtri", "alpha", "ksx", "post", "kpost", "score", "argmax", "exchange"):
        ms, n = m0.profile_get(ph)
        if n:
            phases[ph] = {"ms_total": round(ms, 4), "launches": n, "ms_avg": round(ms / n, 5)}
    post = phases.get("post") or phases.get("kpost") or {"ms_total": 0.0, "launches": 0}
    M0 = g.grid_shape()[2][1] - g.grid_shape()[2][0]          # member 0's rows
    lps = max(1, post["launches"] // max(1, args.steps))
    rows_per_launch = M0 * args.samples / lps
    flops = rows_per_launch * float(N) * float(N)
    t_post = post["ms_total"] / post["launches"] * 1e-3 if post["launches"] else float("nan")
    achieved = flops / t_post / 1e12 if post["launches"] else float("nan")
    line = {
        "metric": "EI candidates scored/sec at N=2048,d=32" if args.workload == "metric" else "%s candidates scored/sec (%s)" % (score.upper(), args.workload),
        "value": args.steps * M_total * args.samples / elapsed, "hyper_samples_per_step": args.samples, "unit": "candidates/s",
        "n_gpus": G, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "ms_per_step_without_phase_events": elapsed_plain / args.steps * 1e3,
        "ms_per_step_with_phase_events_on_member0": (elapsed_events if shared else elapsed) / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "config": {"workload": "%s: %s d=%d, N=%d obs (strided pick from the pool, SURVEY 8d), %d candidates per GPU (%d total), %s, %d hyper "
                               "sample(s) per step = fit + K(X*,X) + posterior mean/var + score:add per member, score:div + arg-max + ONE exchange"
                               % (args.workload, obj_name, d, N, M, M_total, score.upper(), args.samples),
                   "d": d, "n_obs": N, "candidates_per_gpu": M, "candidates_total": M_total, "score": score,
                   "parallelism": "single-process group x%d (b7_group_*: one host process drives every GPU, the reference's own layout); candidate-sharded, "
                                  "fit replicated, one exchange per nomination: %s"
                                  % (G, ("grouped ncclAllReduce (ncclCommInitAll over %d %s)" % (G, "distinct devices" if len(set(devices)) == G else
                                                                                                    "VIRTUAL ranks on one device through the test double"))
                                     if ginfo["uses_rccl"] else "records merged on the host (members share a device: RCCL refuses that)"),
                   "layout": "group", "devices": devices, "rccl_ranks": G if ginfo["uses_rccl"] else 0,
                   "device": m0.device_info()["name"]},
        "roofline": {"bound": "mfma", "kernel": "posterior variance kernel of member 0", "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS,
                     "unit": "TFLOP/s", "frac": achieved / FP64_MFMA_PEAK_TFLOPS if achieved == achieved else None, "traffic": None,
                     "flops_per_launch": flops, "avg_launch_ms": t_post * 1e3},
        "phases_member0": phases, "best": {"value": best[0], "index1": best[1]},
        "step_api": "b7_group_eval_nominate (one call per step; one host wait per member)",
        "cpu_baseline": None,
    }
    print(json.dumps(line))
    sys.stdout.flush()
    g.close()


def main():
    args = parse()
    no_launcher = "RANK" not in os.environ
    if args.workload != "default" and args.gpus > 1 and (args.layout == "group" or (args.layout == "auto" and no_launcher)):
        return run_group(args)
    if args.workload == "default":
        if args.gpus != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1:
            sys.exit("bench.py --workload default runs on one GPU (a latency-bound trial loop)")
        return run_default(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:   # --layout ranks without a launcher
            sys.exit("bench.py --gpus %d --layout ranks must be launched with torch.distributed.run (one process per GPU); "
                     "without a launcher the default is the single-process group" % args.gpus)
        args.gpus = world
    rccl = args.backend in ("rccl", "nccl")

    import torch
    import torch.distributed as td
    if not rccl or os.environ.get("B7_RCCL_LIB"):
        # ranks may share a GPU only in the rehearsals: the gloo exchange, or the tests' shared-memory double for RCCL's
        # transport (tests/stub; the real RCCL refuses two ranks on one device)
        local_rank = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local_rank)
    grouped = "RANK" in os.environ  # launched by torch.distributed.run: join the group even when it has one rank

    class quiet_stdout(object):
        """gloo and RCCL print banners on stdout when a group / communicator comes up: keep stdout for the one JSON
        line by pointing fd 1 at stderr meanwhile."""

        def __enter__(self):
            sys.stdout.flush()
            self.saved = os.dup(1)
            os.dup2(2, 1)

        def __exit__(self, *exc):
            sys.stdout.flush()
            os.dup2(self.saved, 1)
            os.close(self.saved)

    if grouped:
        # control plane only (rendezvous, the id hand-over, the barrier of the timing contract): a gloo group on the
        # CPU.  Every byte of the data path's one exchange goes through the C ABI.
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        with quiet_stdout():
            td.init_process_group("gloo", rank=rank, world_size=world)
            td.barrier()

    import bot7_amd
    from bot7_amd import _lib
    from harness import benchmarks, dist

    ctx = bot7_amd.Context(local_rank)
    info = ctx.device_info()
    if args.workspace_mib:
        ctx.set_workspace(args.workspace_mib << 20)
    if grouped and rccl:
        with quiet_stdout():
            box = [_lib.comm_unique_id() if rank == 0 else None]
            td.broadcast_object_list(box, src=0)
            ctx.comm_init(rank, world, box[0])
            ctx.comm_allreduce([0.0])          # first collective: brings the rings up before anything is timed

    def measure(args):
        """One workload on this rank's context: the JSON line as a dict (rank 0 prints it)."""
        d, N, M_default, obj_name, score = WORKLOADS[args.workload]
        M = args.candidates or M_default
        M_total = M * world
        # ---- inputs, resident in HBM before the timed region
        shard = dist.ShardedScorer(ctx, M_total, rank, world)
        X_obs = make_inputs(ctx, d, N, M_total, shard.lo, shard.hi)
        if obj_name == "dngo":
            # config 5: a fixed "trained" 3 x 50 tanh basis; responses that ARE a Bayesian linear model in those
            # features (what DNGO assumes after training), noise sd 0.1: the head then fits, the posterior mean moves
            # over the grid and EI at the winners is O(1e-1), not the underflow a featureless target would give
            rng = np.random.default_rng(0)
            dims = [d, 50, 50, 50]
            Wn = [rng.normal(scale=1.0 / np.sqrt(dims[i]), size=(dims[i + 1], dims[i])) for i in range(3)]
            bn = [rng.normal(scale=0.1, size=dims[i + 1]) for i in range(3)]
            Z0 = ctx.blr_basis(Wn, bn, "Tanh", X=X_obs)
            Y = (Z0 @ rng.normal(size=(50, 1)) + 0.1 * rng.normal(size=(N, 1)))
            alpha_p, beta, ymean = 1.0, 100.0, float(np.mean(Y))
            hyp = None
        else:
            Y = benchmarks.registry[obj_name](X_obs)
            amp = float(np.var(Y))
            hyp = {"lenscale_sq": np.full(d, d / 8.0), "amp": amp, "noise": 1e-4 * amp, "mean": float(np.mean(Y))}
            ctx.gp_set_data(X_obs, Y)              # the data go up once; a step uploads hypers only
        fmin = [float(Y.min())]

        def score_add():
            ctx.score_ei(fmin, 0.0) if score == "ei" else ctx.score_cb()

        spec = {"score": "ei", "fmin": fmin, "tradeoff": 0.0} if score == "ei" else {"score": "cb"}

        def hyper_samples(samples):               # distinct hypers per sample, as a sampler would hand over
            return [dict(hyp, lenscale_sq=hyp["lenscale_sq"] * (1.0 + 0.05 * s_i)) for s_i in range(samples)]

        def step(samples):
            if obj_name == "dngo":
                if ctx.comm_info()[1] == world:
                    # bots/bayesopt.lua:65-66 + :96 over models/dngo.lua:155-175 as ONE call: features of the observations,
                    # the Bayesian linear head, features of every candidate (recomputed each step, as the reference does),
                    # mean / variance, EI, the (global) arg-max
                    if samples > 1:   # models/dngo.lua:109 'marginalize': S heads over the same features, one call
                        al = alpha_p * (1.0 + 0.1 * np.arange(samples))
                        be = beta * (1.0 + 0.05 * np.arange(samples))
                        return ctx.blr_eval_nominate_marg(Wn, bn, "Tanh", X_obs, Y, al, be, np.full(samples, ymean), score="ei", fmin=fmin,
                                                          global_row_offset=shard.lo)[:2]
                    return ctx.blr_eval_nominate(Wn, bn, "Tanh", X_obs, Y, alpha_p, beta, ymean, score="ei", fmin=fmin,
                                                 global_row_offset=shard.lo)
                ctx.blr_fit_x(Wn, bn, "Tanh", X_obs, Y, alpha_p, beta, ymean)
                ctx.blr_basis(Wn, bn, "Tanh")
                ctx.blr_predict(download=False)
                ctx.score_reset()
                score_add()
                return shard.nominate(1.0, device=None if rccl else "cpu")
            # bots/bayesopt.lua:56-99: per hyper sample one fit + posterior + score:add, then score:div and score:max(1)
            # across all ranks -- b7_eval_nominate, one library call
            return shard.eval_nominate(hyper_samples(samples), spec, device=None if rccl else "cpu")

        def fence():
            ctx.sync()
            torch.cuda.synchronize()
            if grouped:
                td.barrier()
                torch.cuda.synchronize()

        def timed(steps, samples):
            # the interpreter's cyclic garbage collector stays out of the timed region: with torch imported a full collection
            # takes ~40 ms, which is 70 steps of cfg5 (seen as one slow pass in every few runs of 20 steps)
            gc.collect()
            gc.disable()
            try:
                fence()
                t0 = time.perf_counter()
                for _ in range(steps):
                    b = step(samples)
                fence()
                el = time.perf_counter() - t0
            finally:
                gc.enable()
            if grouped:
                t = torch.tensor([el], dtype=torch.float64)
                td.all_reduce(t, op=td.ReduceOp.MAX)
                el = float(t.item())
            return el, b

        for _ in range(args.warmup):
            best = step(args.samples)
        ctx.profile_enable(True)   # HIP events around every kernel phase, on the stream the kernels run on
        ctx.profile_reset()
        elapsed, best = timed(args.steps, args.samples)
        ctx.profile_enable(False)
        if args.dump_outputs:
            share = DUMP_LIMIT_BYTES // world      # every rank writes its own files into the same directory
            dump_outputs(args.dump_outputs, nomination_outputs(ctx, best, "" if world == 1 else "_rank%d" % rank, share), share)
        elapsed_plain = None
        if args.full:
            # the same K steps once more without the per-phase HIP events: at the small configurations the event records
            # themselves (two per phase, ~16 per step) are a third of the step; at the headline size they are 0.1 %
            elapsed_plain, best_plain = timed(args.steps, args.samples)
            assert best_plain == best, "the nomination changed between two identical passes"

        phases = {}
        for ph in ("prep", "kxx", "potrf", "trtri", "alpha", "basis", "mean", "ksx", "post", "kpost", "score", "argmax", "exchange"):
            ms, n = ctx.profile_get(ph)
            if n:
                phases[ph] = {"ms_total": round(ms, 4), "launches": n, "ms_avg": round(ms / n, 5)}
        Npad = (N + 127) // 128 * 128
        post = phases.get("post") or phases.get("kpost") or {"ms_total": 0.0, "launches": 0}
        # dominant kernel: post_kernel.  Algorithmic flops per launch = rows_in_launch * Npad^2 (triangular L^-1
        # exploited: N^2/2 multiply-adds per candidate); rows per launch = M / launches-per-step.
        post_launches_per_step = max(1, post["launches"] // max(1, args.steps))
        n_samples = args.samples
        rows_per_launch = M * n_samples / post_launches_per_step
        n_eff = 128 if obj_name == "dngo" else N   # DNGO: the "observations" of the variance GEMM are the 50 -> 128 padded features
        flops_per_launch = rows_per_launch * float(n_eff) * float(n_eff)
        post_avg_s = (post["ms_total"] / post["launches"] * 1e-3) if post["launches"] else float("nan")
        achieved = flops_per_launch / post_avg_s / 1e12 if post["launches"] else float("nan")
        ksx = phases.get("ksx")
        ksx_gbs = None
        if ksx:
            ksx_gbs = rows_per_launch * (8.0 * Npad + 8.0 * d) / (ksx["ms_avg"] * 1e-3) / 1e9
        n_fits = max(1, args.steps * n_samples)
        fit_ms = sum(phases[p]["ms_total"] for p in ("prep", "kxx", "potrf", "trtri", "alpha") if p in phases) / n_fits
        traffic, traffic_src = pmc_traffic(rows_per_launch, N)
        potrf = phases.get("potrf")
        roofline_fit = roofline_ksx = None
        if potrf and obj_name != "dngo":
            # Cholesky + explicit inverse of the factor: N^3/3 flop each (the trailing updates alone: N^3/3)
            chol_flops = 2.0 * float(N) ** 3 / 3.0
            t_s = potrf["ms_avg"] * 1e-3
            # what bounds ONE factorisation is not the pipe but the chain of things that wait for each other: per 64-column panel
            # the four 16-column pivot chains of the factor routine (3 925 cycles each: 16 x {rsqrt, scale, rank-1} on one wave),
            # its four in-block updates (720), the next block row's solve (1.55 us) and the update of the next diagonal block
            # (0.80 us) -- stamps read inside the launch, profiles/r04_persist_stamps_N2048.txt; DESIGN section 8, "The
            # factorisation's floor".  Publishing / storing the inverse, the grid-wide flag and the tail of the inverse's doubling
            # are the schedule's own overhead and are NOT in the floor.
            panels = Npad // 64
            floor_ms = panels * ((4 * 3925 + 4 * 720) / GPU_CLOCK_HZ * 1e3 + 1.55e-3 + 0.80e-3)
            roofline_fit = {"bound": "dependent chain", "kernel": "potrf_persist_kernel (blocked Cholesky + inverse of the factor, one persistent launch)",
                            "floor_ms": floor_ms, "frac_of_floor": floor_ms / potrf["ms_avg"], "panels": panels,
                            "achieved": chol_flops / t_s / 1e12, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                            "frac": chol_flops / t_s / 1e12 / FP64_MFMA_PEAK_TFLOPS, "traffic": None,
                            "flops_per_launch": chol_flops, "avg_launch_ms": potrf["ms_avg"],
                            "trailing_update_frac": 0.5 * chol_flops / t_s / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                            "note": "one fit is a chain of Npad/64 panels on one CU with the rest of the chip pulling tile jobs: floor_ms is "
                                    "that chain at the measured cost of its links, frac / peak (the fp64-MFMA pipe) are kept for "
                                    "reference only; MFMA-busy and utilisation of the side-by-side shapes (ten fits, sixteen "
                                    "likelihoods: 38 %) in profiles/r03_potrf_pmc.json"}
        if ksx:
            ksx_bytes = rows_per_launch * (8.0 * Npad + 8.0 * d)
            # what actually bounds the kernel: the ONE fp64 pipe per SIMD that MFMA and VALU instructions share.  Per 64 outputs a
            # wave issues dpad/16 v_mfma_f64_16x16x4 (64 cycles each) and the epilogue's VALU instructions (4.8 cycles each;
            # counts per width class from the committed PMC passes, profiles/r03_ksx_pmc_by_class.json -- the kernel is unchanged
            # since); pipe time = outputs / 64 x those cycles / (1024 SIMDs x 2.4 GHz)
            dpad = 4 if d <= 4 else 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 48 if d <= 48 else 64 if d <= 64 else 96
            valu64, src = 25.6, None
            try:
                with open(os.path.join(ROOT, "profiles", KSX_PMC_BY_CLASS)) as f:
                    cls = json.load(f)["classes"].get("DPAD%d" % dpad)
                if cls:
                    valu64, src = float(cls["valu_wave_instructions_per_64_outputs"]), "profiles/" + KSX_PMC_BY_CLASS
            except Exception:
                pass
            pipe_cycles = (dpad / 16.0) * 64.0 + valu64 * 4.8
            pipe_s = rows_per_launch * Npad / 64.0 * pipe_cycles / (1024 * 2.4e9)
            roofline_ksx = {"bound": "fp64 pipe (MFMA + VALU share one issue pipe per SIMD)",
                            "kernel": "ksx_kernel (K(X*,X) assembly + fused posterior mean)",
                            "achieved": ksx_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ksx_gbs / HBM_PEAK_GBS,
                            "frac_of_pipe": pipe_s / (ksx["ms_avg"] * 1e-3),
                            "hbm_frac_ceiling_at_this_d": (ksx_bytes / pipe_s / 1e9) / HBM_PEAK_GBS,
                            "pipe_cycles_per_64_outputs": {"mfma": dpad / 16.0, "valu": valu64, "cycles": pipe_cycles, "source": src or
                                                           "DPAD32's count (no PMC pass for this width class)"},
                            "traffic": None, "algorithmic_bytes_per_launch": ksx_bytes, "avg_launch_ms": ksx["ms_avg"],
                            "note": "frac = algorithmic bytes / time / 8 TB/s (the north star's K(X*,X) number); frac_of_pipe = the share of "
                                    "the kernel's time that its own MFMA + VALU issue cycles account for: the kernel is bound by "
                                    "arithmetic issue, not by HBM, from d ~ 32 up"}

        if obj_name == "dngo":
            post_kernel_name = "post_small_kernel (variance of the Bayesian-linear head over the 64-padded features)"
        elif "kpost" in phases:
            post_kernel_name = "kpost_small_kernel (K(X*,X) + mean + variance in one kernel, K* never stored)"
        elif Npad % 256 == 0 and rows_per_launch / 256 >= 256:
            post_kernel_name = "post_kernel_w4t (posterior variance: L^-1 K*' with fused column sumsq; 256-row n-tiles)"
        else:
            post_kernel_name = "post_kernel_w4 (posterior variance: L^-1 K*' with fused column sumsq; 128-row n-tiles)"
        line = {
            "metric": "EI candidates scored/sec at N=2048,d=32" if args.workload == "metric"
                      else "%s candidates scored/sec (%s)" % (score.upper(), args.workload),
            "value": args.steps * M_total * n_samples / elapsed,   # candidate scorings per second
            "hyper_samples_per_step": n_samples,
            "unit": "candidates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "%s: %s d=%d, N=%d obs (strided pick from the pool, SURVEY 8d), %d %s candidates per "
                                   "GPU (%d total), %s, %d hyper sample%s per step = %s(fit + K(X*,X) + posterior "
                                   "mean/var + score:add) + score:div + arg-max%s"
                                   % (args.workload, obj_name, d, N, M, "Sobol" if d < 40 else "counter-based uniform",
                                      M_total, score.upper(), n_samples, "" if n_samples == 1 else "s",
                                      "" if n_samples == 1 else "%d x " % n_samples,
                                      " + RCCL exchange" if world > 1 else ""),
                       "d": d, "n_obs": N, "candidates_per_gpu": M, "candidates_total": M_total, "score": score,
                       "parallelism": "candidate-sharded x%d, fit replicated, one (value,index) exchange "
                                      "(b7_score_finish_global: %s)"
                                      % (world, "ncclAllReduce inside libbot7hip.so" if rccl else "gloo rehearsal"),
                       "device": info["name"]},
            "roofline": {"bound": "mfma", "kernel": post_kernel_name,
                         "achieved": achieved, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / FP64_MFMA_PEAK_TFLOPS if achieved == achieved else None,
                         "traffic": traffic,
                         "traffic_source": ("%s (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench at "
                                            "the same launch shape)" % traffic_src) if traffic_src else None,
                         "algorithmic_bytes_per_launch": rows_per_launch * N * 8.0,
                         "flops_per_launch": flops_per_launch, "avg_launch_ms": post_avg_s * 1e3,
                         "note": "fp64 v_mfma_f64_16x16x4 peak 78.6 TFLOP/s at 2.4 GHz; in-kernel clock under this load 2.29-2.38 GHz by device, "
                                 "MFMA issue efficiency 96 % (profiles/r02_post_clock.txt, tools/post_clock.py)"},
            # the metric's second half ("GP-fit ms") and the north-star's K(X*,X) target, each against its own roofline
            "roofline_fit": roofline_fit,
            "roofline_ksx": roofline_ksx,
            "gp_fit_ms": fit_ms,
            "ksx_hbm_gbs": ksx_gbs, "ksx_hbm_frac": (ksx_gbs / HBM_PEAK_GBS) if ksx_gbs else None,
            "phases": phases,
            "best": {"value": best[0], "index1": best[1]},
            "step_api": ("b7_blr_eval_nominate (one call, one host synchronisation per step)" if ctx.comm_info()[1] == world
                         else "b7_blr_* + b7_score_* per step, gloo exchange") if obj_name == "dngo" else
                        ("b7_eval_nominate (one call, one host synchronisation per step)" if ctx.comm_info()[1] == world
                         else "b7_gp_predict_hyp + b7_score_* per sample, gloo exchange"),
        }
        if elapsed_plain is not None:
            line["ms_per_step_without_phase_events"] = elapsed_plain / args.steps * 1e3

        extras = args.full and not args.no_extras and obj_name != "dngo"
        cpu_leg = args.full and not args.no_cpu_baseline
        # ---- the reference-faithful S = 10 marginalisation loop (bots/abstract.lua:67), beside the S = 1 headline
        if extras and args.samples == 1:
            S = 10
            step(S)
            el, b10 = timed(2, S)
            line["marginalised"] = {"samples": S, "steps": 2, "ms_per_nomination": el / 2 * 1e3,
                                    "candidate_scorings_per_s": 2 * M_total * S / el,
                                    "marginalised_candidates_per_s": 2 * M_total / el,
                                    "best": {"value": b10[0], "index1": b10[1]}}
        # ---- GP fit (K + Cholesky + L^-1 + alpha + NLL terms) at N = 256 / 1024 / 2048: what one slice-sampler density
        # evaluation costs (HIP-event time on the context's stream over 20 back-to-back fits, host gaps included)
        if extras and rank == 0:
            by_n = {}
            for nf in (256, 1024, 2048):
                if nf > N:
                    continue
                ctx.gp_set_data(X_obs[:nf], Y[:nf])
                ctx.gp_fit_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"], want_nll=True)
                ctx.sync()
                ctx.timer_start(0)
                for _ in range(20):
                    ctx.gp_fit_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"], want_nll=True)
                ctx.timer_stop(0)
                by_n[str(nf)] = round(ctx.timer_ms(0) / 20, 4)
            ctx.gp_set_data(X_obs, Y)
            line["gp_fit_ms_by_N"] = by_n
            # ---- SURVEY 8(d)'s second variant, timed only: noise = 0, so the plain attempt fails and utils/math.lua:174-202's
            # schedule runs -- eps from 1e-8, x 1.1 per retry, each retry a whole factorisation of K + eps I and a host look
            # at its report
            t0 = time.perf_counter()
            r0 = ctx.gp_fit_hyp(hyp["lenscale_sq"], hyp["amp"], 0.0, hyp["mean"], want_nll=True)
            ctx.sync()
            dt = time.perf_counter() - t0
            eps0, growth = 1e-8, 1.1
            retries = int(round(np.log(r0["jitter"] / eps0) / np.log(growth))) if r0["jitter"] > 0 else 0
            line["gp_fit_noiseless"] = {"ms": round(dt * 1e3, 3), "jitter_used": r0["jitter"], "first_failed_pivot": r0["info"],
                                        "retries": retries, "ms_per_attempt": round(dt * 1e3 / (retries + 1), 4),
                                        "note": "noise = 0 (config.noiseless): the jitter schedule of utils/math.lua:159-218, time only"}

        # ---- CPU baseline on a bounded sample, and the arg-max check against it.  The sample is the window of rows around the
        # GPU's GLOBAL winner, so the headline arg-max itself is what the oracle re-derives (the first rows of the
        # grid hold one dominant candidate and say nothing about the winner).
        if rank == 0 and world == 1 and cpu_leg and obj_name != "dngo":
            sample = min(args.cpu_sample, M)

            def window_of(idx1, rows):
                return int(min(max(0, idx1 - 1 - rows // 2), M - rows))

            w0 = window_of(best[1], sample)
            X_hid = ctx.grid_download(w0, sample)
            cb, s_cpu = cpu_baseline(d, N, score, X_obs, Y, hyp, X_hid, w0)
            # the GPU's scores for the same hypers over the same rows, arg-max over the same window
            ctx.gp_fit_hyp(hyp["lenscale_sq"], hyp["amp"], hyp["noise"], hyp["mean"])
            ctx.gp_predict(download=False)
            ctx.score_reset()
            score_add()
            _, _, s_gpu = ctx.score_finish(1.0, download=True)
            gv, gi = ctx.argmax(s_gpu[w0:w0 + sample])
            maxdiff = float(np.max(np.abs(s_gpu[w0:w0 + sample] - s_cpu)))
            line["best_in_cpu_sample"] = {"index1": int(gi), "value": float(gv), "window_offset": w0,
                                          "is_the_global_winner": int(gi) + w0 == int(best[1]) if args.samples == 1 else None,
                                          "matches_cpu_argmax": int(gi) == cb["argmax1"],
                                          "max_abs_score_diff_vs_cpu": maxdiff, "cpu_top2_gap": cb["top2_gap"]}
            line["cpu_baseline"] = cb
            bad = int(gi) != cb["argmax1"] and cb["top2_gap"] > 1e3 * maxdiff
            if args.samples == 1 and int(gi) + w0 != int(best[1]):
                bad = True
            # the S = 10 winner the same way, on a smaller window (ten fits + ten posteriors on the host)
            if "marginalised" in line:
                from oracle import cport, gp
                S, rows = line["marginalised"]["samples"], min(16384, M)
                i10 = line["marginalised"]["best"]["index1"]
                w10 = window_of(i10, rows)
                Xw = ctx.grid_download(w10, rows)
                acc = np.zeros(rows)
                for h in hyper_samples(S):
                    m_o, v_o = gp.predict(gp.fit(X_obs, Y, **h), Xw)
                    cport.accumulate(acc, cport.ei(m_o, v_o, fmin) if score == "ei" else cport.cb(m_o, v_o))
                cport.divide(acc, float(S))
                ci, cv = cport.argmax_first(acc)
                top2 = np.partition(acc, -2)[-2:]
                line["marginalised"]["cpu_check"] = {"window_offset": w10, "rows": rows, "cpu_argmax1": int(ci), "cpu_value": float(cv),
                                                     "is_the_global_winner": int(ci) + w10 == int(i10),
                                                     "abs_value_diff": abs(float(cv) - line["marginalised"]["best"]["value"]),
                                                     "cpu_top2_gap": float(top2[1] - top2[0])}
                if int(ci) + w10 != int(i10):
                    bad = True
            if bad:
                print(json.dumps(line))
                sys.exit("the oracle does not confirm the GPU's arg-max: S=1 window %r, S=10 %r"
                         % (line["best_in_cpu_sample"], line.get("marginalised", {}).get("cpu_check")))
        elif rank == 0 and world == 1 and cpu_leg and obj_name == "dngo":
            # config 5: the head and the acquisition re-derived by the oracle (oracle/blr.py: parity unpinned) on the window of rows
            # around the GPU's winner
            from oracle import blr, cport
            sample = min(args.cpu_sample, M)
            w0 = int(min(max(0, best[1] - 1 - sample // 2), M - sample))
            Xw = ctx.grid_download(w0, sample)
            t0 = time.perf_counter()
            fh = blr.fit(blr.basis(X_obs, Wn, bn, "Tanh"), Y, alpha_p, beta, ymean)
            m_o, v_o = blr.predict(fh, blr.basis(Xw, Wn, bn, "Tanh"))
            s_cpu = cport.ei(m_o, v_o, fmin)
            ci, cv = cport.argmax_first(s_cpu)
            t_cpu = time.perf_counter() - t0
            line["cpu_baseline"] = {"value": sample / t_cpu, "unit": "candidates/s", "cores": usable_cores(), "kind": "port",
                                    "sample": "DNGO head (N=%d, 50 features) + %d candidates (rows %d..%d around the GPU's winner) through "
                                              "oracle/blr.py in %.2f s" % (N, sample, w0 + 1, w0 + sample, t_cpu),
                                    "argmax1": int(ci), "best_value": float(cv)}
            line["best_in_cpu_sample"] = {"index1": int(best[1]) - w0, "window_offset": w0, "matches_cpu_argmax": int(ci) + w0 == int(best[1]),
                                          "is_the_global_winner": int(ci) + w0 == int(best[1]),
                                          "abs_value_diff": abs(float(cv) - float(best[0]))}
        elif rank == 0:
            line["cpu_baseline"] = None
        return line

    line = measure(args)
    # ---- the other BASELINE configurations, compactly, behind the headline (one GPU, the metric workload with --full): the same
    # measurement at few steps, a bounded oracle window around each winner
    if rank == 0 and world == 1 and args.workload == "metric" and args.full and not args.no_extras and not args.no_cpu_baseline:
        import copy
        line["configs"] = {}
        for name in ("cfg2", "cfg3", "cfg4", "cfg5"):
            a2 = copy.copy(args)
            a2.workload, a2.candidates, a2.steps, a2.warmup, a2.samples, a2.no_extras, a2.cpu_sample = name, 0, 5, 1, 1, True, 8192
            a2.dump_outputs = None
            if name in ("cfg2", "cfg5"):
                a2.steps, a2.warmup = 20, 3        # a quarter of a millisecond per step
            l2 = measure(a2)
            # the timed pass WITHOUT the per-phase HIP events (a third of a step at the small configurations); value follows it
            plain_ms = l2["ms_per_step_without_phase_events"]
            c = {"ms_per_step": round(plain_ms, 4), "ms_per_step_with_phase_events": round(l2["ms_per_step"], 4),
                 "value": l2["value"] * l2["ms_per_step"] / plain_ms, "unit": l2["unit"], "steps": a2.steps,
                 "workload": l2["config"]["workload"].split(":")[0], "n_obs": l2["config"]["n_obs"], "d": l2["config"]["d"],
                 "candidates": l2["config"]["candidates_per_gpu"], "best": l2["best"],
                 "dominant_kernel_frac": (l2["roofline"] or {}).get("frac"), "dominant_kernel": (l2["roofline"] or {}).get("kernel"),
                 "ksx": {k: (l2.get("roofline_ksx") or {}).get(k) for k in ("frac", "frac_of_pipe", "bound")} if l2.get("roofline_ksx") else None,
                 "gp_fit_ms": round(l2["gp_fit_ms"], 4) if l2.get("gp_fit_ms") else None}
            chk = l2.get("best_in_cpu_sample")
            if chk:
                c["winner_oracle_confirmed_on_window"] = bool(chk["matches_cpu_argmax"] and chk["is_the_global_winner"])
                c["window_rows"] = a2.cpu_sample
            line["configs"][name] = c
        # ---- and the reference's OWN default experiment (--workload default), compactly: one timed experiment of 100 trials, the
        # oracle behind the same driver for a few seconds (its first ~40 trials: the nominee sequence is the parity check)
        a3 = copy.copy(args)
        a3.steps, a3.warmup, a3.no_cpu_baseline, a3.dump_outputs = 1, 1, False, None
        with quiet_stdout():
            l3 = run_default(a3, ctx=ctx, emit=False, cpu_seconds=4.0)
        last = sorted(l3["kernels_by_N"], key=int)[-1]
        line["default_regime"] = {
            "workload": "python bench.py --workload default: hartmann6 d = 6, 20000 Sobol candidates, budget 100, nSamples 10, EI; a whole trial "
                        "loop (slice sampler on the host, b7_gp_nll_batch per density evaluation, b7_eval_nominate, b7_nominate_commit)",
            "value": l3["value"], "unit": l3["unit"], "ms_per_trial_at_N": {k: v["trial_ms"] for k, v in l3["ms_per_trial"]["at_N"].items()},
            "library_calls_per_experiment": l3["ms_per_trial"]["nll_calls"], "at_N_%s" % last: l3["kernels_by_N"][last],
            "likelihood_kernel_frac_of_chain_floor": l3["roofline"]["frac_of_floor"],
            "fused_posterior_frac_of_pipe": l3["roofline_nominate"]["frac_of_pipe"],
            "cpu_baseline": {k: l3["cpu_baseline"][k] for k in ("value", "unit", "cores", "kind", "trials")},
            "parity": l3["parity"]}
        if l3["parity"].get("failed_at_trial"):
            print(json.dumps(line))
            sys.exit("default regime: the GPU's nominee sequence leaves the oracle-driven loop at trial %d" % l3["parity"]["failed_at_trial"])
    if rank == 0:
        print(json.dumps(line))
    sys.stdout.flush()
    with quiet_stdout():   # nothing after the JSON line reaches stdout
        ctx.close()
        if grouped:
            td.barrier()
            td.destroy_process_group()


if __name__ == "__main__":
    main()
