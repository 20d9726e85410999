"""What the probit classifier costs (csrc/laplace.hip), measured on the GPU and gated by nothing:
  nll       per call of b7_clf_nll_batch (B = 1 and 10) at N = 25 / 64 / 100 / 128, d = 6, with the Newton iteration counts, and
            b7_gp_nll_batch on the same shapes beside it for scale (one Cholesky against a whole Newton solve);
  logfeas   clf_eval_logfeas at the default regime's shape (N = 100, d = 6, 2e4 candidates, S = 10) against the regression
            constraint's eval_nominate(score="logpi") on the same shape;
  parent    b7_eval_nominate and b7_gp_nll_batch of this tree against another built checkout of the project (--parent TREE: the
            parent commit's), in ALTERNATING child processes of this same script, each timing the same seeded inputs: the ratio of
            the medians beside the parent's own process-to-process spread.  This change touches none of their code.
Wall time per call around calls that end in a device synchronisation: median and min .. max over the rounds, after warm-up.
--make-parent DIR: check the parent commit out into DIR (git worktree) and build it with its own bot7_amd.build -- on the build
machine, before the GPU visit.  Prints one JSON object.
usage (GPU box): python tools/clf_cost.py [out.json] [--parent path/to/built/checkout]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--make-parent" in sys.argv:
    dst = os.path.abspath(sys.argv[sys.argv.index("--make-parent") + 1])
    subprocess.check_call(["git", "-C", HERE, "worktree", "add", "--detach", dst, "HEAD"])
    subprocess.check_call([sys.executable, "-m", "bot7_amd.build"], cwd=dst)
    sys.exit(0)
TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else HERE
sys.path.insert(0, os.path.abspath(TREE))
import bot7_amd  # noqa: E402


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


def problem(N, d, S, rng):
    X = rng.random((N, d))
    Y = np.sin(3.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    Cv = np.cos(2.0 * X[:, :3].sum(1, keepdims=True)) + 0.05 * rng.standard_normal((N, 1))
    labels = (Cv > 0.5).astype(np.float64)
    amp = float(np.var(Y))
    reg = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": amp, "noise": 1e-2 * amp, "mean": float(Y.mean())} for s in range(S)]
    clf = [{"lenscale_sq": np.full(d, d / 8.0 * (1 + 0.05 * s)), "amp": 4.0 + 0.5 * s, "noise": 0.0, "mean": -0.3 + 0.05 * s} for s in range(S)]
    return X, Y, Cv, labels, reg, clf


def shared_arm(c):
    """The two entry points this change does not touch, on seeded inputs: what both trees time in their child processes."""
    rng = np.random.default_rng(0)
    X, Y, _, _, reg, _ = problem(100, 6, 10, rng)
    c.grid_sobol(20000, 6, 1, download=False)
    c.gp_set_data(X, Y)
    fmin = [float(Y.min())]
    ls = np.stack([h["lenscale_sq"] for h in reg])
    amp, nz, mn = (np.array([h[k] for h in reg]) for k in ("amp", "noise", "mean"))
    return {"eval_nominate": timed(lambda: c.eval_nominate(reg, score="ei", fmin=fmin), 20, 300),
            "gp_nll_batch_B1": timed(lambda: c.gp_nll_batch(ls[:1], amp[:1], nz[:1], mn[:1]), 50, 1000),
            "gp_nll_batch_B10": timed(lambda: c.gp_nll_batch(ls, amp, nz, mn), 50, 1000)}


if "--shared-arm" in sys.argv:
    c = bot7_amd.Context(0)
    print(json.dumps(shared_arm(c)))
    c.close()
    sys.exit(0)

parent = sys.argv[sys.argv.index("--parent") + 1] if "--parent" in sys.argv else None
args = [a for a in sys.argv[1:] if not a.startswith("--") and a not in (parent, TREE)]
out = {"nll": {}, "logfeas": {}}
c = bot7_amd.Context(0)
rng = np.random.default_rng(0)
for N in (25, 64, 100, 128):
    X, Y, Cv, labels, reg, clf = problem(N, 6, 10, rng)
    ls = np.stack([h["lenscale_sq"] for h in reg])
    amp, nz, mn = (np.array([h[k] for h in reg]) for k in ("amp", "noise", "mean"))
    r = {}
    c.gp_set_data(X, labels)
    for B in (1, 10):
        _, iters, info = c.clf_nll_batch(clf[:B], want_info=True)
        r["clf_nll_batch_B%d" % B] = dict(timed(lambda: c.clf_nll_batch(clf[:B]), 20, 200), iters=[int(i) for i in iters], not_converged=int(info.sum()))
    c.gp_set_data(X, Y)
    for B in (1, 10):
        r["gp_nll_batch_B%d" % B] = timed(lambda: c.gp_nll_batch(ls[:B], amp[:B], nz[:B], mn[:B]), 20, 200)
        r["clf_over_gp_B%d" % B] = round(r["clf_nll_batch_B%d" % B]["median_ms"] / r["gp_nll_batch_B%d" % B]["median_ms"], 2)
    out["nll"]["N%d" % N] = r
X, Y, Cv, labels, reg, clf = problem(100, 6, 10, rng)
c.grid_sobol(20000, 6, 1, download=False)
c.gp_set_data(X, labels)
out["logfeas"]["shape"] = {"N": 100, "d": 6, "M": 20000, "S": 10}
out["logfeas"]["clf_eval_logfeas"] = timed(lambda: c.clf_eval_logfeas(clf), 10, 100)
out["logfeas"]["iters"] = [int(i) for i in c.clf_eval_logfeas(clf, want_report=True)[2]["iters"]]
c.gp_set_data(X, Cv)
out["logfeas"]["eval_nominate_logpi"] = timed(lambda: c.eval_nominate(reg, score="logpi", fmin=[0.5], tradeoff=0.0), 10, 100)
out["logfeas"]["clf_over_logpi"] = round(out["logfeas"]["clf_eval_logfeas"]["median_ms"] / out["logfeas"]["eval_nominate_logpi"]["median_ms"], 2)
c.close()
if parent:
    runs = {"this": [], "parent": []}
    for rep in range(4):                      # alternating processes: this, parent, this, parent, ...
        for who, tree in (("this", HERE), ("parent", parent)):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--shared-arm", "--tree", tree], capture_output=True, text=True, check=True)
            runs[who].append(json.loads(res.stdout.strip().splitlines()[-1]))
    cmp_ = {}
    for key in runs["this"][0]:
        mine = [r[key]["median_ms"] for r in runs["this"]]
        theirs = [r[key]["median_ms"] for r in runs["parent"]]
        cmp_[key] = {"this_medians_ms": mine, "parent_medians_ms": theirs, "ratio_of_medians": round(float(np.median(mine) / np.median(theirs)), 4),
                     "parent_spread_max_over_min": round(max(theirs) / min(theirs), 4), "this_spread_max_over_min": round(max(mine) / min(mine), 4)}
    out["parent"] = cmp_
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
