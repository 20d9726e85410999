"""The bits of everything made by the three kernels that walk the observations in slabs past 64 query rows -- ksx_kernel
(covar.hip), believer_kernel (batch.hip), kg_kernel (kg.hip) -- as one SHA-256 per case, through the shipped library's entry
points only.  tests/test_gpu_cov_walk_bits.py recomputes them and compares with tests/golden/cov_walk_bits.json.

Cases: d in {3, 6, 12, 24, 40, 60, 96} (one per dpad class) x {ardse, ardmatern52}, M = 200 candidates (three full query blocks
and one with 8 live rows: the clamp), S = 2 hyper samples, N in {24, 100, 150} (Npad 64, 128, 256: 1/2, 2/4 and 4/8 slabs of the
64/32-row classes -- no prefetch, one flip, several).
  ksx       (N = 150; below that the one-launch kernels serve) gp_fit + gp_download's L and alpha (K(X,X), blockIdx.y split),
            gp_predict's mean and variance (fused mean), eval_nominate's S = 2 accumulator (launch_ksx_batch)
  believer  eval_nominate_batch(q = 3): values, indices, the accumulator
  kg        kg_nominate(points = 5, trace) + kg_last(slopes): rows, alpha, slopes, values
Every case requires a fit report without jitter.  The inputs are made of exact float64 operations only (no generator, no libm).

usage (GPU box; BOT7HIP_LIB selects another build of the library):
    python tools/cov_walk_bits.py            print the hashes, compare with the recorded ones when they exist
    python tools/cov_walk_bits.py --write    record them, with the compiler's version line
The file may be regenerated only from a build whose three kernels and ksx_exp.h are unchanged."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "cov_walk_bits.json")
REGEN = ("tests/golden/cov_walk_bits.json may be regenerated (tools/cov_walk_bits.py --write) only from a build whose ksx_kernel, "
         "believer_kernel, kg_kernel and ksx_exp.h are unchanged")

DIMS = (3, 6, 12, 24, 40, 60, 96)
KERNELS = ("ardse", "ardmatern52")
NS = (24, 100, 150)
M, S = 200, 2


def case_ids():
    ids = []
    for kern in KERNELS:
        for d in DIMS:
            ids.append("ksx-%s-d%d-N150" % (kern, d))
            for what in ("believer", "kg"):
                ids.extend("%s-%s-d%d-N%d" % (what, kern, d, N) for N in NS)
    return ids


def points(n, d, first):
    """n rows of a Kronecker sequence in the unit cube: frac(row * a_k), row = first, first + 1, ..; exact operations only."""
    a = np.fmod((np.arange(d, dtype=np.float64) + 1.0) * 0.7548776662466927, 1.0)
    r = np.arange(n, dtype=np.float64).reshape(n, 1) + float(first)
    return np.fmod(r * a.reshape(1, d), 1.0)


def problem(d, N):
    X, Xc = points(N, d, 1), points(M, d, 1001)
    s = np.zeros(N)
    for k in range(d):
        s = s + X[:, k]
    t = s / float(d) - 0.5
    Y = ((t * t) * 4.0 + X[:, 0] * 0.3).reshape(N, 1)
    ls = (np.fmod((np.arange(d, dtype=np.float64) + 1.0) * 0.381966011250105, 1.0) * 0.5 + 0.75) * (d / 8.0)
    hyps = [{"lenscale_sq": ls * (1.0 + 0.25 * s_), "amp": 1.3 - 0.2 * s_, "noise": 1e-3, "mean": 0.1} for s_ in range(S)]
    return X, Y, Xc, hyps


def _clean(rep, what):
    if np.any(np.asarray(rep["jitter"]) != 0.0) or np.any(np.asarray(rep["info"]) != 0):
        raise RuntimeError("%s: the fit needed jitter (%r, %r): the case no longer pins the plain path" % (what, rep["jitter"], rep["info"]))


def _digest(items):
    h = hashlib.sha256()
    for a in items:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_hash(ctx, cid):
    what, kern, d, N = cid.split("-")
    d, N = int(d[1:]), int(N[1:])
    X, Y, Xc, hyps = problem(d, N)
    fmin = [float(Y.min())]
    ctx.gp_set_kernel(kern)
    ctx.grid_upload(Xc)
    if what == "ksx":
        h = hyps[0]
        _clean(ctx.gp_fit(X, Y, h["lenscale_sq"], h["amp"], h["noise"], h["mean"]), cid)
        L, al, _ = ctx.gp_download(N)
        mean, var = ctx.gp_predict()
        ctx.gp_set_data(X, Y)
        v, i, rep = ctx.eval_nominate(hyps, score="ei", fmin=fmin, want_report=True)
        _clean(rep, cid)
        acc = ctx.score_finish(1.0, download=True)[2]
        return _digest([L, al, mean, var, np.float64(v), np.int64(i), acc])
    ctx.gp_set_data(X, Y)
    if what == "believer":
        vals, idx, rep = ctx.eval_nominate_batch(hyps, 3, score="ei", fmin=fmin, want_report=True)
        _clean(rep, cid)
        acc = ctx.score_finish(1.0, download=True)[2]
        return _digest([vals, idx, acc])
    v, i, rep = ctx.kg_nominate(hyps, points=5, want_report=True, trace=True)
    _clean(rep, cid)
    last = ctx.kg_last(slopes=True)
    return _digest([np.float64(v), np.int64(i), last["rows"], last["alpha"], last["slopes"], last["values"]])


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def compiler_line():
    try:
        out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout
        return next((ln.strip() for ln in out.splitlines() if "HIP version" in ln), out.strip().splitlines()[0] if out.strip() else "unknown")
    except OSError:
        return "unknown"


def main():
    import bot7_amd
    ctx = bot7_amd.Context(0)
    got = {}
    for cid in case_ids():
        got[cid] = case_hash(ctx, cid)
        print(got[cid], cid, flush=True)
    ctx.close()
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump({"hipcc": compiler_line(), "sha256": got}, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
        return 0
    if not os.path.exists(GOLDEN):
        return 0
    want = recorded()["sha256"]
    bad = [c for c in got if want.get(c) != got[c]]
    print("%d of %d cases differ from the recorded bits" % (len(bad), len(got)))
    if bad:
        print(REGEN)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
