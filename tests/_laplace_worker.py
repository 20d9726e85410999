"""Worker of tests/test_gpu_laplace.py::test_world_of_two_is_refused: rank `r` of a world of two on cuda:0 (communicator over the
shared-memory RCCL double).  Each rank holds its shard of the candidates; b7_clf_nll_batch, b7_clf_fit_hyp and b7_clf_eval_logfeas
must refuse (the classifier over a sharded grid is not built) without issuing a collective, and the b7_eval_nominate that follows
must work as ever.
usage: python tests/_laplace_worker.py rank world id_hex out.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402
from harness import dist  # noqa: E402
from test_gpu_laplace import _clf_problem  # noqa: E402

rank, world, ident, out = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4]
ctx = bot7_amd.Context(0)
ctx.comm_init(rank, world, ident.ljust(128, b"\0"))
X, v, G, hyps = _clf_problem(24, 3, 600)
hyps = hyps[:2]
lo, hi = dist.shard_range(len(G), rank, world)
ctx.grid_upload(G[lo:hi])
ctx.gp_set_data(X, v)
res = {"codes": [], "messages": []}
h = hyps[0]
for call in (lambda: ctx.clf_nll_batch(hyps), lambda: ctx.clf_fit_hyp(h["lenscale_sq"], h["amp"], 0.0, h["mean"]), lambda: ctx.clf_eval_logfeas(hyps)):
    try:
        call()
        res["codes"].append(0)
        res["messages"].append("")
    except _lib.Bot7HipError as e:
        res["codes"].append(e.code)
        res["messages"].append(str(e))
res["value"], res["index"] = ctx.eval_nominate(hyps, global_row_offset=lo, score="ei", fmin=[0.0])
with open(out, "w") as f:
    json.dump(res, f)
