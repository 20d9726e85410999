"""Worker of tests/test_gpu_mes.py::test_world_of_two_is_refused: rank `r` of a world of two on cuda:0 (communicator over the
shared-memory RCCL double).  Each rank holds its shard of the candidates; b7_eval_nominate(B7_SCORE_MES) and b7_score_mes must
refuse (y* over a sharded grid is not built) without issuing a collective, and the EI nomination that follows must work as ever.
usage: python tests/_mes_worker.py rank world id_hex out.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402
from harness import dist  # noqa: E402
from test_gpu_mes import world_problem  # noqa: E402

rank, world, ident, out = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4]
ctx = bot7_amd.Context(0)
ctx.comm_init(rank, world, ident.ljust(128, b"\0"))
X, y, Xc, hyps = world_problem()
lo, hi = dist.shard_range(len(Xc), rank, world)
ctx.grid_upload(Xc[lo:hi])
ctx.gp_set_data(X, y)
res = {"codes": [], "messages": []}
h = hyps[0]
for call in (lambda: ctx.eval_nominate(hyps, score="mes", global_row_offset=lo),
             lambda: (ctx.gp_predict_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"]), ctx.score_reset(), ctx.score_mes())):
    try:
        call()
        res["codes"].append(0)
        res["messages"].append("")
    except _lib.Bot7HipError as e:
        res["codes"].append(e.code)
        res["messages"].append(str(e))
ctx.gp_set_data(X, y)
res["value"], res["index"] = ctx.eval_nominate(hyps, score="ei", fmin=[float(y.min())], global_row_offset=lo)
with open(out, "w") as f:
    json.dump(res, f)
