"""Worker of tests/test_gpu_kg.py::test_world_of_two_is_refused: rank `r` of a world of two on cuda:0 (communicator over the
shared-memory RCCL double).  Each rank holds its shard of the candidates; b7_kg_nominate must refuse (the knowledge gradient over a
sharded grid is not built) without issuing a collective, and the b7_eval_nominate that follows must work as ever.
usage: python tests/_kg_worker.py rank world id_hex out.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402
from harness import dist  # noqa: E402
from test_gpu_kg import hyper_samples, problem  # noqa: E402

rank, world, ident, out = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4]
ctx = bot7_amd.Context(0)
ctx.comm_init(rank, world, ident.ljust(128, b"\0"))
X, y, Xc, hyp = problem(37, 3, 1000, seed=1)
hyps = hyper_samples(hyp, 2)
lo, hi = dist.shard_range(len(Xc), rank, world)
ctx.grid_upload(Xc[lo:hi])
ctx.gp_set_data(X, y)
res = {"code": 0, "message": ""}
try:
    ctx.kg_nominate(hyps, points=4)
except _lib.Bot7HipError as e:
    res["code"], res["message"] = e.code, str(e)
res["value"], res["index"] = ctx.eval_nominate(hyps, global_row_offset=lo, score="ei", fmin=[float(np.min(y))])
with open(out, "w") as f:
    json.dump(res, f)
