"""Worker of tests/test_gpu_nllgrad.py::test_world_of_two_is_refused: rank `r` of a world of two on cuda:0 (communicator over the
shared-memory RCCL double).  b7_gp_fit_hyp_grad, b7_gp_nll_grad and b7_gp_fit_map must refuse (likelihood gradients over sharded
data are not built) without issuing a collective, and the b7_gp_fit_hyp that follows must work as ever.
usage: python tests/_nllgrad_worker.py rank world id_hex out.json"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import bot7_amd  # noqa: E402
from bot7_amd import _lib  # noqa: E402
import _nllgrad_ref as R  # noqa: E402

rank, world, ident, out = int(sys.argv[1]), int(sys.argv[2]), bytes.fromhex(sys.argv[3]), sys.argv[4]
ctx = bot7_amd.Context(0)
ctx.comm_init(rank, world, ident.ljust(128, b"\0"))
X, y, h = R.problem(24, 3, 7)
ctx.gp_set_data(X, y)
fit = ctx.gp_fit_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)
res = {"codes": [], "messages": []}
t0 = np.concatenate([np.log(h["lenscale_sq"]), [np.log(h["amp"]), np.log(h["noise"]), h["mean"]]])
for call in (lambda: ctx.gp_fit_hyp_grad(h["lenscale_sq"], h["amp"], h["noise"], h["mean"]), lambda: ctx.gp_nll_grad(),
             lambda: ctx.gp_fit_map(t0, t0 - 1.0, t0 + 1.0)):
    try:
        call()
        res["codes"].append(0)
        res["messages"].append("")
    except _lib.Bot7HipError as e:
        res["codes"].append(e.code)
        res["messages"].append(str(e))
res["nll"] = float(ctx.gp_fit_hyp(h["lenscale_sq"], h["amp"], h["noise"], h["mean"], want_nll=True)["nll"][0])
res["nll_before"] = float(fit["nll"][0])
with open(out, "w") as f:
    json.dump(res, f)
