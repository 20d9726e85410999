"""Where a nomination's fits live, and what that leaves in the context's own fit slot.

The posterior launchers are told where a fit lives (FitSet, csrc/b7_internal.h) instead of reading the context's fit fields.  Two
places where the two used to be tied together:

* the route "fits side by side, posterior one sample after the other" (a workspace too small for K* of all samples) predicts from
  the batch slots; the context's own slot must be exactly what a fit made afterwards expects, and the route must repeat itself;
* with one hyper sample a batch nomination's believer reads the fit where it was produced: the context's own slot in the general
  layout, batch slot 0 in the small regime.  A context on the launch schedule produces it in its own slot in both.

Everything is held bit for bit; nothing here has a tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def problem(N, d, M, S, seed):
    rng = np.random.default_rng(seed)
    X, Xc = rng.random((N, d)), rng.random((M, d))
    y = np.sin(3.0 * X[:, :3].sum(axis=1)) + X[:, -1] ** 2 + 0.05 * rng.standard_normal(N)
    amp = float(np.var(y))
    hyps = [{"lenscale_sq": rng.uniform(0.5, 1.5, d) * d / 6.0, "amp": amp * (1.0 + 0.2 * s), "noise": 1e-2 * amp,
             "mean": float(np.mean(y)) + 0.05 * s} for s in range(S)]
    return X, y.reshape(-1, 1), Xc, hyps


def stage(c, X, y, Xc):
    c.gp_set_kernel("ardse")
    c.grid_upload(Xc)
    c.gp_set_data(X, y)


def counted(c, call):
    c.profile_enable(True)
    try:
        c.profile_reset()
        out = call()
        counts = {ph: c.profile_get(ph)[1] for ph in ("kxx", "ksx", "post", "kpost")}
    finally:
        c.profile_enable(False)
    return out, counts


def bits(v):
    return np.asarray(v, dtype=np.float64).tobytes()


def test_own_slot_after_the_sample_by_sample_route():
    """N = 150 (Npad 256), d = 5, M = 200, S = 3 under a 128 KiB workspace: the fits run side by side (one "kxx" phase), the
    posterior one sample after the other (at least S "ksx" and "post" phases).  A fit with a fourth hyper vector and its
    prediction on the same context equal a fresh context's byte for byte, and the nomination repeated gives the first call's bits."""
    import bot7_amd
    S = 3
    X, y, Xc, hyps = problem(150, 5, 200, S + 1, 4)
    sp = {"score": "ei", "fmin": [float(y.min())], "tradeoff": 0.0}
    c = bot7_amd.Context(0)
    try:
        stage(c, X, y, Xc)
        c.set_workspace(128 << 10)
        try:
            (v1, i1), n1 = counted(c, lambda: c.eval_nominate(hyps[:S], **sp))
            assert n1["kxx"] == 1 and n1["ksx"] >= S and n1["post"] >= S and n1["kpost"] == 0, n1
            rep = c.gp_fit_hyp(**hyps[S])
            mu, var = c.gp_predict(download=True)
            (v2, i2), n2 = counted(c, lambda: c.eval_nominate(hyps[:S], **sp))
        finally:
            c.set_workspace(4 << 30)
    finally:
        c.close()
    f = bot7_amd.Context(0)
    try:
        stage(f, X, y, Xc)
        frep = f.gp_fit_hyp(**hyps[S])
        fmu, fvar = f.gp_predict(download=True)
    finally:
        f.close()
    assert rep["info"] == 0 and frep["info"] == 0 and rep["jitter"] == frep["jitter"] == 0.0
    assert np.isfinite(mu).all() and np.isfinite(var).all()
    assert mu.tobytes() == fmu.tobytes() and var.tobytes() == fvar.tobytes()
    assert n2 == n1, (n1, n2)
    assert bits(v2) == bits(v1) and i2 == i1, ((v1, i1), (v2, i2))


def diag_batch(monkeypatch, env, value, X, y, Xc, hyps, q, sp):
    """eval_nominate_batch on a fresh context of the diagnostic build created under the switch env=value: (values, picks, phase counts)"""
    import bot7_amd
    monkeypatch.setenv(env, value)
    try:
        cd = bot7_amd.Context(0, lib="diag")
    finally:
        monkeypatch.delenv(env)
    try:
        stage(cd, X, y, Xc)
        (vd, idd), nd = counted(cd, lambda: cd.eval_nominate_batch(hyps, q, **sp))
    finally:
        cd.close()
    return vd, idd, nd


@pytest.mark.parametrize("N,d", [(150, 5), (24, 3)])
def test_one_sample_batch_reads_the_fit_where_it_was_produced(N, d, monkeypatch):
    """S = 1, q = 3.  N = 150: the fit is produced in the context's own slot and stays there.  N = 24: the one-launch fit
    produces it in batch slot 0 (no "kxx" phase).  A diagnostic context on the launch schedule (B7_POTRF_SCHED=1) assembles K
    itself (one "kxx" phase per fit) and keeps the fit in its own slot in both cases: the picks are the same, and at N = 150,
    where both contexts run the same arithmetic, so are the bits of the values.  At N = 24 the launch schedule factors the one
    64-block with another kernel than the one-launch fit, and its values differ in the last bits wherever the believer reads the
    fit (1.1e-13 relative on pick 1); there the values are held, bit for bit, to a
    diagnostic context with B7_FIT_SMALL=0 -- the general schedule that the small kernels equal bit for bit
    (test_gpu_parity.py), which also fits into, and keeps, the context's own slot."""
    import bot7_amd
    q, M = 3, 200
    X, y, Xc, hyps = problem(N, d, M, 1, 4)
    sp = {"score": "ei", "fmin": [float(y.min())], "tradeoff": 0.0}
    c = bot7_amd.Context(0)
    try:
        stage(c, X, y, Xc)
        (v, i), n = counted(c, lambda: c.eval_nominate_batch(hyps, q, **sp))
    finally:
        c.close()
    vd, idd, nd = diag_batch(monkeypatch, "B7_POTRF_SCHED", "1", X, y, Xc, hyps, q, sp)
    assert n["kxx"] == (0 if N <= 128 else 1) and nd["kxx"] == 1, (n, nd)
    assert len(set(i.tolist())) == q and i.min() >= 1 and i.max() <= M
    print("N = %d: picks %s / %s, values %s / %s" % (N, i.tolist(), idd.tolist(), v.tolist(), vd.tolist()))
    assert np.array_equal(i, idd)
    if N <= 128:
        vd, idd, nd = diag_batch(monkeypatch, "B7_FIT_SMALL", "0", X, y, Xc, hyps, q, sp)
        print("N = %d, B7_FIT_SMALL=0: picks %s, values %s" % (N, idd.tolist(), vd.tolist()))
        assert nd["kxx"] == 1 and np.array_equal(i, idd), (nd, i, idd)
    assert bits(v) == bits(vd)
