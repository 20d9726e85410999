"""The catalogue of context-reuse tests (tests/test_reuse_host.py, tests/test_gpu_reuse.py): a deterministic problem generator,
CALLS (one entry per public result-producing route of bot7_amd.Context), EXEMPT (the public methods that need no entry) and the
walk-and-compare machinery.  A reused context must give, call for call, the bytes a new context gives for the same call: DESIGN.md
section 3, "the same call gives the same bits".

An entry assumes only what `setup` leaves: the problem's grid and data resident, its covariance kernel selected, default options.
It returns a dict of name -> bytes | int | str; a refusal (Bot7HipError) is a result too, ("refused", code, message).  The entries
marked `mutates` change the grid or the data; the walker runs `setup` again behind them."""
import collections

import numpy as np

from bot7_amd._lib import Bot7HipError, pareto_front2, pareto_front3

KINDS = ("ei", "cb", "logei", "logpi", "mes")
Z = 50   # the head's basis width: a d -> 50 tanh layer


class Problem(object):
    pass


def _smooth(X, phase):
    d = X.shape[1]
    k = np.arange(1, d + 1, dtype=np.float64)
    return np.sin(3.0 * X + 0.7 * k + phase).sum(axis=1) / np.sqrt(d) + (X * np.cos(k + phase)).sum(axis=1) ** 2 / d


def _hyps(d, S, y):
    amp = float(np.var(y))
    return [dict(lenscale_sq=np.full(d, d / 8.0 * (1.0 + 0.25 * s)), amp=amp, noise=1e-3 * amp, mean=float(np.mean(y))) for s in range(S)]


def problem(N, d, M, S, seed, ycols=1, scale=1.0, dup_rows=0, zero_noise=False, head=False, kernel="ardse", q=4, n_features=64,
            name=None):
    """X in [0, 1)^d, Y a smooth function plus small noise, times `scale`; S well-conditioned hyper vectors (lenscale_sq =
    d/8 (1 + 0.25 s), noise = 1e-3 amp).  dup_rows: rows [dup_rows, 2 dup_rows) repeat rows [0, dup_rows); zero_noise: noise 0 (the two
    together make K singular: the jitter schedule).  head: `setup` makes the context a Bayesian-linear head before the GP data
    arrive.  Two more objectives (Y2, Y3) for the partner contexts of the hypervolume calls."""
    rng = np.random.default_rng(seed)
    P = Problem()
    P.N, P.d, P.M, P.S, P.ycols, P.kernel, P.head, P.q, P.n_features = N, d, M, S, ycols, kernel, head, q, n_features
    P.X = rng.random((N, d))
    P.G = rng.random((M, d))
    if dup_rows:
        P.X[dup_rows:2 * dup_rows] = P.X[:dup_rows]
    cols = [_smooth(P.X, 0.3 * c) for c in range(ycols)]
    noise = 0.0 if zero_noise else 0.01
    P.Y = scale * (np.stack(cols, axis=1) + noise * rng.standard_normal((N, ycols)))
    P.Y2 = scale * (_smooth(P.X, 1.9) + noise * rng.standard_normal(N))
    P.Y3 = scale * (_smooth(P.X, 4.1) + noise * rng.standard_normal(N))
    if dup_rows:
        for y in (P.Y, P.Y2, P.Y3):
            y[dup_rows:2 * dup_rows] = y[:dup_rows]
    P.hyps, P.hyps2, P.hyps3 = _hyps(d, S, P.Y[:, 0]), _hyps(d, S, P.Y2), _hyps(d, S, P.Y3)
    if zero_noise:
        for h in P.hyps + P.hyps2 + P.hyps3:
            h["noise"] = 0.0
    P.fmin = P.Y.min(axis=0)
    P.pend = rng.random((3, d))
    P.x_new = rng.random(d)
    P.y_new = scale * np.array([_smooth(P.x_new[None], 0.3 * c)[0] for c in range(ycols)])
    P.logw = np.where(np.arange(M) % 7 == 3, -np.inf, -0.5 * rng.random(M))
    P.net = ([rng.normal(scale=1.0 / np.sqrt(d), size=(Z, d))], [rng.normal(scale=0.1, size=Z)])
    P.blr = (1.0, 1.0 / max(1e-3 * float(np.var(P.Y[:, 0])), 1e-300), float(np.mean(P.Y[:, 0])))   # alpha_prec, beta, mean
    P.name = name or "N%d_d%d_M%d_S%d_c%d_%s_seed%d" % (N, d, M, S, ycols, kernel, seed)
    P.key = (P.name, N, d, M, S, ycols, kernel, seed, scale, dup_rows, zero_noise, head)
    return P


def derived(P, X, Y, Y2, Y3, G, tag):
    """P's problem on another data set and grid (the hypers, the pending points and the network stay): what a walker holds after
    grid_remove_rows / gp_append, for the reference that is given the same state by upload."""
    Q = Problem()
    Q.__dict__.update(P.__dict__)
    Q.X, Q.Y, Q.Y2, Q.Y3, Q.G = X, Y, Y2, Y3, G
    Q.N, Q.M = X.shape[0], G.shape[0]
    Q.fmin = P.fmin
    Q.logw = np.resize(P.logw, Q.M)
    Q.name = "%s/%s" % (P.name, tag)
    Q.key = P.key + (tag,)
    return Q


Env = collections.namedtuple("Env", "ctx p2 p3 P")


def setup(env):
    """What every entry may assume.  The partners hold the same grid and the data of objectives 2 and 3."""
    c, P = env.ctx, env.P
    c.gp_set_opts()
    c.mes_set_levels(8)
    c.grid_upload(P.G)
    if P.head:   # the context has just been a Bayesian-linear head: N = z rows of features, model_kind 1
        c.blr_fit_x(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr)
        c.blr_basis(P.net[0], P.net[1], "Tanh")
        c.blr_predict(download=False)
    c.gp_set_kernel(P.kernel)
    c.gp_set_data(P.X, P.Y)
    for p, y in ((env.p2, P.Y2), (env.p3, P.Y3)):
        if p is not None:
            p.gp_set_opts()
            p.grid_upload(P.G)
            p.gp_set_kernel(P.kernel)
            p.gp_set_data(P.X, y)


def _b(a, dtype=np.float64):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype)).tobytes()


def _report(rep):
    return {"jitter": _b(rep["jitter"]), "info": _b(rep["info"], np.int32)}


def _acc(c):
    v, i, sc = c.score_finish(1.0, download=True)
    return {"acc_value": _b(v), "acc_idx": int(i), "acc": _b(sc)}


# ---- fits and likelihoods
def c_gp_fit(env):
    c, P = env.ctx, env.P
    r = c.gp_fit(P.X, P.Y, want_nll=True, **P.hyps[0])
    mu, var = c.gp_predict()
    return {"nll": _b(r["nll"]), "jitter": _b(r["jitter"]), "info": int(r["info"]), "mean": _b(mu), "var": _b(var)}


def c_gp_fit_hyp(env):
    c, P = env.ctx, env.P
    r = c.gp_fit_hyp(want_nll=True, **P.hyps[0])
    L, al, Li = c.gp_download(P.N, P.ycols)
    r2 = c.gp_predict_hyp(download=True, want_nll=True, **P.hyps[-1])
    return {"nll": _b(r["nll"]), "jitter": _b(r["jitter"]), "info": int(r["info"]), "L": _b(L), "alpha": _b(al), "Linv": _b(Li),
            "nll2": _b(r2["nll"]), "jitter2": _b(r2["jitter"]), "info2": int(r2["info"]), "mean": _b(r2["mean"]), "var": _b(r2["var"])}


def c_gp_set_data(env):
    c, P = env.ctx, env.P
    c.gp_set_data(P.X[::-1], P.Y[::-1])
    r = c.gp_fit_hyp(want_nll=True, **P.hyps[0])
    mu, var = c.gp_predict()
    return {"nll": _b(r["nll"]), "jitter": _b(r["jitter"]), "info": int(r["info"]), "mean": _b(mu), "var": _b(var)}


def c_gp_nll_batch(env):
    c, P = env.ctx, env.P
    nll, jit, info = c.gp_nll_batch(np.stack([h["lenscale_sq"] for h in P.hyps]), [h["amp"] for h in P.hyps],
                                    [h["noise"] for h in P.hyps], [h["mean"] for h in P.hyps], want_info=True)
    return {"nll": _b(nll), "jitter": _b(jit), "info": _b(info, np.int32)}


def c_gp_nll1(env):
    h = env.P.hyps[-1]
    nll, jit, info = env.ctx.gp_nll1(h["lenscale_sq"], h["amp"], h["noise"], h["mean"])
    return {"nll": _b(nll), "jitter": _b(jit), "info": int(info)}


def c_gp_opts(env):
    c, P = env.ctx, env.P
    try:
        c.gp_set_opts(var_with_noise=1, var_clamp=1, var_min=1e-12)
        c.gp_fit_hyp(**P.hyps[0])
        mu, var = c.gp_predict()
    finally:
        c.gp_set_opts()
    return {"mean": _b(mu), "var": _b(var)}


def c_gp_kernel(env):
    c, P = env.ctx, env.P
    try:
        c.gp_set_kernel("ardmatern52" if P.kernel == "ardse" else "ardse")
        v, i, rep = c.eval_nominate(P.hyps, score="ei", fmin=P.fmin, want_report=True)
        out = dict(_report(rep), value=_b(v), idx=int(i), **_acc(c))
    finally:
        c.gp_set_kernel(P.kernel)
    return out


# ---- plain scoring
def _score(kind):
    def fn(env):
        c, P = env.ctx, env.P
        c.gp_fit_hyp(**P.hyps[0])
        c.gp_predict(download=False)
        c.score_reset()
        if kind == "cb":
            c.score_cb()
        elif kind == "mes":
            c.score_mes()
        else:
            getattr(c, "score_" + kind)(P.fmin, 0.0)
        out = _acc(c)
        if kind == "mes":
            ys, br = c.mes_last_ystar()
            out.update(ystar=_b(ys), bracket=_b(br))
        return out
    return fn


def c_score_finish_global(env):
    c, P = env.ctx, env.P
    c.gp_fit_hyp(**P.hyps[0])
    c.gp_predict(download=False)
    c.score_reset()
    c.score_ei(P.fmin, 0.0)
    v, i = c.score_finish_global(1.0, 0)
    x = c.exchange_info()
    return {"value": _b(v), "idx": int(i), "world": int(x["world"]), "rows": _b(x["rows"], np.int64), "winner": int(x["winner_idx1"]),
            "winner_row": _b(x["winner_row"])}


# ---- eval_nominate and the other nominations
def _eval_nominate(kind, all_samples, levels=None):
    def fn(env):
        c, P = env.ctx, env.P
        try:
            v, i, rep = c.eval_nominate(P.hyps if all_samples else P.hyps[:1], score=kind, fmin=P.fmin, want_report=True, levels=levels)
            out = dict(_report(rep), value=_b(v), idx=int(i), **_acc(c))
            if kind == "mes":
                ys, br = c.mes_last_ystar()
                out.update(ystar=_b(ys), bracket=_b(br))
        finally:
            if levels is not None:
                c.mes_set_levels(8)
        return out
    return fn


def c_nominate_commit(env):
    c, P = env.ctx, env.P
    v, i = c.eval_nominate(P.hyps, score="ei", fmin=P.fmin)
    row, off = c.nominate_commit(i, 0)
    return {"value": _b(v), "idx": int(i), "row": _b(row), "offset": int(off), "grid": _b(c.grid_download())}


def c_batch(env):
    c, P = env.ctx, env.P
    vals, idx, rep = c.eval_nominate_batch(P.hyps, P.q, score="ei", fmin=P.fmin, want_report=True)
    return dict(_report(rep), values=_b(vals), idx=_b(idx, np.int64), **_acc(c))


def c_refine(env):
    c, P = env.ctx, env.P
    v, i, x, rv, ri, rep = c.eval_nominate_refine(P.hyps, score="ei", fmin=P.fmin, starts=4, iters=4, want_report=True)
    last = c.refine_last()
    return dict(_report(rep), value=_b(v), idx=int(i), x=_b(x), refined=_b(rv), start=int(ri), last_x=_b(last["x"]),
                last_val=_b(last["val"]), last_idx=_b(last["start_idx1"], np.int64), last_status=_b(last["status"], np.int32))


def c_ts(env):
    c, P = env.ctx, env.P
    vals, idx, rep = c.ts_nominate(P.hyps, P.q // 2, n_features=P.n_features, seed=7, want_report=True)
    dr = c.ts_last_draws(0)
    return dict(_report(rep), values=_b(vals), idx=_b(idx, np.int64), paths=_b(c.ts_last_paths()), omega=_b(dr["omega"]),
                phase=_b(dr["phase"]), weight=_b(dr["weight"]), eps=_b(dr["eps"]))


def c_kg(env):
    c, P = env.ctx, env.P
    v, i, rep = c.kg_nominate(P.hyps, points=4, want_report=True)
    last = c.kg_last()
    return dict(_report(rep), value=_b(v), idx=int(i), rows=_b(last["rows"], np.int64), alpha=_b(last["alpha"]),
                values=_b(last["values"]), own_alpha=_b(last["own_alpha"]))


def c_feas(env):
    c, P = env.ctx, env.P
    env.p2.eval_nominate(P.hyps2, score="logpi", fmin=[float(np.median(P.Y2))])   # a constraint's log feasibility, on its own context
    c.feas_reset()
    c.feas_add(P.logw)
    c.feas_add_acc(env.p2)
    fv, fi = c.feas_nominate()
    v, i, rep = c.eval_nominate_feasible(P.hyps, score="logei", fmin=P.fmin, want_report=True)
    return dict(_report(rep), value=_b(v), idx=int(i), column=_b(c.feas_get()), feas_value=_b(fv), feas_idx=int(fi), **_acc(c))


# ---- the kept posterior and the hypervolume nominations
def c_posterior(env):
    c, P = env.ctx, env.P
    out = _report(c.eval_posterior(P.hyps, want_report=True))
    for s in range(P.S):
        mu, var = c.posterior_get(s)
        out["mean%d" % s], out["var%d" % s] = _b(mu), _b(var)
    return out


def _fronts(P, m):
    Y = np.stack([P.Y[:, 0], P.Y2, P.Y3][:m], axis=1)
    ref = Y.max(axis=0) + 0.1 * (Y.max(axis=0) - Y.min(axis=0))
    return (pareto_front2 if m == 2 else pareto_front3)(Y, ref)[0], ref


def _ehvi(who, m):
    def fn(env):
        c, P = env.ctx, env.P
        front, ref = _fronts(P, m)
        c.eval_posterior(P.hyps)
        env.p2.eval_posterior(P.hyps2)
        if m == 3:
            env.p3.eval_posterior(P.hyps3)
            v, i = getattr(c, who)(env.p2, env.p3, front, ref)
        else:
            v, i = getattr(c, who)(env.p2, front, ref)
        return dict(value=_b(v), idx=int(i), **_acc(c))
    return fn


# ---- samplers and model edits
def c_slice(env):
    c, P = env.ctx, env.P
    t = np.stack([np.concatenate([np.log(h["lenscale_sq"]), [np.log(h["amp"]), np.log(max(h["noise"], 1e-12)), h["mean"]]])
                  for h in (P.hyps[0], P.hyps[-1])])
    t[1] += 0.05
    r = c.gp_slice_sample(t, t[0] - 3.0, t[0] + 3.0, np.ones(P.d + 3), U=2, seed=11, max_evals=64)
    return {"theta": _b(r["theta"]), "value": _b(r["value"]), "status": _b(r["status"], np.int32), "nevals": _b(r["nevals"], np.int32)}


def c_fantasize(env):
    c, P = env.ctx, env.P
    c.gp_fit_hyp(**P.hyps[0])
    y, mu, cov = c.gp_fantasize(P.pend, 4, seed=5, want_moments=True)
    return {"draws": _b(y), "mu": _b(mu), "cov": _b(cov)}


def c_predict_at(env):
    c, P = env.ctx, env.P
    c.gp_fit_hyp(**P.hyps[0])
    mu, var = c.gp_predict_at(P.pend)
    return {"mean": _b(mu), "var": _b(var)}


def c_append(env):
    c, P = env.ctx, env.P
    c.gp_fit_hyp(**P.hyps[0])
    c.gp_append(P.x_new, P.y_new)
    L, al, Li = c.gp_download(P.N + 1, P.ycols)
    mu, var = c.gp_predict()
    r = c.gp_fit_hyp(want_nll=True, **P.hyps[-1])   # the resident data grew with the fit
    return {"L": _b(L), "alpha": _b(al), "Linv": _b(Li), "mean": _b(mu), "var": _b(var), "nll": _b(r["nll"])}


def c_grad_at(env):
    c, P = env.ctx, env.P
    c.gp_fit_hyp(**P.hyps[0])
    mu, var, dmu, dvar = c.gp_grad_at(P.pend)
    return {"mean": _b(mu), "var": _b(var), "dmean": _b(dmu), "dvar": _b(dvar)}


# ---- grids: each is followed by a nomination over the new grid
def _after_grid(env, out):
    c, P = env.ctx, env.P
    v, i = c.eval_nominate(P.hyps[:1], score="ei", fmin=P.fmin)
    out.update(grid=_b(c.grid_download()), value=_b(v), idx=int(i), **_acc(c))
    return out


def c_grid_upload(env):
    env.ctx.grid_upload(env.P.G[::-1][: env.P.M - 5])
    return _after_grid(env, {})


def c_grid_sobol(env):
    return _after_grid(env, {"sobol": _b(env.ctx.grid_sobol(env.P.M - 1, env.P.d, skip=3))})


def c_grid_random(env):
    c, P = env.ctx, env.P
    out = {"random": _b(c.grid_random(P.M - 2, P.d, seed=9, row_offset=5))}
    lo, hi = c.grid_colrange()
    c.grid_apply_onesided(mins=np.full(P.d, 0.125), col_ext=-lo)
    out.update(lo=_b(lo), hi=_b(hi))
    return _after_grid(env, out)


def c_grid_random_torch(env):
    return _after_grid(env, {"random": _b(env.ctx.grid_random_torch(env.P.M - 3, env.P.d, seed=4))})


def c_grid_trust_region(env):
    c, P = env.ctx, env.P
    center = P.X[int(np.argmin(P.Y[:, 0]))]
    c.grid_trust_region(center, np.clip(center - 0.2, 0.0, 1.0), np.clip(center + 0.2, 0.0, 1.0), 0.5, seed=3)
    return _after_grid(env, {})


def c_grid_remove_rows(env):
    c, P = env.ctx, env.P
    return _after_grid(env, {"removed": _b(c.grid_remove_rows([2, 5, P.M]))})


def c_grid_remove(env):
    return _after_grid(env, {"row": _b(env.ctx.grid_remove(3))})


# ---- the Bayesian-linear head
def _blr(kind):
    def fn(env):
        c, P = env.ctx, env.P
        v, i, j = c.blr_eval_nominate(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr, score=kind, fmin=P.fmin[:1], want_jitter=True)
        return dict(value=_b(v), idx=int(i), jitter=_b(j), **_acc(c))
    return fn


def _blr_marg(kind):
    def fn(env):
        c, P = env.ctx, env.P
        a, b, m = P.blr
        v, i, j, nll = c.blr_eval_nominate_marg(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], [a, 2.0 * a, 0.5 * a], [b, 0.5 * b, b], [m, m, 0.9 * m],
                                                score=kind, fmin=P.fmin[:1], want_nll=True)
        return dict(value=_b(v), idx=int(i), jitter=_b(j), nll=_b(nll), **_acc(c))
    return fn


def c_blr_predict(env):
    c, P = env.ctx, env.P
    nll = c.blr_fit_x(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr, want_nll=True)
    feats = c.blr_basis(P.net[0], P.net[1], "Tanh", download=True)
    mu, var = c.blr_predict()
    c.score_reset()
    c.score_ei(P.fmin[:1], 0.0)
    return dict(nll=_b(nll), features=_b(feats), mean=_b(mu), var=_b(var), **_acc(c))


def c_blr_features(env):
    c, P = env.ctx, env.P
    Z0 = c.blr_basis(P.net[0], P.net[1], "Tanh", X=P.X)
    c.blr_features(c.blr_basis(P.net[0], P.net[1], "Tanh", X=P.G))
    nll = c.blr_fit(Z0, P.Y[:, 0], *P.blr, want_nll=True)
    mu, var = c.blr_predict()
    return dict(nll=_b(nll), Z0=_b(Z0), mean=_b(mu), var=_b(var))


def _on_the_head(policy):
    """A GP-only policy asked of a context that is a head: its fit slot and N are the head's."""
    def fn(env):
        c, P = env.ctx, env.P
        c.blr_fit_x(P.net[0], P.net[1], "Tanh", P.X, P.Y[:, 0], *P.blr)
        if policy == "kg":
            v, i = c.kg_nominate(P.hyps, points=4)
            return {"value": _b(v), "idx": int(i)}
        if policy == "mes":
            v, i = c.eval_nominate(P.hyps, score="mes")
            return {"value": _b(v), "idx": int(i)}
        vals, idx = c.eval_nominate_batch(P.hyps, P.q, score="ei", fmin=P.fmin)
        return {"values": _b(vals), "idx": _b(idx, np.int64)}
    return fn


Call = collections.namedtuple("Call", "fn methods mutates")
CALLS = collections.OrderedDict()


def _add(name, fn, methods, mutates=False):
    CALLS[name] = Call(fn, tuple(methods.split()), mutates)


_add("gp_fit+gp_predict", c_gp_fit, "gp_fit gp_predict")
_add("gp_fit_hyp+gp_predict_hyp", c_gp_fit_hyp, "gp_fit_hyp gp_predict_hyp gp_download")
_add("gp_set_data", c_gp_set_data, "gp_set_data gp_fit_hyp gp_predict", True)
_add("gp_nll_batch", c_gp_nll_batch, "gp_nll_batch")
_add("gp_nll1", c_gp_nll1, "gp_nll1")
_add("gp_set_opts", c_gp_opts, "gp_set_opts gp_fit_hyp gp_predict")
_add("gp_set_kernel", c_gp_kernel, "gp_set_kernel eval_nominate score_finish")
for _k in KINDS:
    _add("score_" + _k, _score(_k), "gp_fit_hyp gp_predict score_reset score_finish score_%s%s" % (_k, " mes_last_ystar" if _k == "mes" else ""))
_add("score_finish_global", c_score_finish_global, "score_reset score_ei score_finish_global exchange_info")
for _k in KINDS:
    _add("eval_nominate[%s,S=1]" % _k, _eval_nominate(_k, False), "eval_nominate score_finish")
    _add("eval_nominate[%s,S]" % _k, _eval_nominate(_k, True), "eval_nominate score_finish")
_add("eval_nominate[mes,levels=5]", _eval_nominate("mes", True, 5), "eval_nominate mes_set_levels mes_last_ystar")
_add("nominate_commit", c_nominate_commit, "eval_nominate nominate_commit grid_download", True)
_add("eval_nominate_batch", c_batch, "eval_nominate_batch")
_add("eval_nominate_refine", c_refine, "eval_nominate_refine refine_last refine_shape")
_add("ts_nominate", c_ts, "ts_nominate ts_last_paths ts_last_draws")
_add("kg_nominate", c_kg, "kg_nominate kg_last")
_add("eval_nominate_feasible", c_feas, "feas_reset feas_add feas_add_acc feas_nominate eval_nominate_feasible feas_get")
_add("eval_posterior", c_posterior, "eval_posterior posterior_get")
_add("ehvi_nominate", _ehvi("ehvi_nominate", 2), "eval_posterior ehvi_nominate")
_add("logehvi_nominate", _ehvi("logehvi_nominate", 2), "eval_posterior logehvi_nominate")
_add("ehvi3_nominate", _ehvi("ehvi3_nominate", 3), "eval_posterior ehvi3_nominate")
_add("logehvi3_nominate", _ehvi("logehvi3_nominate", 3), "eval_posterior logehvi3_nominate")
_add("gp_slice_sample", c_slice, "gp_slice_sample")
_add("gp_fantasize", c_fantasize, "gp_fantasize")
_add("gp_predict_at", c_predict_at, "gp_predict_at")
_add("gp_append", c_append, "gp_append gp_download", True)
_add("gp_grad_at", c_grad_at, "gp_grad_at")
_add("grid_upload", c_grid_upload, "grid_upload", True)
_add("grid_sobol", c_grid_sobol, "grid_sobol", True)
_add("grid_random", c_grid_random, "grid_random grid_colrange grid_apply_onesided", True)
_add("grid_random_torch", c_grid_random_torch, "grid_random_torch", True)
_add("grid_trust_region", c_grid_trust_region, "grid_trust_region", True)
_add("grid_remove_rows", c_grid_remove_rows, "grid_remove_rows grid_download", True)
_add("grid_remove", c_grid_remove, "grid_remove", True)
for _k in KINDS:
    _add("blr_eval_nominate[%s]" % _k, _blr(_k), "blr_eval_nominate", True)
_add("blr_eval_nominate_marg[ei]", _blr_marg("ei"), "blr_eval_nominate_marg", True)
_add("blr_eval_nominate_marg[mes]", _blr_marg("mes"), "blr_eval_nominate_marg", True)
_add("blr_predict", c_blr_predict, "blr_fit_x blr_basis blr_predict", True)
_add("blr_features", c_blr_features, "blr_basis blr_features blr_fit blr_predict", True)
for _k in ("kg", "mes", "batch"):
    _add("head_then_" + _k, _on_the_head(_k), "blr_fit_x", True)

PARTNERED = ("eval_nominate_feasible", "ehvi_nominate", "logehvi_nominate", "ehvi3_nominate", "logehvi3_nominate")   # take p2 (and p3)

EXEMPT = collections.OrderedDict([(m, "host -> device -> host on buffers of its own; nothing of the context's model or grid is read or kept")
                                  for m in ("ei_compute", "cb_compute", "logei_compute", "logpi_compute", "mes_compute", "mes_ystar", "kg_compute",
                                            "ehvi_compute", "logehvi_compute", "ehvi3_compute", "logehvi3_compute", "score_grad_compute",
                                            "rff_compute", "argmax", "chol")])
EXEMPT.update((m, "timer / profile call: returns times, not results") for m in ("timer_start", "timer_stop", "timer_ms", "profile_enable",
                                                                                 "profile_reset", "profile_get"))
EXEMPT.update((m, "communicator call: needs several processes (tests/test_dist_gloo.py, tests/test_sharded_loop.py)")
              for m in ("comm_init", "comm_info", "comm_destroy", "comm_allreduce"))
EXEMPT.update((m, "diagnostic trace of a call the catalogue runs untraced; the trace changes no result (its own tests pin that)")
              for m in ("gp_slice_trace_enable", "gp_slice_trace", "refine_trace_enable", "refine_trace"))
EXEMPT.update((m, "life cycle or a host-side query: no device result") for m in ("close", "device_info", "sync", "set_workspace", "grid_shape"))


def public_methods(cls):
    return sorted(n for n, v in vars(cls).items() if not n.startswith("_") and callable(v) and not isinstance(v, staticmethod))


def covered():
    named = set(EXEMPT)
    for call in CALLS.values():
        named.update(call.methods)
    return named


# ---- what refuses, by rule (the expected set of the tests): (call, problem) -> the error code, or None
INVALID, STATE, UNSUPPORTED = -1, -4, -5
_ONE_COLUMN = ("gp_nll_batch", "gp_nll1", "eval_nominate_batch", "eval_nominate_refine", "ts_nominate", "kg_nominate", "eval_nominate_feasible",
               "eval_posterior", "ehvi_nominate", "logehvi_nominate", "ehvi3_nominate", "logehvi3_nominate", "gp_slice_sample", "gp_fantasize",
               "gp_grad_at", "score_mes", "eval_nominate[mes,S=1]", "eval_nominate[mes,S]", "eval_nominate[mes,levels=5]")


def expected_refusal(name, P):
    if name in ("blr_eval_nominate[mes]", "blr_eval_nominate_marg[mes]"):
        return UNSUPPORTED   # MES on the head's one-call routes
    if name.startswith("head_then_"):
        return STATE         # a head's fit leaves no resident GP data: KG, MES and the believer refuse
    if P.ycols != 1 and name in _ONE_COLUMN:
        return UNSUPPORTED   # multi-column fits: fit, predict, EI / LogEI / LogPI / CB only
    if name == "gp_slice_sample" and (P.N > 128 or P.d > 32):
        return UNSUPPORTED   # the sampler is a small-regime route
    return None


# ---- walk and compare
class Mismatch(AssertionError):
    pass


def run_call(name, env):
    try:
        return CALLS[name].fn(env)
    except Bot7HipError as e:
        return ("refused", e.code, str(e))


def is_refusal(res):
    return isinstance(res, tuple) and len(res) == 3 and res[0] == "refused"


def first_difference(got, want):
    """None when the two results are the same bytes, else a description."""
    if is_refusal(got) or is_refusal(want):
        return None if got == want else "refusal differs: reused %r, fresh %r" % (got, want)
    if sorted(got) != sorted(want):
        return "items differ: reused %s, fresh %s" % (sorted(got), sorted(want))
    for k in sorted(want):
        if got[k] != want[k]:
            if isinstance(want[k], bytes) and len(got[k]) == len(want[k]) and len(want[k]) % 8 == 0:
                a, b = np.frombuffer(got[k], dtype=np.uint64), np.frombuffer(want[k], dtype=np.uint64)
                bad = np.flatnonzero(a != b)
                fa, fb = np.frombuffer(got[k], dtype=np.float64), np.frombuffer(want[k], dtype=np.float64)
                return "item %r: %d of %d words differ, first at %d: reused %r, fresh %r" % (k, bad.size, a.size, bad[0], fa[bad[0]], fb[bad[0]])
            return "item %r differs (%r vs %r)" % (k, got[k] if not isinstance(got[k], bytes) else len(got[k]),
                                                    want[k] if not isinstance(want[k], bytes) else len(want[k]))
    return None


def all_finite(res):
    """The float64 items of a result that hold a NaN or +inf (-inf is a legal log score and a legal feasibility weight); the integer
    items are left out by name."""
    bad = []
    for k, v in res.items():
        if isinstance(v, bytes) and len(v) % 8 == 0 and not k.startswith(("info", "idx", "rows", "status", "nevals", "last_idx", "last_status")):
            a = np.frombuffer(v, dtype=np.float64)
            if np.isnan(a).any() or np.isposinf(a).any():
                bad.append(k)
    return bad


class Walker(object):
    """One long-lived set of contexts (the context under test and its partners) and a factory of fresh sets for the references.
    `fresh(partners)` returns (ctx, p2, p3, close), p2 and p3 None unless `partners`.  References are cached by (problem key, call)."""

    def __init__(self, make, fresh, names=None, cache=None):
        self.ctx, self.p2, self.p3 = make()
        self.fresh, self.names = fresh, list(names or CALLS)
        self.cache = {} if cache is None else cache
        self.compared, self.refused = 0, set()

    def env(self, P):
        return Env(self.ctx, self.p2, self.p3, P)

    def reference(self, P, name):
        key = (P.key, name)
        if key not in self.cache:
            c, p2, p3, close = self.fresh(name in PARTNERED)
            try:
                e = Env(c, p2, p3, P)
                setup(e)
                self.cache[key] = run_call(name, e)
            finally:
                close()
        return self.cache[key]

    def fill(self, P, names=None):
        """Run the calls for their side effect on the buffers only (the poison); returns the results."""
        e = self.env(P)
        setup(e)
        out = {}
        for name in names or self.names:
            out[name] = run_call(name, e)
            if CALLS[name].mutates:
                setup(e)
        return out

    def compare(self, step, P, name, got):
        """`got`, the walker's result of `name` at P, against the fresh reference: the same bytes; a refusal exactly where
        expected_refusal says so; a finite reference otherwise."""
        want = self.reference(P, name)
        diff = first_difference(got, want)
        if diff is not None:
            raise Mismatch("step %r, call %r: %s" % (step, name, diff))
        code = expected_refusal(name, P)
        if is_refusal(want) != (code is not None) or (code is not None and want[1] != code):
            raise Mismatch("step %r, call %r: expected %s, the fresh context gave %r" % (
                step, name, "a result" if code is None else "refusal %d" % code, want if is_refusal(want) else "a result"))
        if is_refusal(want):
            self.refused.add((P.name.split("/")[0], name, want[1]))
        else:
            bad = all_finite(want)
            if bad:
                raise Mismatch("step %r, call %r: the reference is not finite in %s" % (step, name, bad))
        self.compared += 1

    def step(self, step, P, names=None, between=None):
        """Run the calls at P in order and compare each with its fresh reference; a difference raises Mismatch naming the step
        and the call.  between(walker, P) -> P', when given, runs between two calls and returns the problem as it then stands."""
        e = self.env(P)
        setup(e)
        for name in names or self.names:
            self.compare(step, P, name, run_call(name, e))
            if between is not None:
                P = between(self, P)
                e = self.env(P)
            elif CALLS[name].mutates:
                setup(e)
        return P
