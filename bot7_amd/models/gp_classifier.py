"""A probit Gaussian-process CLASSIFIER by Laplace's method behind the gp_regressor protocol: the model of a constraint that is
observed only as a binary outcome -- "the run failed here" -- with no value to regress on (Gelbart, Snoek & Adams 2014, section 2.3;
Rasmussen & Williams 2006, algorithms 3.1 / 3.2).  No counterpart in the reference's models/.

The response column holds labels, each exactly 0 or 1, 1 meaning the constraint is VIOLATED; Pr[label = 1 | h] = Phi(h) of a latent
GP h with the regressor's covariance kernels (config.kernel: 'ardse' | 'ardmatern52') and a constant prior mean.  Everything
numerical happens in libbot7hip.so (b7_clf_*: csrc/laplace.hip); nothing is computed here but Phi of two downloaded vectors in
predict.

Hyper vector: the regressor's, [ lenscale_sq_1 .. lenscale_sq_d, amp, noise, mean ].  noise is carried as 0 and ignored (the probit
link has unit variance); mean is the latent's prior mean.

Hyper sampling (config.sampler = 'slice'): the registered host slice sampler walks
    log p(theta | X, labels) = -nll(theta) + flat prior inside bounds,   theta = [log lenscale_sq, log amp, mean]
where nll is -log of Laplace's approximate evidence, one b7_clf_nll_batch per density evaluation (a whole Newton solve inside one
launch).  config.sampler = 'slice_device' and config.chains > 1 are not built for the classifier and are refused by name.  With
config.sample = False (default) sample_hypers returns the point estimate."""
import numpy as np

from .gp_regressor import gp_regressor


class gp_classifier(gp_regressor):
    title = "bot7.models.gp_classifier"

    def __init__(self, config=None, context=None):
        if "fit" in dict(config or {}):
            raise NotImplementedError("gp_classifier with config.fit = %r: gradients of the Laplace evidence are not built (the fit is the "
                                      "regressor's)" % (dict(config)["fit"],))
        super().__init__(config, context)
        if self.config.get("sampler", "slice") == "slice_device":
            raise NotImplementedError("gp_classifier with sampler 'slice_device': the classifier's chain on the device is not built "
                                      "(use sampler = 'slice')")
        if int(self.config.get("chains", 1)) > 1:
            raise NotImplementedError("gp_classifier with config.chains > 1: lock-step chains are not built for the classifier")

    # ---- hyper-parameters -------------------------------------------------------------------------
    @staticmethod
    def _labels(Y_obs, N):
        Y = np.asarray(Y_obs, dtype=np.float64).reshape(N, -1)
        if Y.shape[1] != 1:
            raise NotImplementedError("gp_classifier: %d response columns (one column of 0 / 1 labels is built)" % Y.shape[1])
        return Y

    def init(self, X_obs, Y_obs):
        """Point initialisation: lenscale_sq = d/8, amp = 1 (a latent of unit scale: probabilities between Phi(-1) and Phi(1) one
        prior standard deviation out), noise = 0, mean = Phi^-1 of the labels' smoothed rate (k + 1)/(N + 2)."""
        X = np.atleast_2d(np.asarray(X_obs, dtype=np.float64))
        Y = self._labels(Y_obs, X.shape[0])
        d = X.shape[1]
        from statistics import NormalDist
        mean = NormalDist().inv_cdf((float(Y.sum()) + 1.0) / (Y.shape[0] + 2.0))
        self.hyp = self.parse_hypers(np.concatenate([np.full(d, d / 8.0), [1.0, 0.0, mean]]))
        return self.hyp

    @staticmethod
    def _to_theta(h):
        return np.concatenate([np.log(h["lenscale_sq"]), [np.log(h["amp"]), h["mean"]]])

    @staticmethod
    def _from_theta(t):
        d = t.size - 2
        return {"lenscale_sq": np.exp(t[:d]), "amp": float(np.exp(t[d])), "noise": 0.0, "mean": float(t[d + 1])}

    def _bounds_compute(self, X, Y):
        """Flat bounds on [log lenscale_sq, log amp, mean] (config.bounds overrides): the regressor's lengthscale box, a latent
        amplitude between 1e-2 and 1e2 (Phi saturates beyond) and a prior mean within four units of zero."""
        b = self.config.get("bounds") or {}
        d = X.shape[1]
        lo = np.concatenate([np.full(d, np.log(b.get("lenscale_sq_min", 1e-3 * d))), [np.log(b.get("amp_min", 1e-2)), b.get("mean_min", -4.0)]])
        hi = np.concatenate([np.full(d, np.log(b.get("lenscale_sq_max", 1e3 * d))), [np.log(b.get("amp_max", 1e2)), b.get("mean_max", 4.0)]])
        return lo, hi

    def log_posterior(self, theta, X_obs, Y_obs):
        theta = np.asarray(theta, dtype=np.float64).ravel()
        X = np.atleast_2d(np.asarray(X_obs, dtype=np.float64))
        return self._density(X, self._labels(Y_obs, X.shape[0]))(theta, None)

    def _density(self, X, Y):
        """The sampler's density for one update: -nll on the device inside the bounds, -inf outside."""
        lo, hi = self._bounds(X, Y)
        self._make_resident(X, Y)
        ctx = self.ctx

        def f(t, _args):
            t = np.asarray(t, dtype=np.float64).ravel()
            if not ((t >= lo) & (t <= hi)).all():      # also NaN: it fails both comparisons
                return -np.inf
            self.nEvals = getattr(self, "nEvals", 0) + 1
            nll, iters, info = ctx.clf_nll_batch([self._from_theta(t)], want_info=True)
            self.last_fit = {"nll": float(nll[0]), "iters": int(iters[0]), "info": int(info[0])}
            return -float(nll[0])
        return f

    def sample_hypers(self, X_obs, Y_obs, _a=None, _b=None, state=None):
        """model:sample_hypers(X, labels[, nil, nil, true]) -> flat hyper vector, as gp_regressor.sample_hypers on the host sampler."""
        X = np.atleast_2d(np.asarray(X_obs, dtype=np.float64))
        Y = self._labels(Y_obs, X.shape[0])
        if self.hyp is None:
            self.init(X, Y)
        if self.config.get("sample"):
            Samplers = self._samplers()
            if getattr(self, "_sampler", None) is None:
                self._sampler = Samplers[self.config.get("sampler", "slice")]()
                self._sopt = self._sampler.configure(dict(self.config.get("sampler_opt") or {}, seed=self.config.get("seed", 0)))
                self._sopt.setdefault("width", 0.5)
            kept = getattr(self, "_chain_state", None)
            theta = kept[0] if kept is not None and kept[1] is self.hyp else self._to_theta(self.hyp)
            lo, hi = self._bounds(X, Y)
            theta = np.clip(theta, lo, hi)
            n_updates = 1 if state else int(self.config.get("nBurnin", 0))
            f = self._density(X, Y)
            for _ in range(n_updates):
                theta = self._sampler.sample(f, theta.reshape(1, -1), dict(self._sopt, nSamples=1), None)[0]
            self.hyp = self._from_theta(np.asarray(theta, dtype=np.float64))
            self._chain_state = (theta, self.hyp)
        h = self.hyp
        return np.concatenate([h["lenscale_sq"], [h["amp"], h["noise"], h["mean"]]])

    def nll(self, X_obs, Y_obs, hyp=None):
        """-log of Laplace's approximate evidence of the labels under hyp (b7_clf_nll_batch)."""
        hyp = hyp or self.hyp
        X = np.atleast_2d(np.asarray(X_obs, dtype=np.float64))
        Y = self._labels(Y_obs, X.shape[0])
        self._make_resident(X, Y)
        nll, iters, info = self.ctx.clf_nll_batch([hyp], want_info=True)
        self.last_fit = {"nll": nll, "iters": int(iters[0]), "info": int(info[0])}
        return nll

    # ---- posterior ---------------------------------------------------------------------------------
    def fit(self, X_obs, Y_obs, hyp=None):
        """One Laplace fit into the context's fit slot (b7_clf_fit_hyp); there is no rank-one append for a classifier."""
        hyp = hyp or self.hyp
        if hyp is None:
            hyp = self.init(X_obs, Y_obs)
        X = np.atleast_2d(np.asarray(X_obs, dtype=np.float64))
        Y = self._labels(Y_obs, X.shape[0])
        self._make_resident(X, Y)
        self.last_fit = self.ctx.clf_fit_hyp(hyp["lenscale_sq"], hyp["amp"], 0.0, hyp["mean"])
        return self.last_fit

    def predict(self, X_obs, Y_obs, X_hid, hyp=None, req=None):
        """Pr[violated | x] at the rows of X_hid under hyp: Phi(mu / sqrt(var + 1)) of the latent posterior, the probit likelihood
        averaged over it.  Returns {'mean': M x 1 probabilities, 'var': M latent variances, 'latent': M x 1 latent means}."""
        self.fit(X_obs, Y_obs, hyp)
        if self._is_resident(X_hid):
            mu, var = self.ctx.gp_predict(download=True)
        else:
            mu, var = self.ctx.gp_predict_at(np.atleast_2d(np.asarray(X_hid, dtype=np.float64)))
        import math
        ndtr = np.vectorize(lambda z: 0.5 * math.erfc(-z * 0.7071067811865476), otypes=[np.float64])
        mu = np.asarray(mu, dtype=np.float64).reshape(-1, 1)
        req = req or {"mean": True, "var": True}
        out = {"latent": mu}
        if req.get("mean"):
            out["mean"] = ndtr(mu / np.sqrt(np.asarray(var, dtype=np.float64).reshape(-1, 1) + 1.0))
        if req.get("var"):
            out["var"] = var
        return out

    def predict_device(self, X_obs, Y_obs, X_hid, hyp=None):
        raise NotImplementedError("gp_classifier.predict_device: a classifier feeds no acquisition score; its log feasibility over the "
                                  "resident grid is Context.clf_eval_logfeas")

    def fantasize(self, nFantasies, X_obs, Y_obs, X_pend, hyp=None):
        raise NotImplementedError("gp_classifier.fantasize: fantasies of binary outcomes are not built")
