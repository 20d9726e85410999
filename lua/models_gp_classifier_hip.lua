--[[
A probit Gaussian-process CLASSIFIER by Laplace's method behind the gp_hip protocol: the model of a constraint that is observed
only as a binary outcome -- the run failed here -- with no value to regress on (Gelbart, Snoek & Adams 2014, section 2.3;
Rasmussen & Williams 2006, algorithms 3.1 / 3.2).  No counterpart in the reference's models/.
Register:  bot7.models.gp_classifier_hip = require('bot7hip.models_gp_classifier_hip')   (after bot7.models.gp_hip)
and name it as a binary constraint's model: config.bot.constraints[k] = {threshold = 0.5, binary = true, model = {...}}.
Mirrors bot7_amd/models/gp_classifier.py method for method (that file is what the tests drive); checked by the static checker only.

The response column holds labels, each exactly 0 or 1, 1 = VIOLATED; Pr[label = 1 | h] = Phi(h) of a latent GP h with gp_hip's
covariance kernels and a constant prior mean.  Hyper vector: gp_hip's, { lenscale_sq_1..d, amp, noise, mean }; noise is carried as 0
and ignored.  Hyper sampling (config.sample = true): the reference's own bot7.samplers.slice over
    log p(theta | X, labels) = -nll(theta) + flat prior inside bounds,   theta = { log lenscale_sq, log amp, mean }
with nll = -log of Laplace's approximate evidence, one b7_clf_nll_batch per density evaluation (a whole Newton solve inside one
launch).  config.sampler = 'slice_device' and config.chains > 1 are refused by name.
--]]
local ffi = require('ffi')
local hip = require('bot7hip.bot7hip_ffi')

local title  = 'bot7.models.gp_classifier_hip'
local parent = 'bot7.models.gp_hip'
local model, parent = torch.class(title, parent)

function model:__init(config)
  parent.__init(self, config)
  assert(self.config.sampler ~= 'slice_device', 'gp_classifier with sampler slice_device: the chain of a classifier on the device is not built (use sampler = slice)')
  assert((self.config.chains or 1) <= 1, 'gp_classifier with config.chains > 1: lock-step chains are not built for the classifier')
end

-- the inverse of Phi by bisection on erfc-free arithmetic is not worth a dependency: Acklam's rational approximation (1e-9
-- relative) is far inside what a starting point of a chain needs
local function inv_cdf(p)
  local a = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00}
  local b = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01}
  local c = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00}
  local d = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00}
  if p < 0.02425 then
    local q = math.sqrt(-2 * math.log(p))
    return (((((c[1]*q + c[2])*q + c[3])*q + c[4])*q + c[5])*q + c[6]) / ((((d[1]*q + d[2])*q + d[3])*q + d[4])*q + 1)
  elseif p > 1 - 0.02425 then
    local q = math.sqrt(-2 * math.log(1 - p))
    return -(((((c[1]*q + c[2])*q + c[3])*q + c[4])*q + c[5])*q + c[6]) / ((((d[1]*q + d[2])*q + d[3])*q + d[4])*q + 1)
  end
  local q = p - 0.5
  local r = q * q
  return (((((a[1]*r + a[2])*r + a[3])*r + a[4])*r + a[5])*r + a[6]) * q / (((((b[1]*r + b[2])*r + b[3])*r + b[4])*r + b[5])*r + 1)
end

function model:init(X_obs, Y_obs)
  local d, n = X_obs:size(2), Y_obs:size(1)
  self.hyp = {lenscale_sq = torch.DoubleTensor(d):fill(d / 8), amp = 1.0, noise = 0.0, mean = inv_cdf((Y_obs:sum() + 1) / (n + 2))}
  return self.hyp
end

local function to_theta(h)
  local d = h.lenscale_sq:nElement()
  local t = torch.DoubleTensor(d + 2)
  t:narrow(1, 1, d):copy(h.lenscale_sq):log()
  t[d+1] = math.log(h.amp); t[d+2] = h.mean
  return t
end
local function from_theta(t)
  local d = t:nElement() - 2
  return {lenscale_sq = t:narrow(1, 1, d):clone():exp(), amp = math.exp(t[d+1]), noise = 0.0, mean = t[d+2]}
end
function model:bounds(X, Y)
  local b, d = self.config.bounds or {}, X:size(2)
  local lo, hi = torch.DoubleTensor(d + 2), torch.DoubleTensor(d + 2)
  lo:narrow(1, 1, d):fill(math.log(b.lenscale_sq_min or 1e-3 * d)); hi:narrow(1, 1, d):fill(math.log(b.lenscale_sq_max or 1e3 * d))
  lo[d+1] = math.log(b.amp_min or 1e-2); hi[d+1] = math.log(b.amp_max or 1e2)
  lo[d+2] = b.mean_min or -4.0; hi[d+2] = b.mean_max or 4.0
  return lo, hi
end

-- B evidences at once (hyps: a Lua array of hyp tables): one launch of B workgroups, the current fit stays as it is
function model:nll_batch(X_obs, Y_obs, hyps)
  self:stage_data(X_obs, Y_obs)
  local B, keep = #hyps, {}
  local arr = ffi.new('b7_hyp[?]', B)
  for s, h in ipairs(hyps) do
    local ls = hip.pin(h.lenscale_sq)
    keep[s] = ls
    arr[s - 1].lenscale_sq, arr[s - 1].amp, arr[s - 1].noise, arr[s - 1].mean = hip.data(ls), h.amp, 0.0, h.mean
  end
  local out, iters, info = torch.DoubleTensor(B), ffi.new('int[?]', B), ffi.new('int[?]', B)
  hip.check(hip.C.b7_clf_nll_batch(hip.ctx, B, arr, torch.data(out), iters, info))
  self.last_fit = {iters = iters[B - 1], info = info[B - 1]}
  return out
end

function model:nll(X_obs, Y_obs, hyp)
  return self:nll_batch(X_obs, Y_obs, {hyp or self.hyp})[1]
end

function model:log_posterior(theta, X_obs, Y_obs)
  local theta = theta:view(-1)
  local lo, hi = self:bounds(X_obs, Y_obs)
  if theta:lt(lo):any() or theta:gt(hi):any() or theta:ne(theta):any() then return -math.huge end
  self.nEvals = self.nEvals + 1
  return -self:nll(X_obs, Y_obs, from_theta(theta))
end

function model:sample_hypers(X_obs, Y_obs, _, _, state)
  if not self.hyp then self:init(X_obs, Y_obs) end
  if self.config.sample then
    local Samplers = require('bot7.samplers')
    if not self.sampler then
      self.sampler = Samplers[self.config.sampler or 'slice']()
      self.sopt    = self.sampler.configure(self.config.sampler_opt or {})
      self.sopt.width = self.sopt.width or 0.5
    end
    local kept      = self._chain_state
    local theta     = (kept and kept.hyp == self.hyp) and kept.theta or to_theta(self.hyp)
    local lo, hi    = self:bounds(X_obs, Y_obs)
    theta = torch.cmin(torch.cmax(theta, lo), hi)
    local n_updates = state and 1 or (self.config.nBurnin or 0)
    local f = function(t, _) return self:log_posterior(t, X_obs, Y_obs) end
    self.sopt.nSamples = 1
    for _ = 1, n_updates do
      theta = self.sampler.sample(f, theta:view(1, -1), self.sopt, nil)[1]
    end
    self.hyp = from_theta(theta)
    self._chain_state = {theta = theta:clone(), hyp = self.hyp}
  end
  local h = self.hyp
  return torch.cat(h.lenscale_sq, torch.DoubleTensor{h.amp, h.noise, h.mean})
end

-- one Laplace fit into the context's fit slot: b7_gp_predict / b7_gp_predict_at then return the LATENT mean and variance
function model:fit(X_obs, Y_obs, hyp, want_nll)
  local hyp = hyp or self.hyp
  self:stage_data(X_obs, Y_obs)
  local ls = hip.pin(hyp.lenscale_sq)
  local h  = ffi.new('b7_hyp', {hip.data(ls), hyp.amp, 0.0, hyp.mean})
  local nll, iters, info = ffi.new('double[1]'), ffi.new('int[1]'), ffi.new('int[1]')
  hip.check(hip.C.b7_clf_fit_hyp(hip.ctx, h, nll, iters, info))
  self.last_fit = {iters = iters[0], info = info[0]}
  return nll[0]
end

-- Pr[violated | x] = Phi(mu / sqrt(var + 1)) of the latent posterior: {mean = M x 1 probabilities, var = M latent variances,
-- latent = M x 1 latent means}
function model:predict(X_obs, Y_obs, X_hid, hyp, req)
  local req = req or {mean = true, var = true}
  local out = parent.predict(self, X_obs, Y_obs, X_hid, hyp, {mean = true, var = true})
  local z   = torch.cdiv(out.mean:view(-1), torch.sqrt(out.var + 1))
  local p   = torch.erf(z * 0.7071067811865476):add(1):mul(0.5)
  return {mean = req.mean and p:view(-1, 1) or nil, var = req.var and out.var or nil, latent = out.mean}
end

function model:predict_device()
  error('gp_classifier.predict_device: a classifier feeds no acquisition score; its log feasibility over the resident grid is b7_clf_eval_logfeas')
end

function model:fantasize()
  error('gp_classifier.fantasize: fantasies of binary outcomes are not built')
end

return model
