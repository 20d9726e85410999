--[[
Drop-ins for bot7.scores.expected_improvement / confidence_bound (scores/*.lua) backed by b7_score_*.
Register:  local S = require('bot7hip.scores_hip')
           bot7.scores.expected_improvement = S.expected_improvement ; bot7.scores.confidence_bound = S.confidence_bound
S.max_value_entropy_search has no original either (b7_score_mes; Wang & Jegelka, ICML 2017): register it as a new score.
S.log_probability_of_improvement has no original either (b7_score_logpi): log Phi(z), a constraint's log probability of feasibility.
S.log_expected_improvement has no original to replace: log-space EI (b7_score_logei; Ament et al., NeurIPS 2023), which still
ranks the candidates where EI has underflowed to 0.  Register it as a new score: bot7.scores.log_expected_improvement = ...
They return the M-element score tensor like the originals (bots/bayesopt.lua:76 adds it); with a gp_hip model the
posterior never leaves the GPU between predict and score.  Mirrors bot7_amd/scores/*.py.
--]]
local ffi = require('ffi')
local hip = require('bot7hip.bot7hip_ffi')
local S   = {}

local function finish(M)
  local out = torch.DoubleTensor(M)
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  hip.check(hip.C.b7_score_finish(hip.ctx, 1.0, v, i, torch.data(out)))
  return out
end

do
  local EI, parent = torch.class('bot7.scores.expected_improvement_hip', 'bot7.scores.abstract')
  function EI:__init(config)
    parent.__init(self)
    local config = config or {}
    config['tradeoff']   = config.tradeoff or 0.0     -- scores/expected_improvement.lua:30
    config['nFantasies'] = config.nFantasies or 100   -- :31
    self.config = config
  end
  function EI:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    local hyp, config = hyp or model.hyp, config or self.config
    local X_obs, Y_obs = X_obs, Y_obs
    if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
    -- fantasize outcomes for pending jobs and append them to the _obs tensors (:51-60)
    if torch.isTensor(X_pend) and X_pend:dim() > 0 and X_pend:size(1) > 0 then
      if X_pend:dim() == 1 then X_pend = X_pend:view(1, -1) end
      local Y_pend = model:fantasize(config.nFantasies, X_obs, Y_obs, X_pend, hyp)   -- nPend x nFantasies, :57
      X_obs = X_obs:cat(X_pend, 1)                                                     -- :58
      Y_obs = Y_obs:narrow(2, 1, 1):repeatTensor(1, config.nFantasies):cat(Y_pend, 1)  -- :59
    end
    model:predict_device(X_obs, Y_obs, X_hid, hyp)                                   -- :63
    local fmins = hip.pin(Y_obs:min(1):view(-1))                                     -- :64
    hip.check(hip.C.b7_score_reset(hip.ctx))
    hip.check(hip.C.b7_score_ei(hip.ctx, hip.data(fmins), config.tradeoff or 0.0))   -- :69-88 (row mean when > 1 column)
    return finish(X_hid:size(1))
  end
  S.expected_improvement = EI
end

do
  -- log EI = log(sigma) + log(phi(z) + z Phi(z)); config and the pending-points branch are EI's own.  The tensor it returns
  -- holds LOGARITHMS: a host-side marginalisation (bots/bayesopt.lua:76-79 score:add / score:div) would average logs, so
  -- this score is meant for the fused nomination (bots_bayesopt_hip), which marginalises by log-sum-exp on the device and
  -- never calls this method.  A call from anywhere else says so once, on stderr
  local warned = false
  local LEI, parent = torch.class('bot7.scores.log_expected_improvement_hip', 'bot7.scores.abstract')
  function LEI:__init(config)
    parent.__init(self)
    local config = config or {}
    config['tradeoff']   = config.tradeoff or 0.0
    config['nFantasies'] = config.nFantasies or 100
    self.config = config
  end
  function LEI:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    if not warned then
      warned = true
      io.stderr:write('bot7.scores.log_expected_improvement_hip: returning LOG scores; averaging them over hyper samples on the ',
                      'host (bot7.bots.bayesopt) is not the marginal EI: use bot7.bots.bayesopt_hip, or nSamples = 1\n')
    end
    local hyp, config = hyp or model.hyp, config or self.config
    local X_obs, Y_obs = X_obs, Y_obs
    if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
    if torch.isTensor(X_pend) and X_pend:dim() > 0 and X_pend:size(1) > 0 then
      if X_pend:dim() == 1 then X_pend = X_pend:view(1, -1) end
      local Y_fant = model:fantasize(config.nFantasies, X_obs, Y_obs, X_pend, hyp)
      Y_obs = Y_obs:narrow(2, 1, 1):repeatTensor(1, config.nFantasies)
      Y_obs = Y_obs:cat(Y_fant, 1)
      X_obs = X_obs:cat(X_pend, 1)
    end
    model:predict_device(X_obs, Y_obs, X_hid, hyp)
    local fmins = hip.pin(Y_obs:min(1):view(-1))
    hip.check(hip.C.b7_score_reset(hip.ctx))
    hip.check(hip.C.b7_score_logei(hip.ctx, hip.data(fmins), config.tradeoff or 0.0))   -- the log of the row mean when > 1 column
    return finish(X_hid:size(1))
  end
  S.log_expected_improvement = LEI
end

do
  -- log PI = log Phi(z) (b7_score_logpi; no original).  On a constraint's model, with Y_obs' minimum replaced by the threshold
  -- (config.threshold) and tradeoff 0, it is that constraint's log probability of feasibility: what bots_bayesopt_hip's
  -- nominate_constrained adds onto the feasibility column.  A LOG score like log EI: meant for the fused nomination, which
  -- marginalises by log-sum-exp on the device.  No pending points: one response column
  local LPI, parent = torch.class('bot7.scores.log_probability_of_improvement_hip', 'bot7.scores.abstract')
  function LPI:__init(config)
    parent.__init(self)
    local config = config or {}
    config['tradeoff'] = config.tradeoff or 0.0
    self.config = config
  end
  function LPI:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    local hyp, config = hyp or model.hyp, config or self.config
    if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
    assert(not (torch.isTensor(X_pend) and X_pend:dim() > 0 and X_pend:size(1) > 0),
           'log_probability_of_improvement_hip: pending points (fantasies) are not supported')
    model:predict_device(X_obs, Y_obs, X_hid, hyp)
    local fmins = hip.pin(config.threshold and torch.Tensor{config.threshold} or Y_obs:min(1):view(-1))
    hip.check(hip.C.b7_score_reset(hip.ctx))
    hip.check(hip.C.b7_score_logpi(hip.ctx, hip.data(fmins), config.tradeoff or 0.0))
    return finish(X_hid:size(1))
  end
  S.log_probability_of_improvement = LPI
end

do
  -- max-value entropy search (Wang & Jegelka, ICML 2017; b7_score_mes): K = config.nLevels quantiles of the grid MINIMUM's
  -- distribution under this hyper sample are found on the device, then score = mean_k h((mu - y*_k)/sigma).  A linear score:
  -- the host-side marginalisation (bots/bayesopt.lua:76-79) averages it as it averages EI.  No pending points: one response column
  local MES, parent = torch.class('bot7.scores.max_value_entropy_search_hip', 'bot7.scores.abstract')
  function MES:__init(config)
    parent.__init(self)
    local config = config or {}
    config['nLevels'] = config.nLevels or 8
    self.config = config
  end
  function MES:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    local hyp, config = hyp or model.hyp, config or self.config
    if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
    assert(not (torch.isTensor(X_pend) and X_pend:dim() > 0 and X_pend:size(1) > 0),
           'max_value_entropy_search_hip: pending points (fantasies) are not supported')
    model:predict_device(X_obs, Y_obs, X_hid, hyp)
    hip.check(hip.C.b7_mes_set_levels(hip.ctx, config.nLevels or 8))
    hip.check(hip.C.b7_score_reset(hip.ctx))
    hip.check(hip.C.b7_score_mes(hip.ctx))
    return finish(X_hid:size(1))
  end
  S.max_value_entropy_search = MES
end

do
  -- Thompson sampling (b7_ts_nominate; no original): not a per-point score.  The class only carries config.nFeatures to
  -- bots_bayesopt_hip.lua, whose nominate / nominate_batch call the library in place of eval + arg-max.  With config.bot.objectives
  -- (two or three objectives, any batch) its nominate_objectives_ts keeps every objective's paths (b7_ts_paths) and nominates by the
  -- hypervolume improvement of their values (b7_ts_hvi_nominate / b7_ts_hvi3_nominate).  Checked by the static checker only (no
  -- LuaJIT / Torch7 in the pipeline).
  local TS, parent = torch.class('bot7.scores.thompson_sampling_hip', 'bot7.scores.abstract')
  function TS:__init(config)
    parent.__init(self)
    local config = config or {}
    config['nFeatures'] = config.nFeatures or 1024
    self.config = config
  end
  function TS:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    error('thompson_sampling_hip is not a per-point score: nominate through bot7.bots.bayesopt_hip (b7_ts_nominate)')
  end
  S.thompson_sampling = TS
end

do
  -- Constrained Thompson sampling (b7_ts_paths + b7_ts_feas_nominate; no original; the selection rule of SCBO, Eriksson & Poloczek
  -- 2021): not a per-point score.  The class only carries config.nFeatures to bots_bayesopt_hip.lua, whose nominate_constrained_ts
  -- keeps the paths of the objective and of every constraint and nominates feasible-first.  Checked by the static checker only.
  local CTS, parent = torch.class('bot7.scores.constrained_thompson_sampling_hip', 'bot7.scores.abstract')
  function CTS:__init(config)
    parent.__init(self)
    local config = config or {}
    config['nFeatures'] = config.nFeatures or 1024
    self.config = config
  end
  function CTS:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    error('constrained_thompson_sampling_hip is not a per-point score: nominate through bot7.bots.bayesopt_hip (b7_ts_feas_nominate)')
  end
  S.constrained_thompson_sampling = CTS
end

do
  -- The knowledge gradient (b7_kg_nominate; no original): not a per-point score either -- it needs the posterior covariance against
  -- its discretisation set.  The class carries config.points / discretisation / nFeatures to bots_bayesopt_hip.lua, whose
  -- nominate calls the library in place of eval + arg-max.  Checked by the static checker only.
  local KG, parent = torch.class('bot7.scores.knowledge_gradient_hip', 'bot7.scores.abstract')
  function KG:__init(config)
    parent.__init(self)
    local config = config or {}
    config['points']         = config.points or 16
    config['discretisation'] = config.discretisation or 'mean'
    config['nFeatures']      = config.nFeatures or 1024
    self.config = config
  end
  function KG:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    error('knowledge_gradient_hip is not a per-point score: nominate through bot7.bots.bayesopt_hip (b7_kg_nominate)')
  end
  S.knowledge_gradient = KG
end

do
  -- The exact two-objective expected hypervolume improvement (b7_ehvi_nominate; no original): not a per-point score of one posterior
  -- -- it needs the kept posteriors of two objectives, a front and a reference point.  bots_bayesopt_hip.lua's nominate_objectives
  -- calls the library in place of eval + arg-max (config.bot.objectives); with config.bot.objectives.models it hands over to
  -- nominate_objectives3 (three objectives, b7_ehvi3_nominate).  Checked by the static checker only.
  local EHVI, parent = torch.class('bot7.scores.expected_hypervolume_improvement_hip', 'bot7.scores.abstract')
  function EHVI:__init(config)
    parent.__init(self)
    self.config = config or {}
  end
  function EHVI:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    error('expected_hypervolume_improvement_hip is not a per-point score: nominate through bot7.bots.bayesopt_hip (b7_ehvi_nominate)')
  end
  S.expected_hypervolume_improvement = EHVI
end

do
  -- The same policy by the log score (b7_logehvi_nominate / b7_logehvi3_nominate; no original): it still ranks the candidates where
  -- the linear score is 0 in every row.  nominate_objectives / nominate_objectives3 tell the two kinds apart by this class's name.
  local LogEHVI, parent = torch.class('bot7.scores.log_expected_hypervolume_improvement_hip', 'bot7.scores.abstract')
  function LogEHVI:__init(config)
    parent.__init(self)
    self.config = config or {}
  end
  function LogEHVI:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    error('log_expected_hypervolume_improvement_hip is not a per-point score: nominate through bot7.bots.bayesopt_hip (b7_logehvi_nominate)')
  end
  S.log_expected_hypervolume_improvement = LogEHVI
end

do
  local CB, parent = torch.class('bot7.scores.confidence_bound_hip', 'bot7.scores.abstract')
  function CB:__init(config)
    parent.__init(self)
    local config = config or {}
    config['tradeoff']   = config.tradeoff or 1.0     -- scores/confidence_bound.lua:31-34
    config['nFantasies'] = config.nFantasies or 100
    config['bound']      = config.bound or 'lower'
    config['sign']       = config.sign or -1.0
    self.config = config
  end
  -- the reference's fantasies block re-declares its locals (scores/confidence_bound.lua:56): pending points have no
  -- effect there, and none here
  function CB:__call__(model, hyp, X_obs, Y_obs, X_hid, X_pend, config)
    local hyp, config = hyp or model.hyp, config or self.config
    model:predict_device(X_obs, Y_obs, X_hid, hyp)                                 -- :63
    hip.check(hip.C.b7_score_reset(hip.ctx))
    hip.check(hip.C.b7_score_cb(hip.ctx, config.tradeoff or 1.0,
                                (config.bound:lower() == 'upper') and 1 or 0, config.sign or -1.0))  -- :70-94
    return finish(X_hid:size(1))
  end
  S.confidence_bound = CB
end

return S
