--[[
bot7.bots.bayesopt with eval + nominate as ONE library call (b7_eval_nominate).

bots/bayesopt.lua:56-99 draws nSamples hyper vectors, adds one acquisition vector per sample on the host, divides,
and takes score:max(1).  With the *_hip model and scores that is nSamples fits + posteriors + score:adds on the GPU
and one M-vector download per sample.  This subclass keeps the sampling exactly as the parent does it (:68 burn-in
call, :74-75 per sample) but hands all nSamples hyper tables to the library at once: the fits, posteriors and
score:adds are enqueued back to back, the arg-max follows on the device (across GPUs when dist_hip has set up a
communicator), and the host waits once.  Nothing but the winner's index comes back.

Register:  bot7.bots.bayesopt = require('bot7hip.bots_bayesopt_hip')      -- or pass it as the bot class
Falls back to the parent's nominate whenever the model or score is not a *_hip one (e.g. DNGO).

Several GPUs, two layouts (INTEGRATION.md section 4):
  * ONE process, a group of GPUs (bot7hip_ffi.use_group{...}): self.candidates stays the reference's host tensor of ALL
    candidates, nominate's index is an index into it, and the parent's run_trial (bots/abstract.lua:112-152) runs
    unchanged -- the steal hook deletes the row on whichever GPU holds it.
  * one process per GPU (dist_hip.init): self.candidates is THIS RANK'S SHARD, nominate's index is 1-based in the UNION of
    the shards, and run_trial below replaces the parent's line 118 by dist_hip.commit; everything else is the parent's
    code.  The random initial picks (bots/bayesopt.lua:90-91) are drawn against the union's row count.
The harness's Python stand-in for this file is harness/bots/bayesopt.py + harness/dist.py.
--]]
local ffi = require('ffi')
local hip = require('bot7hip.bot7hip_ffi')
local D   = require('bot7hip.dist_hip')

local title  = 'bot7.bots.bayesopt_hip'
local parent = 'bot7.bots.bayesopt'
local bot, parent = torch.class(title, parent)

function bot:__init(objective, hypers, config, cache)
  parent.__init(self, objective, hypers, config, cache)
end

-- b7_score_spec of a *_hip score object, or nil when the score has no device form
local function score_spec(score, Y_obs, keep)
  local cfg, kind = score.config or {}, torch.type(score)
  if kind == 'bot7.scores.expected_improvement_hip' or kind == 'bot7.scores.log_expected_improvement_hip'
     or kind == 'bot7.scores.log_probability_of_improvement_hip' then
    local fmins = hip.pin(Y_obs:min(1):view(-1))            -- scores/expected_improvement.lua:64
    keep[#keep + 1] = fmins
    local code = (kind == 'bot7.scores.expected_improvement_hip') and hip.SCORE_EI or hip.SCORE_LOGEI   -- log-space EI: no original
    if kind == 'bot7.scores.log_probability_of_improvement_hip' then code = hip.SCORE_LOGPI end          -- log PI: no original
    return ffi.new('b7_score_spec', {code, cfg.tradeoff or 0.0, 0, 0.0, hip.data(fmins)})
  elseif kind == 'bot7.scores.max_value_entropy_search_hip' then   -- no original; one GPU only (a sharded grid answers "unsupported")
    hip.check(hip.C.b7_mes_set_levels(hip.ctx, cfg.nLevels or 8))
    return ffi.new('b7_score_spec', {hip.SCORE_MES, 0.0, 0, 0.0, nil})
  elseif kind == 'bot7.scores.confidence_bound_hip' then
    local upper = (string.lower(cfg.bound or 'lower') == 'upper') and 1 or 0   -- scores/confidence_bound.lua:72
    return ffi.new('b7_score_spec', {hip.SCORE_CB, cfg.tradeoff or 1.0, upper, cfg.sign or -1.0, nil})
  end
  return nil
end

-- Thompson sampling (b7_ts_nominate; no original): q pathwise posterior samples, path j under hyper sample j mod S, each path's
-- first minimum among the rows no earlier path took.  The seed comes from torch's generator, once per call.  One rank, no group.
-- Returns a LongTensor of q indices into `candidates` as it stands.
local function ts_nominate(self, q, candidates)
  assert(D.world == 1 and not hip.group, 'thompson_sampling: one rank, no group (sharded Thompson sampling is not built)')
  local model, keep = self.model, {}
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local X_obs, S = self.observed, self.config.bot.nSamples
  if torch.type(model) == 'bot7.models.dngo_hip' then
    -- the head's exact weight-space paths (b7_blr_ts_nominate): the point hyp table predict uses, or config.model.hyps, a list of them
    local hyps = (model.config or {}).hyps
                 or {model.blr_hyp or {alpha = 1.0, beta = 1.0 / (1e-2 * Y_obs:var()), mean = Y_obs:mean()}}
    local out, vmin = model:ts_nominate(X_obs, Y_obs, candidates, hyps, q, ffi.new('uint64_t', torch.random()))
    self.best_score = vmin
    return out
  end
  assert(torch.type(model) == 'bot7.models.gp_hip', 'thompson_sampling: needs the gp_hip or the dngo_hip model')
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  model:stage(X_obs, Y_obs, candidates)
  hip.set_kernel(model.kernel_code)
  local seed = ffi.new('uint64_t', torch.random())
  local v, i = ffi.new('double[?]', q), ffi.new('int64_t[?]', q)
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  hip.check(hip.C.b7_ts_nominate(hip.ctx, S, hyps, q, (self.score.config or {}).nFeatures or 1024, seed, v, i, jit, info))
  local out = torch.LongTensor(q)
  for k = 0, q - 1 do out[k + 1] = tonumber(i[k]) end
  self.best_score = v[0]
  return out
end

-- The knowledge gradient (b7_kg_nominate; no original): the row whose evaluation is expected to lower the minimum of the posterior
-- mean the most, over config.score.points discretisation rows (default 16).  config.score.discretisation = 'mean' (default): the
-- library takes the rows of lowest marginal mean; 'thompson': the minimisers of that many b7_ts_nominate paths under the same hyper
-- samples are handed over.  One rank, no group, no batch.  Returns a LongTensor of one index into `candidates` as it stands.
local function nominate_kg(self, candidates)
  assert(D.world == 1 and not hip.group, 'knowledge_gradient: one rank, no group (the knowledge gradient over a sharded grid is not built)')
  assert((self.config.bot.batch or 1) == 1, 'knowledge_gradient: config.bot.batch > 1 (knowledge-gradient batches are not built)')
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'knowledge_gradient: needs the gp_hip model')
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local X_obs, S = self.observed, self.config.bot.nSamples
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  model:stage(X_obs, Y_obs, candidates)
  hip.set_kernel(model.kernel_code)
  local cfg = self.score.config or {}
  local n = math.min(cfg.points or 16, hip.KG_MAX_POINTS, candidates:size(1))
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  local rows = nil
  if (cfg.discretisation or 'mean') == 'thompson' then
    local seed = ffi.new('uint64_t', torch.random())
    local pv = ffi.new('double[?]', n)
    rows = ffi.new('int64_t[?]', n)
    hip.check(hip.C.b7_ts_nominate(hip.ctx, S, hyps, n, cfg.nFeatures or 1024, seed, pv, rows, jit, info))
  else
    assert((cfg.discretisation or 'mean') == 'mean', "knowledge_gradient: config.score.discretisation is 'mean' or 'thompson'")
  end
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  hip.check(hip.C.b7_kg_nominate(hip.ctx, S, hyps, n, rows, v, i, jit, info))
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  self.best_score = v[0]
  return torch.LongTensor{tonumber(i[0])}
end

function bot:nominate(candidates)
  local candidates = candidates or self.candidates
  if self.config.bot.objectives then return self:nominate_objectives(candidates) end   -- two objectives: below
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91
    -- sharded one process per GPU: against the UNION's rows (every rank draws the same number from the same stream)
    local rows = (D.world > 1) and assert(D.M_global, 'dist_hip.shard_range first') or candidates:size(1)
    return torch.rand(1):mul(rows):long():add(1)
  end
  if torch.type(self.score) == 'bot7.scores.thompson_sampling_hip' then return ts_nominate(self, 1, candidates) end
  if torch.type(self.score) == 'bot7.scores.knowledge_gradient_hip' then return nominate_kg(self, candidates) end
  local model, keep = self.model, {}
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local spec = (torch.type(model) == 'bot7.models.gp_hip') and score_spec(self.score, Y_obs, keep) or nil
  if spec == nil then return parent.nominate(self, candidates) end

  local X_obs, S = self.observed, self.config.bot.nSamples
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls                                                     -- alive until the call has returned
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  if candidates ~= nil then
    model:stage(X_obs, Y_obs, candidates)                                    -- data + grid resident; uploads what changed
  else
    model:stage_data(X_obs, Y_obs)   -- this rank's shard has run empty: it still refits and takes part in the exchange
  end
  hip.set_kernel(model.kernel_code)   -- config.model.kernel on the context, or on every member of the group
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  if hip.group then   -- one process, several GPUs: i indexes self.candidates, the host tensor of all candidates
    hip.gcheck(hip.C.b7_group_eval_nominate(hip.group, S, hyps, spec, v, i, jit, info))
  else                -- i is 1-based in the union of the ranks' shards (= in self.candidates when there is one rank)
    hip.check(hip.C.b7_eval_nominate(hip.ctx, S, hyps, spec, D.lo, v, i, jit, info))   -- :76-79 + :96
  end
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  self.best_score = v[0]
  return torch.LongTensor{tonumber(i[0])}
end

-- q nominees from ONE library call (b7_eval_nominate_batch; no counterpart in the reference, whose bots nominate one point per
-- trial): nominate's pick, then q - 1 more by kriging-believer variance downdates, the rows already picked left out.  Returns a
-- LongTensor of q indices into `candidates` as it stands (the caller commits them: utils.tensor.steal takes an index list).
-- One rank, no group: sharded batches are not built.  config.bot.batch (default 1) is the q a driver passes; nominate_batch(1)
-- is nominate.
function bot:nominate_batch(q, candidates)
  local candidates = candidates or self.candidates
  q = q or self.config.bot.batch or 1
  if self.config.bot.objectives and torch.type(self.score) == 'bot7.scores.thompson_sampling_hip' then
    return self:nominate_objectives_ts(q, candidates)                        -- multi-objective Thompson sampling: below
  end
  if torch.type(self.score) == 'bot7.scores.constrained_thompson_sampling_hip' then
    return self:nominate_constrained_ts(q, candidates)                       -- constrained Thompson sampling: below
  end
  if q == 1 then return self:nominate(candidates) end
  assert(D.world == 1 and not hip.group, 'nominate_batch: one rank, no group (sharded batches are not built)')
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91, q distinct rows
    return torch.randperm(candidates:size(1)):narrow(1, 1, q):long()
  end
  if torch.type(self.score) == 'bot7.scores.thompson_sampling_hip' then return ts_nominate(self, q, candidates) end
  assert(torch.type(self.score) ~= 'bot7.scores.knowledge_gradient_hip', 'nominate_batch: knowledge-gradient batches are not built')
  local model, keep = self.model, {}
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local spec = (torch.type(model) == 'bot7.models.gp_hip') and score_spec(self.score, Y_obs, keep) or nil
  assert(spec ~= nil, 'nominate_batch: needs the gp_hip model and a *_hip score')
  local X_obs, S = self.observed, self.config.bot.nSamples
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  model:stage(X_obs, Y_obs, candidates)
  hip.set_kernel(model.kernel_code)
  local v, i = ffi.new('double[?]', q), ffi.new('int64_t[?]', q)
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  hip.check(hip.C.b7_eval_nominate_batch(hip.ctx, S, hyps, spec, q, v, i, jit, info))
  local out = torch.LongTensor(q)
  for k = 0, q - 1 do out[k + 1] = tonumber(i[k]) end
  self.best_score = v[0]
  return out
end

-- The nominee refined off the grid (b7_eval_nominate_refine; no counterpart in the reference's bots): nominate's pick, then
-- gradient ascent on the marginalised acquisition from config.bot.refine.starts grid rows for .iters iterations inside the grid's
-- box.  Returns the refined point (a d-vector) and the index into `candidates` of the row its start came from: the caller steals
-- that row, evaluates the objective at the point and observes the point.  One rank, no group, a gp_hip model and an EI / LogEI /
-- CB score: the library refuses the rest by name.
function bot:nominate_refine(candidates)
  local candidates = candidates or self.candidates
  assert(D.world == 1 and not hip.group, 'nominate_refine: one rank, no group (sharded refinement is not built)')
  local ref = self.config.bot.refine or {}
  local model, keep = self.model, {}
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local spec = (torch.type(model) == 'bot7.models.gp_hip') and score_spec(self.score, Y_obs, keep) or nil
  assert(spec ~= nil, 'nominate_refine: needs the gp_hip model and a *_hip score')
  local X_obs, S = self.observed, self.config.bot.nSamples
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  model:stage(X_obs, Y_obs, candidates)
  hip.set_kernel(model.kernel_code)
  local d = candidates:size(2)
  local opts = ffi.new('b7_refine_opts[1]')
  hip.check(hip.C.b7_refine_default_opts(opts))
  opts[0].starts = ref.starts or opts[0].starts
  opts[0].iters  = ref.iters or opts[0].iters
  opts[0].eta0   = ref.eta0 or opts[0].eta0
  local lo, hi = hip.pin(torch.Tensor(self.config.grid.mins)), hip.pin(torch.Tensor(self.config.grid.maxes))
  keep[#keep + 1], keep[#keep + 2] = lo, hi
  opts[0].lo, opts[0].hi = hip.data(lo), hip.data(hi)
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  local rv, ri = ffi.new('double[1]'), ffi.new('int64_t[1]')
  local x = torch.Tensor(d)
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  hip.check(hip.C.b7_eval_nominate_refine(hip.ctx, S, hyps, spec, opts, v, i, hip.data(x), rv, ri, jit, info))
  self.best_score = rv[0]
  return x, tonumber(ri[0])
end

-- q Thompson nominees refined off the grid by descent on their own sample paths (b7_ts_nominate_refine; no original): switched on by
-- config.score.refine = {starts, iters, eta0} under the thompson_sampling_hip score; config.bot.refine stays the per-point scores'.
-- lo / hi (d-vectors; nil: config.grid.mins / maxes) are the box, a trust-region driver passes its trial's.  Returns a LongTensor of
-- the q GRID NOMINEES' indices into `candidates` as it stands -- distinct by construction, whichever start won: the caller steals
-- those rows -- and the refined points (q x d), which it evaluates and observes.  One rank, no group, the gp_hip model, no
-- constraints or objectives: the rest is refused by name.
function bot:nominate_ts_refine(q, candidates, lo, hi)
  local candidates = candidates or self.candidates
  q = q or self.config.bot.batch or 1
  assert(D.world == 1 and not hip.group, 'nominate_ts_refine: one rank, no group (refinement of sample paths over a sharded grid is not built)')
  assert(torch.type(self.score) == 'bot7.scores.thompson_sampling_hip', 'nominate_ts_refine: config.score.refine refines thompson_sampling_hip nominees')
  assert(not self.config.bot.constraints and not self.config.bot.objectives,
         'nominate_ts_refine: refinement under constraints or several objectives is not built')
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_ts_refine: needs the gp_hip model (the dngo head\'s paths are not refined)')
  local ref = (self.score.config or {}).refine
  if type(ref) ~= 'table' then ref = {} end
  local Y_obs = self.responses
  if Y_obs:dim() == 1 then Y_obs = Y_obs:view(-1, 1) end
  local X_obs, S = self.observed, self.config.bot.nSamples
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps = ffi.new('b7_hyp[?]', S)
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
  end
  model:stage(X_obs, Y_obs, candidates)
  hip.set_kernel(model.kernel_code)
  local d = candidates:size(2)
  local opts = ffi.new('b7_refine_opts[1]')
  hip.check(hip.C.b7_refine_default_opts(opts))
  opts[0].starts = ref.starts or opts[0].starts
  opts[0].iters  = ref.iters or opts[0].iters
  opts[0].eta0   = ref.eta0 or opts[0].eta0
  local blo, bhi = hip.pin(lo or torch.Tensor(self.config.grid.mins)), hip.pin(hi or torch.Tensor(self.config.grid.maxes))
  keep[#keep + 1], keep[#keep + 2] = blo, bhi
  opts[0].lo, opts[0].hi = hip.data(blo), hip.data(bhi)
  local seed = ffi.new('uint64_t', torch.random())
  local v, i = ffi.new('double[?]', q), ffi.new('int64_t[?]', q)
  local rv, ri = ffi.new('double[?]', q), ffi.new('int64_t[?]', q)
  local x = torch.Tensor(q, d)
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  hip.check(hip.C.b7_ts_nominate_refine(hip.ctx, S, hyps, q, (self.score.config or {}).nFeatures or 1024, seed, opts, v, i,
                                        hip.data(x), rv, ri, jit, info))
  local out = torch.LongTensor(q)
  for k = 0, q - 1 do out[k + 1] = tonumber(i[k]) end
  self.best_score = rv[0]
  return out, x
end

-- S hyper tables of `model` over (X_obs, Y_obs) as a b7_hyp array, sampled as bots/bayesopt.lua:68,73-75 does
local function sample_hyps(model, X_obs, Y_obs, S, keep)
  model:sample_hypers(X_obs, Y_obs)                                          -- :68
  local hyps, tabs = ffi.new('b7_hyp[?]', S), {}
  for s = 1, S do                                                            -- :73-75
    local hyp = model:parse_hypers(model:sample_hypers(X_obs, Y_obs, nil, nil, true))
    local ls  = hip.pin(hyp.lenscale_sq)
    keep[#keep + 1] = ls
    hyps[s-1].lenscale_sq, hyps[s-1].amp, hyps[s-1].noise, hyps[s-1].mean = hip.data(ls), hyp.amp, hyp.noise, hyp.mean
    tabs[s] = hyp
  end
  return hyps, tabs   -- the array for the library, and the tables model:parse_hypers returned (a trust-region trial hands them out again)
end

-- fn() with the library's current context switched to a constraint's own, together with EVERY per-context cache bot7hip_ffi
-- keeps beside it: the "resident grid" record and the covariance kernel last set (hip.set_kernel skips the library when the
-- code equals its cache: with the objective's cache left in place a Matern constraint model on a new context, which starts
-- on ARD-SE, would never reach b7_gp_set_kernel)
local function on_context(con, fn)
  local ctx0, res0, ker0 = hip.ctx, hip.resident, hip.kernel
  hip.ctx, hip.resident, hip.kernel = con.ctx, con.resident, con.kernel
  local ok, err = pcall(fn)
  con.resident, con.kernel = hip.resident, hip.kernel
  hip.ctx, hip.resident, hip.kernel = ctx0, res0, ker0
  if not ok then error(err, 2) end
end

-- The driver has stolen the row this bot nominated last (bots/abstract.lua:118) and self.candidates is a NEW host tensor, one
-- row shorter: the same stable deletion on the constraint's context, whose "resident grid" record then names the new tensor, so
-- that model:stage uploads nothing (the steal hook does this for hip.ctx alone).  Anything else -- another shape, no nominee on
-- record -- forgets the record and the grid is uploaded again.
local function follow_steal(con, idx, candidates)
  local r = con.resident
  if r == nil then return end
  if idx ~= nil and candidates:isContiguous() and r.rows == candidates:size(1) + 1 and r.cols == candidates:size(2) then
    local arr = ffi.new('int64_t[1]', idx)
    hip.check(hip.C.b7_grid_remove_rows(con.ctx, arr, 1, nil))
    con.resident = {ptr = torch.data(candidates), rows = candidates:size(1), cols = candidates:size(2)}
  elseif not (r.rows == candidates:size(1) and r.ptr == torch.data(candidates)) then
    con.resident = nil
  end
end

-- CONSTRAINED nomination (b7_eval_nominate_feasible; no counterpart in the reference; Gelbart et al. 2014, Gardner et al. 2014):
-- config.bot.constraints = {{threshold = t_1, model = {...}}, ...}; the objective returns a row {y, c_1 .. c_C}; self.responses
-- keeps all 1 + C columns.  self.constraints[k] = {threshold, model (a gp_hip), ctx (a context of its own)} is set up on first
-- use.  Per model-based trial every constraint model samples its hypers and stages data and grid on ITS context, where
-- b7_eval_nominate(LogPI, fmin = t_k, tradeoff 0) leaves log Pr[c_k <= t_k] in the accumulator; the objective's context sums them
-- into its feasibility column (b7_feas_reset, b7_feas_add_acc) and nominates with the weight, fmin = the best response among the
-- rows that satisfy every constraint -- or by feasibility alone (b7_feas_nominate) while there is none.  The driver steals the
-- returned row from self.candidates (bots/abstract.lua:118: the contract follow_steal relies on); the next call deletes it from
-- every constraint context's grid before anything is staged there.  One rank, no group, EI / LogEI / LogPI; at parity with
-- harness/bots/bayesopt.py's nominate_constrained.
-- A constraint with binary = true is observed only as an outcome (0 satisfied, 1 violated; threshold 0.5): its model is a
-- gp_classifier_hip and b7_clf_eval_logfeas leaves the same log accumulator in place of b7_eval_nominate(LogPI).  With a binary
-- constraint present the rows whose objective is not finite (the run failed: there is no value) are left out of the OBJECTIVE
-- model's data; they stay in every constraint model's.
function bot:nominate_constrained(candidates)
  local candidates = candidates or self.candidates
  if torch.type(self.score) == 'bot7.scores.constrained_thompson_sampling_hip' then
    return self:nominate_constrained_ts(nil, candidates)                     -- constrained Thompson sampling: below
  end
  assert(D.world == 1 and not hip.group, 'nominate_constrained: one rank, no group (sharded constrained nomination is not built)')
  local cons = assert(self.config.bot.constraints, 'nominate_constrained: config.bot.constraints is not set')
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91
    return torch.rand(1):mul(candidates:size(1)):long():add(1)
  end
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_constrained: needs the gp_hip model')
  local R, S = self.responses, self.config.bot.nSamples
  local X_obs, Y_obs = self.observed, R:narrow(2, 1, 1):contiguous()
  if self.constraints == nil then
    self.constraints = {}
    for k, cfg in ipairs(cons) do
      local ctxp = ffi.new('b7_ctx*[1]')
      assert(hip.C.b7_create(ctxp, hip.device) == 0, 'nominate_constrained: b7_create failed')   -- the objective's device
      local mtype = (cfg.model or {}).type or (cfg.binary and 'gp_classifier' or 'gp_regressor')
      assert((cfg.binary and true or false) == (mtype == 'gp_classifier' or mtype == 'gp_classifier_hip'),
             'config.bot.constraints[' .. k .. ']: a binary constraint is modelled by a gp_classifier, and a gp_classifier models nothing else')
      assert(not cfg.binary or cfg.threshold == 0.5, 'config.bot.constraints[' .. k .. '] is binary: the labels are 0 and 1, threshold 0.5')
      local class = cfg.binary and bot7.models.gp_classifier_hip or bot7.models.gp_hip
      self.constraints[k] = {threshold = cfg.threshold, model = class(cfg.model), ctx = ffi.gc(ctxp[0], hip.C.b7_destroy),
                             binary = cfg.binary and true or false,
                             kernel = hip.KERNEL_ARDSE}   -- a new context starts on ARD-SE: the constraint's own kernel cache
    end
  end
  local feasible, binary = torch.ByteTensor(R:size(1)):fill(1), false
  for k, con in ipairs(self.constraints) do
    local C_obs = R:narrow(2, k + 1, 1):contiguous()
    feasible:cmul(C_obs:view(-1):le(con.threshold))
    binary = binary or con.binary
    follow_steal(con, self.constrained_idx, candidates)
    on_context(con, function()
      if not con.inited then con.model:init(X_obs, C_obs); con.inited = true end
      local hyps = sample_hyps(con.model, X_obs, C_obs, S, keep)
      con.model:stage(X_obs, C_obs, candidates)
      hip.set_kernel(con.model.kernel_code)
      local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
      if con.binary then                                                     -- the classifier's log Pr[feasible] in the accumulator
        hip.check(hip.C.b7_clf_eval_logfeas(hip.ctx, S, hyps, v, i, nil, nil))
      else
        local t = hip.pin(torch.Tensor{con.threshold})
        keep[#keep + 1] = t
        local spec = ffi.new('b7_score_spec', {hip.SCORE_LOGPI, 0.0, 0, 0.0, hip.data(t)})
        hip.check(hip.C.b7_eval_nominate(hip.ctx, S, hyps, spec, 0, v, i, nil, nil))
      end
    end)
  end
  -- the rows that reach the objective's model: all of them unless a binary constraint is present (a failed run has no objective)
  local Y_all, have_objective = Y_obs, true
  if binary then
    local finite = Y_obs:view(-1):eq(Y_obs:view(-1)):cmul(torch.abs(Y_obs:view(-1)):lt(math.huge))
    have_objective = finite:sum() > 0
    if have_objective and finite:sum() < Y_obs:size(1) then
      local rows = finite:nonzero():view(-1)
      X_obs, Y_obs = X_obs:index(1, rows), Y_obs:index(1, rows)
    end
  end
  local hyps
  if have_objective then
    hyps = sample_hyps(model, X_obs, Y_obs, S, keep)
    model:stage(X_obs, Y_obs, candidates)
  elseif not hip.is_resident(candidates) then
    hip.upload_grid(candidates)                                              -- feasibility alone: no objective model yet
  end
  hip.set_kernel(model.kernel_code)
  hip.check(hip.C.b7_feas_reset(hip.ctx))
  for _, con in ipairs(self.constraints) do hip.check(hip.C.b7_feas_add_acc(hip.ctx, con.ctx)) end
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  if feasible:sum() == 0 or not have_objective then                          -- Gelbart et al. 2014, section 3.2
    hip.check(hip.C.b7_feas_nominate(hip.ctx, v, i))
  else
    local Y_feas = Y_all:index(1, feasible:nonzero():view(-1))
    local spec = assert(score_spec(self.score, Y_feas, keep), 'nominate_constrained: needs a *_hip score')
    local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
    hip.check(hip.C.b7_eval_nominate_feasible(hip.ctx, S, hyps, spec, v, i, jit, info))
  end
  self.best_score = v[0]
  self.constrained_idx = tonumber(i[0])   -- what the driver steals next: follow_steal
  return torch.LongTensor{self.constrained_idx}
end

-- TWO-OBJECTIVE nomination (b7_ehvi_nominate; no counterpart in the reference; Emmerich, Yang & Deutz 2016):
-- config.bot.objectives = {ref = {r1, r2} | nil, model = {...}}, config.score.type = 'expected_hypervolume_improvement' (or
-- 'log_expected_hypervolume_improvement': the same trial by the log score, b7_logehvi_nominate / b7_logehvi3_nominate); the
-- objective returns a row {y1, y2}, both minimised; self.responses keeps both columns.  The bot's own model sees column 1,
-- self.objective2 = {model (a gp_hip), ctx (a context of its own)}, set up on first use, column 2.  Per model-based trial both
-- models sample their hypers and both contexts keep their posterior over the same grid rows (b7_eval_posterior); the front of the
-- observations under the reference point comes from b7_pareto_front2 and the objective's context nominates (b7_ehvi_nominate).
-- ref = nil: per column the maximum of the observations plus 10 % of the column's range (of max(|maximum|, 1) where there is no
-- range), recomputed every trial.  The driver steals the returned row from self.candidates (bots/abstract.lua:118); the next call
-- deletes it from the second context's grid before anything is staged there (follow_steal).  One rank, no group, no batch, no
-- refinement, no constraints; at parity with harness/bots/bayesopt.py's nominate_objectives.
function bot:nominate_objectives(candidates)
  local candidates = candidates or self.candidates
  assert(D.world == 1 and not hip.group, 'nominate_objectives: one rank, no group (two objectives over a sharded grid are not built)')
  local obj = assert(self.config.bot.objectives, 'nominate_objectives: config.bot.objectives is not set')
  if torch.type(self.score) == 'bot7.scores.thompson_sampling_hip' then      -- Thompson paths, two or three objectives, any batch: below
    return self:nominate_objectives_ts(self.config.bot.batch or 1, candidates)
  end
  if obj.models then return self:nominate_objectives3(candidates) end       -- {ref, models = {m2, m3}}: three objectives, below
  assert((self.config.bot.batch or 1) == 1, 'nominate_objectives: config.bot.batch > 1 (two-objective batches are not built)')
  assert(not self.config.bot.refine, 'nominate_objectives: config.bot.refine (refinement of a two-objective nominee is not built)')
  assert(not self.config.bot.constraints, 'nominate_objectives: config.bot.constraints (constraints combined with objectives are not built)')
  local logkind = torch.type(self.score) == 'bot7.scores.log_expected_hypervolume_improvement_hip'   -- the log score: b7_logehvi*_nominate
  assert(logkind or torch.type(self.score) == 'bot7.scores.expected_hypervolume_improvement_hip',
         'nominate_objectives: config.score.type must be expected_hypervolume_improvement or log_expected_hypervolume_improvement')
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91
    return torch.rand(1):mul(candidates:size(1)):long():add(1)
  end
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_objectives: needs the gp_hip model (the Bayesian-linear head is not built)')
  local R, S = self.responses, self.config.bot.nSamples
  assert(R:dim() == 2 and R:size(2) == 2, 'nominate_objectives: the objective must return rows of 2 columns {y1, y2}')
  local X_obs, Y1, Y2 = self.observed, R:narrow(2, 1, 1):contiguous(), R:narrow(2, 2, 1):contiguous()
  if self.objective2 == nil then
    local ctxp = ffi.new('b7_ctx*[1]')
    assert(hip.C.b7_create(ctxp, hip.device) == 0, 'nominate_objectives: b7_create failed')   -- the objective's device
    self.objective2 = {model = bot7.models.gp_hip(obj.model), ctx = ffi.gc(ctxp[0], hip.C.b7_destroy),
                       kernel = hip.KERNEL_ARDSE}   -- a new context starts on ARD-SE: the second objective's own kernel cache
  end
  local o2 = self.objective2
  local ref = hip.pin(torch.Tensor(2))
  keep[#keep + 1] = ref
  if obj.ref then
    ref[1], ref[2] = obj.ref[1], obj.ref[2]
  else
    local hi, lo = R:max(1):view(-1), R:min(1):view(-1)
    for k = 1, 2 do
      local span = hi[k] - lo[k]
      if not (span > 0) then span = math.max(math.abs(hi[k]), 1) end
      ref[k] = hi[k] + 0.1 * span
    end
  end
  local Rc = hip.pin(R:contiguous())
  keep[#keep + 1] = Rc
  local front, P = ffi.new('double[?]', 2 * math.max(1, math.min(R:size(1), hip.EHVI_PMAX))), ffi.new('int[1]')
  assert(hip.C.b7_pareto_front2(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P) == 0,
         'nominate_objectives: a front of more than EHVI_PMAX points, or a reference point that is not finite')
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  local hyps = sample_hyps(model, X_obs, Y1, S, keep)
  model:stage(X_obs, Y1, candidates)
  hip.set_kernel(model.kernel_code)
  hip.check(hip.C.b7_eval_posterior(hip.ctx, S, hyps, jit, info))
  follow_steal(o2, self.objectives_idx, candidates)
  on_context(o2, function()
    if not o2.inited then o2.model:init(X_obs, Y2); o2.inited = true end
    local hyps2 = sample_hyps(o2.model, X_obs, Y2, S, keep)
    o2.model:stage(X_obs, Y2, candidates)
    hip.set_kernel(o2.model.kernel_code)
    hip.check(hip.C.b7_eval_posterior(hip.ctx, S, hyps2, nil, nil))
  end)
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  if logkind then
    hip.check(hip.C.b7_logehvi_nominate(hip.ctx, o2.ctx, front, P[0], hip.data(ref), v, i))
  else
    hip.check(hip.C.b7_ehvi_nominate(hip.ctx, o2.ctx, front, P[0], hip.data(ref), v, i))
  end
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  self.best_score = v[0]
  self.objectives_idx = tonumber(i[0])   -- what the driver steals next: follow_steal
  return torch.LongTensor{self.objectives_idx}
end

-- THREE-OBJECTIVE nomination (b7_ehvi3_nominate; no counterpart in the reference): config.bot.objectives = {ref = {r1, r2, r3} | nil,
-- models = {{...}, {...}}}; the objective returns a row {y1, y2, y3}, all minimised.  The bot's own model sees column 1,
-- self.objectives23[k] = {model (a gp_hip), ctx (a context of its own)}, set up on first use, columns 2 and 3.  Per model-based trial
-- the three models sample their hypers and the three contexts keep their posterior over the same grid rows (b7_eval_posterior); the
-- front comes from b7_pareto_front3 and the objective's context nominates over the box decomposition (b7_ehvi3_nominate).  ref = nil:
-- as for two objectives, per column.  One rank, no group, no batch, no refinement, no constraints, no trust region; at parity with
-- harness/bots/bayesopt.py's nominate_objectives3.
function bot:nominate_objectives3(candidates)
  local candidates = candidates or self.candidates
  assert(D.world == 1 and not hip.group, 'nominate_objectives3: one rank, no group (three objectives over a sharded grid are not built)')
  local obj = assert(self.config.bot.objectives, 'nominate_objectives3: config.bot.objectives is not set')
  assert(type(obj.models) == 'table' and #obj.models == 2,
         'nominate_objectives3: config.bot.objectives.models holds two models, the second and the third objective (four or more objectives are not built)')
  assert((self.config.bot.batch or 1) == 1, 'nominate_objectives3: config.bot.batch > 1 (three-objective batches are not built)')
  assert(not self.config.bot.refine, 'nominate_objectives3: config.bot.refine (refinement of a three-objective nominee is not built)')
  assert(not self.config.bot.constraints, 'nominate_objectives3: config.bot.constraints (constraints combined with objectives are not built)')
  assert(not self.config.bot.trust_region, 'nominate_objectives3: config.bot.trust_region (three objectives inside a trust region are not built)')
  local logkind = torch.type(self.score) == 'bot7.scores.log_expected_hypervolume_improvement_hip'   -- the log score: b7_logehvi*_nominate
  assert(logkind or torch.type(self.score) == 'bot7.scores.expected_hypervolume_improvement_hip',
         'nominate_objectives3: config.score.type must be expected_hypervolume_improvement or log_expected_hypervolume_improvement')
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91
    return torch.rand(1):mul(candidates:size(1)):long():add(1)
  end
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_objectives3: needs the gp_hip model (the Bayesian-linear head is not built)')
  local R, S = self.responses, self.config.bot.nSamples
  assert(R:dim() == 2 and R:size(2) == 3, 'nominate_objectives3: the objective must return rows of 3 columns {y1, y2, y3}')
  local X_obs, Y1 = self.observed, R:narrow(2, 1, 1):contiguous()
  if self.objectives23 == nil then
    self.objectives23 = {}
    for k = 1, 2 do
      local ctxp = ffi.new('b7_ctx*[1]')
      assert(hip.C.b7_create(ctxp, hip.device) == 0, 'nominate_objectives3: b7_create failed')   -- the objective's device
      self.objectives23[k] = {model = bot7.models.gp_hip(obj.models[k]), ctx = ffi.gc(ctxp[0], hip.C.b7_destroy),
                              kernel = hip.KERNEL_ARDSE}
    end
  end
  local ref = hip.pin(torch.Tensor(3))
  keep[#keep + 1] = ref
  if obj.ref then
    ref[1], ref[2], ref[3] = obj.ref[1], obj.ref[2], obj.ref[3]
  else
    local hi, lo = R:max(1):view(-1), R:min(1):view(-1)
    for k = 1, 3 do
      local span = hi[k] - lo[k]
      if not (span > 0) then span = math.max(math.abs(hi[k]), 1) end
      ref[k] = hi[k] + 0.1 * span
    end
  end
  local Rc = hip.pin(R:contiguous())
  keep[#keep + 1] = Rc
  local front, P = ffi.new('double[?]', 3 * math.max(1, math.min(R:size(1), hip.EHVI3_PMAX))), ffi.new('int[1]')
  assert(hip.C.b7_pareto_front3(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P) == 0,
         'nominate_objectives3: a front of more than EHVI3_PMAX points, or a reference point that is not finite')
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  local hyps = sample_hyps(model, X_obs, Y1, S, keep)
  model:stage(X_obs, Y1, candidates)
  hip.set_kernel(model.kernel_code)
  hip.check(hip.C.b7_eval_posterior(hip.ctx, S, hyps, jit, info))
  for k = 1, 2 do
    local o, Yk = self.objectives23[k], R:narrow(2, k + 1, 1):contiguous()
    follow_steal(o, self.objectives_idx, candidates)
    on_context(o, function()
      if not o.inited then o.model:init(X_obs, Yk); o.inited = true end
      local hypsk = sample_hyps(o.model, X_obs, Yk, S, keep)
      o.model:stage(X_obs, Yk, candidates)
      hip.set_kernel(o.model.kernel_code)
      hip.check(hip.C.b7_eval_posterior(hip.ctx, S, hypsk, nil, nil))
    end)
  end
  local v, i = ffi.new('double[1]'), ffi.new('int64_t[1]')
  if logkind then
    hip.check(hip.C.b7_logehvi3_nominate(hip.ctx, self.objectives23[1].ctx, self.objectives23[2].ctx, front, P[0], hip.data(ref), v, i))
  else
    hip.check(hip.C.b7_ehvi3_nominate(hip.ctx, self.objectives23[1].ctx, self.objectives23[2].ctx, front, P[0], hip.data(ref), v, i))
  end
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  self.best_score = v[0]
  self.objectives_idx = tonumber(i[0])   -- what the driver steals next: follow_steal
  return torch.LongTensor{self.objectives_idx}
end

-- MULTI-OBJECTIVE THOMPSON SAMPLING (b7_ts_paths + b7_ts_hvi_nominate / b7_ts_hvi3_nominate; no counterpart in the reference; TSEMO:
-- Bradford, Schweidtmann & Lapkin 2018): config.score.type = 'thompson_sampling' with either config.bot.objectives form, any
-- config.bot.batch >= 1.  Per model-based trial every objective's model samples its hypers, stages its column on its own context and
-- keeps q sample paths (b7_ts_paths, a seed from torch's generator each, in objective order); the first context nominates: path j
-- takes the row whose sampled values improve the hypervolume of the observations' front plus the earlier picks under path j the most.
-- Returns a LongTensor of q indices into `candidates` as it stands; the driver steals them (utils.tensor.steal takes an index list)
-- and the next call deletes them from the other contexts' grids before anything is staged there.  One rank, no group, no refinement,
-- no constraints, no trust region; at parity with harness/bots/bayesopt.py's nominate_objectives_ts.
local function follow_steal_rows(con, idxs, candidates)
  local r = con.resident
  if r == nil then return end
  local n = idxs and idxs:nElement() or 0
  if n > 0 and candidates:isContiguous() and r.rows == candidates:size(1) + n and r.cols == candidates:size(2) then
    local arr = ffi.new('int64_t[?]', n)
    for k = 1, n do arr[k - 1] = idxs[k] end
    hip.check(hip.C.b7_grid_remove_rows(con.ctx, arr, n, nil))
    con.resident = {ptr = torch.data(candidates), rows = candidates:size(1), cols = candidates:size(2)}
  elseif not (r.rows == candidates:size(1) and r.ptr == torch.data(candidates)) then
    con.resident = nil
  end
end

function bot:nominate_objectives_ts(q, candidates)
  local candidates = candidates or self.candidates
  q = q or self.config.bot.batch or 1
  assert(D.world == 1 and not hip.group, 'nominate_objectives_ts: one rank, no group (objectives over a sharded grid are not built)')
  local obj = assert(self.config.bot.objectives, 'nominate_objectives_ts: config.bot.objectives is not set')
  local m = obj.models and 3 or 2
  assert(m == 2 or (type(obj.models) == 'table' and #obj.models == 2),
         'nominate_objectives_ts: config.bot.objectives.models holds two models, the second and the third objective (four or more objectives are not built)')
  assert(q >= 1 and q <= hip.BATCH_MAX, 'nominate_objectives_ts: config.bot.batch outside 1 .. BATCH_MAX')
  assert(not self.config.bot.refine, 'nominate_objectives_ts: config.bot.refine (refinement of a multi-objective nominee is not built)')
  assert(not self.config.bot.constraints, 'nominate_objectives_ts: config.bot.constraints (constraints combined with objectives are not built)')
  assert(not self.config.bot.trust_region, 'nominate_objectives_ts: config.bot.trust_region (objectives inside a trust region are not built)')
  assert(torch.type(self.score) == 'bot7.scores.thompson_sampling_hip', 'nominate_objectives_ts: config.score.type must be thompson_sampling')
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91, q distinct rows
    if q == 1 then return torch.rand(1):mul(candidates:size(1)):long():add(1) end
    return torch.randperm(candidates:size(1)):narrow(1, 1, q):long()
  end
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_objectives_ts: needs the gp_hip model (the Bayesian-linear head is not built)')
  local R, S = self.responses, self.config.bot.nSamples
  assert(R:dim() == 2 and R:size(2) == m, 'nominate_objectives_ts: the objective must return rows of one column per objective')
  local X_obs, Y1 = self.observed, R:narrow(2, 1, 1):contiguous()
  if self.objectives_ts == nil then
    self.objectives_ts = {}
    for k = 1, m - 1 do
      local ctxp = ffi.new('b7_ctx*[1]')
      assert(hip.C.b7_create(ctxp, hip.device) == 0, 'nominate_objectives_ts: b7_create failed')   -- the objective's device
      self.objectives_ts[k] = {model = bot7.models.gp_hip(m == 2 and obj.model or obj.models[k]), ctx = ffi.gc(ctxp[0], hip.C.b7_destroy),
                               kernel = hip.KERNEL_ARDSE}
    end
  end
  local others = self.objectives_ts
  local ref = hip.pin(torch.Tensor(m))
  keep[#keep + 1] = ref
  if obj.ref then
    for k = 1, m do ref[k] = obj.ref[k] end
  else
    local hi, lo = R:max(1):view(-1), R:min(1):view(-1)
    for k = 1, m do
      local span = hi[k] - lo[k]
      if not (span > 0) then span = math.max(math.abs(hi[k]), 1) end
      ref[k] = hi[k] + 0.1 * span
    end
  end
  local Rc = hip.pin(R:contiguous())
  keep[#keep + 1] = Rc
  local pmax = (m == 2) and hip.EHVI_PMAX or hip.EHVI3_PMAX
  local front, P = ffi.new('double[?]', m * math.max(1, math.min(R:size(1), pmax))), ffi.new('int[1]')
  if m == 2 then
    assert(hip.C.b7_pareto_front2(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P) == 0,
           'nominate_objectives_ts: a front of more than EHVI_PMAX points, or a reference point that is not finite')
  else
    assert(hip.C.b7_pareto_front3(hip.data(Rc), R:size(1), hip.data(ref), front, nil, P) == 0,
           'nominate_objectives_ts: a front of more than EHVI3_PMAX points, or a reference point that is not finite')
  end
  local F = (self.score.config or {}).nFeatures or 1024
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  -- every model samples its hypers and stages its column, in objective order ...
  local hyps = {}
  hyps[1] = sample_hyps(model, X_obs, Y1, S, keep)
  model:stage(X_obs, Y1, candidates)
  hip.set_kernel(model.kernel_code)
  for k = 1, m - 1 do
    local o, Yk = others[k], R:narrow(2, k + 1, 1):contiguous()
    follow_steal_rows(o, self.objectives_rows, candidates)
    on_context(o, function()
      if not o.inited then o.model:init(X_obs, Yk); o.inited = true end
      hyps[k + 1] = sample_hyps(o.model, X_obs, Yk, S, keep)
      o.model:stage(X_obs, Yk, candidates)
      hip.set_kernel(o.model.kernel_code)
    end)
  end
  -- ... then the paths, a seed each, in objective order, and the first context nominates
  local seeds = {}
  for k = 1, m do seeds[k] = ffi.new('uint64_t', torch.random()) end
  hip.check(hip.C.b7_ts_paths(hip.ctx, S, hyps[1], q, F, seeds[1], jit, info))
  for k = 1, m - 1 do
    hip.check(hip.C.b7_ts_paths(others[k].ctx, S, hyps[k + 1], q, F, seeds[k + 1], nil, nil))
  end
  local v, i, y = ffi.new('double[?]', q), ffi.new('int64_t[?]', q), ffi.new('double[?]', q * m)
  if m == 2 then
    hip.check(hip.C.b7_ts_hvi_nominate(hip.ctx, others[1].ctx, front, P[0], hip.data(ref), v, i, y))
  else
    hip.check(hip.C.b7_ts_hvi3_nominate(hip.ctx, others[1].ctx, others[2].ctx, front, P[0], hip.data(ref), v, i, y))
  end
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  local out = torch.LongTensor(q)
  for k = 0, q - 1 do out[k + 1] = tonumber(i[k]) end
  self.best_score = v[0]
  self.objectives_rows = out   -- what the driver steals next: follow_steal_rows
  return out
end

-- CONSTRAINED THOMPSON SAMPLING (b7_ts_paths + b7_ts_feas_nominate; no counterpart in the reference; the selection rule of SCBO:
-- Eriksson & Poloczek, AISTATS 2021): config.score.type = 'constrained_thompson_sampling' with config.bot.constraints, any
-- config.bot.batch from 1 to 16.  Per model-based trial the objective's model and every constraint's model sample their hypers and
-- stage their column on their own context, every context keeps q sample paths (a distinct seed from torch's generator each), and the
-- objective's context nominates: path j takes the row of lowest f_j among the rows where every c_kj <= t_k, or the row of smallest
-- total violation where its paths see no feasible row.  No fmin, no feasibility column.  Returns a LongTensor of q indices into
-- `candidates` as it stands; the driver steals them and the next call deletes them from the constraint contexts' grids before anything
-- is staged there (follow_steal_rows).  At parity with harness/bots/bayesopt.py's nominate_constrained_ts.  Checked by the static
-- checker only (no LuaJIT / Torch7 in the pipeline).
local function constrained_ts_refusal(self, q)
  local kind, b = 'constrained_thompson_sampling', self.config.bot
  if not b.constraints or #b.constraints == 0 then
    return kind .. ' without config.bot.constraints: the policy needs a constraint, each with a model of its own'
  end
  if b.refine then return kind .. ' with config.bot.refine: refinement of a constrained nominee is not built' end
  if b.objectives then return kind .. ' with config.bot.objectives: constraints combined with objectives are not built' end
  if b.trust_region then return kind .. ' with config.bot.trust_region: constraints inside a trust region (the outer loop of SCBO) are not built' end
  if D.world ~= 1 or hip.group then return kind .. ' over sharded candidates: constrained Thompson sampling over a sharded grid is not built' end
  if torch.type(self.model) == 'bot7.models.dngo_hip' then
    return kind .. ' with the dngo model: joint paths with the Bayesian-linear head are not built'
  end
  if torch.type(self.model) ~= 'bot7.models.gp_hip' then return kind .. ' needs the gp_hip model' end
  for k, cfg in ipairs(b.constraints) do
    if cfg.binary then
      return kind .. ' with config.bot.constraints[' .. k .. '] binary: sample paths of the latent of a classifier are not built (binary constraints nominate through the feasibility weight)'
    end
    local mtype = cfg.model and cfg.model.type or 'gp_regressor'
    if mtype ~= 'gp_regressor' and mtype ~= 'gp_hip' then
      return kind .. ' with config.bot.constraints[' .. k .. '] on the ' .. mtype .. ' model: a constraint is modelled by a gp_regressor'
    end
  end
  if #b.constraints > hip.TS_FEAS_CMAX then return kind .. ' with more than 8 constraints: at most 8 are built' end
  if q > hip.BATCH_MAX then return kind .. ' with config.bot.batch above 16: at most 16 nominees per trial are built' end
  return nil
end

function bot:nominate_constrained_ts(q, candidates)
  local candidates = candidates or self.candidates
  q = q or self.config.bot.batch or 1
  local why = constrained_ts_refusal(self, q)
  if why then error(why, 2) end
  local cons = self.config.bot.constraints
  if self.nTrials <= self.config.bot.nInitial then                          -- bots/bayesopt.lua:90-91, q distinct rows
    if q == 1 then return torch.rand(1):mul(candidates:size(1)):long():add(1) end
    return torch.randperm(candidates:size(1)):narrow(1, 1, q):long()
  end
  local model, keep = self.model, {}
  local R, S, C = self.responses, self.config.bot.nSamples, #cons
  assert(R:dim() == 2 and R:size(2) == 1 + C, 'nominate_constrained_ts: the objective must return rows {y, c_1 .. c_C}')
  local X_obs, Y1 = self.observed, R:narrow(2, 1, 1):contiguous()
  if self.constraints == nil then
    self.constraints = {}
    for k, cfg in ipairs(cons) do
      local ctxp = ffi.new('b7_ctx*[1]')
      assert(hip.C.b7_create(ctxp, hip.device) == 0, 'nominate_constrained_ts: b7_create failed')   -- the objective's device
      self.constraints[k] = {threshold = cfg.threshold, model = bot7.models.gp_hip(cfg.model), ctx = ffi.gc(ctxp[0], hip.C.b7_destroy),
                             kernel = hip.KERNEL_ARDSE}
    end
  end
  local F = (self.score.config or {}).nFeatures or 1024
  local jit, info = ffi.new('double[?]', S), ffi.new('int[?]', S)
  -- every model samples its hypers and stages its column, the objective first ...
  local hyps = {}
  hyps[1] = sample_hyps(model, X_obs, Y1, S, keep)
  model:stage(X_obs, Y1, candidates)
  hip.set_kernel(model.kernel_code)
  local ctxs, thr = ffi.new('b7_ctx*[?]', C), ffi.new('double[?]', C)
  for k, con in ipairs(self.constraints) do
    local Ck = R:narrow(2, k + 1, 1):contiguous()
    follow_steal_rows(con, self.constrained_rows, candidates)
    on_context(con, function()
      if not con.inited then con.model:init(X_obs, Ck); con.inited = true end
      hyps[k + 1] = sample_hyps(con.model, X_obs, Ck, S, keep)
      con.model:stage(X_obs, Ck, candidates)
      hip.set_kernel(con.model.kernel_code)
    end)
    ctxs[k - 1], thr[k - 1] = con.ctx, con.threshold
  end
  -- ... then the paths, a distinct seed each, and the objective's context nominates
  local seeds, seen = {}, {}
  while #seeds < 1 + C do
    local sd = torch.random()
    if not seen[sd] then seen[sd] = true; seeds[#seeds + 1] = ffi.new('uint64_t', sd) end
  end
  hip.check(hip.C.b7_ts_paths(hip.ctx, S, hyps[1], q, F, seeds[1], jit, info))
  for k, con in ipairs(self.constraints) do
    hip.check(hip.C.b7_ts_paths(con.ctx, S, hyps[k + 1], q, F, seeds[k + 1], nil, nil))
  end
  local key, cls, i = ffi.new('double[?]', q), ffi.new('int[?]', q), ffi.new('int64_t[?]', q)
  local y, reruns = ffi.new('double[?]', q * (1 + C)), ffi.new('int[1]')
  hip.check(hip.C.b7_ts_feas_nominate(hip.ctx, ctxs, thr, C, key, cls, i, y, reruns))
  for s = 0, S - 1 do
    if jit[s] > 0 then   -- the reference's warning text, utils/math.lua:210-212
      print(string.format('Warning: utils.math.chol succeeded in factorizing the\ninput matrix after applying a jitter of %.2e', jit[s]))
    end
  end
  local out = torch.LongTensor(q)
  for k = 0, q - 1 do
    assert(tonumber(i[k]) >= 1, 'nominate_constrained_ts: a path has a NaN in every row: nothing to nominate')
    out[k + 1] = tonumber(i[k])
  end
  self.best_score = key[0]
  self.constrained_reruns = reruns[0]
  self.constrained_rows = out   -- what the driver steals next: follow_steal_rows
  return out
end

-- ---- trust-region nomination (TuRBO-1: Eriksson, Pearce, Gardner, Turner & Poloczek, NeurIPS 2019; no original) --------------
-- config.bot.trust_region = nil (the reference's loop, untouched) or a table {length_init, length_min, length_max,
-- success_tolerance, failure_tolerance, perturb, base}; absent entries take the library's defaults (b7_tr_init), perturb
-- min(1, 20 / d), base config.grid.type.  config.grid.size is the number of candidates per trial: the grid is made per trial on
-- the device and never crosses to the host.  The box (b7_tr_box) and the counters that resize it (b7_tr_init, b7_tr_update) are
-- the library's own, shared with harness/bots/bayesopt.py, which this mirrors.

-- a fresh base grid of config.grid.size rows on the device, resident only; with mins / maxes mapped there by the generator
local function tr_base_grid(self, rec, mins, maxes)
  local M, d = self.config.grid.size, self.config.grid.dims
  hip.forget_resident()
  if rec.base == 'sobol' then   -- the sequence from point 1: the caller rotates it
    rec.skip = 1
    hip.check(hip.C.b7_grid_sobol(hip.ctx, M, d, 1, hip.data(mins), hip.data(maxes), nil))
  else                          -- a seed from torch's generator
    rec.base_seed = torch.random()
    hip.check(hip.C.b7_grid_random(hip.ctx, M, d, ffi.new('uint64_t', rec.base_seed), 0, hip.data(mins), hip.data(maxes), nil))
  end
end

-- rows idx (a LongTensor, 1-based) of the resident grid -> an idx:nElement() x d tensor; just those rows cross
local function tr_rows(idx, d)
  local out = torch.Tensor(idx:nElement(), d)
  for k = 1, idx:nElement() do
    local row = out:select(1, k)
    hip.check(hip.C.b7_grid_download(hip.ctx, idx[k] - 1, 1, torch.data(row)))
  end
  return out
end

-- One trial's nominees -> (rows q x d, the trial's trace record).  The first nInitial trials of a run and after a restart:
-- random rows of a fresh global base grid.  Afterwards: the hyper samples as sample_hyps draws them on the observations since the
-- last restart, the box around the best of those, a fresh base grid mapped into it on the device, and the nomination through
-- nominate_batch / nominate UNCHANGED on a resident-only handle -- they see the window as the observations and the trial's hyper
-- samples as their own draws.  No row is removed: the grid is discarded.  One rank, no group, a gp_hip model; no refinement, no
-- constraints, no second objective.
function bot:nominate_trust_region()
  local cfg, tr = self.config, self.config.bot.trust_region
  assert(D.world == 1 and not hip.group, 'nominate_trust_region: one rank, no group (the sharded trust-region loop is not built)')
  assert(not cfg.bot.refine, 'nominate_trust_region: config.bot.refine (refinement inside a trust region is not built)')
  assert(not cfg.bot.constraints, 'nominate_trust_region: config.bot.constraints (constraints inside a trust region are not built)')
  assert(not cfg.bot.objectives, 'nominate_trust_region: config.bot.objectives (two objectives inside a trust region are not built)')
  local model, keep = self.model, {}
  assert(torch.type(model) == 'bot7.models.gp_hip', 'nominate_trust_region: needs the gp_hip model (the box is shaped by ARD lengthscales)')
  local q, d, M, S = cfg.bot.batch or 1, cfg.grid.dims, cfg.grid.size, cfg.bot.nSamples
  local base = tr.base or cfg.grid.type or 'sobol'
  assert(base == 'sobol' or base == 'random', 'nominate_trust_region: config.bot.trust_region.base is sobol or random')
  assert(base ~= 'sobol' or d < 40, 'nominate_trust_region: the sobol base is built for fewer than 40 dimensions (base = random takes any)')
  local mins, maxes = hip.pin(torch.Tensor(cfg.grid.mins)), hip.pin(torch.Tensor(cfg.grid.maxes))
  if self.tr_state == nil then
    self.tr_state = ffi.new('b7_tr_state[1]')
    assert(hip.C.b7_tr_init(self.tr_state, d, q, tr.length_init or 0, tr.length_min or 0, tr.length_max or 0,
                            tr.success_tolerance or 0, tr.failure_tolerance or 0) == 0,
           'nominate_trust_region: length_min <= length_init <= length_max, all finite')
    self.tr_start, self.tr_since, self.tr_trace = 0, 0, {}
  end
  local rec = {trial = self.nTrials, length_before = self.tr_state[0].length, base = base, prob = tr.perturb or math.min(1, 20 / d),
               restart = false}
  if self.tr_since < cfg.bot.nInitial then                                   -- bots/bayesopt.lua:90-91 on a fresh global grid
    tr_base_grid(self, rec, mins, maxes)
    hip.resident_only(M, d)
    local idx
    if q == 1 then idx = torch.rand(1):mul(M):long():add(1) else idx = torch.randperm(M):narrow(1, 1, q):long() end
    rec.kind, rec.index = 'initial', idx
    return tr_rows(idx, d), rec
  end
  local n = self.observed:size(1) - self.tr_start
  local R = self.responses
  if R:dim() == 1 then R = R:view(-1, 1) end
  local X_win, Y_win = self.observed:narrow(1, self.tr_start + 1, n), R:narrow(1, self.tr_start + 1, n)
  local hyps, tabs = sample_hyps(model, X_win, Y_win, S, keep)
  local col, at, low = Y_win:select(2, 1), 1, math.huge                      -- the best row since the restart: the first of equals,
  for k = 1, n do                                                            -- and a NaN response never is the best
    if col[k] < low then at, low = k, col[k] end
  end
  local center = hip.pin(X_win:select(1, at):clone())
  local lo, hi = torch.Tensor(d), torch.Tensor(d)
  assert(hip.C.b7_tr_box(d, S, hyps, hip.data(center), self.tr_state[0].length, hip.data(mins), hip.data(maxes), hip.data(lo),
                         hip.data(hi)) == 0, 'nominate_trust_region: b7_tr_box refused the hyper samples, the bounds or the center')
  tr_base_grid(self, rec, nil, nil)
  local shift = nil
  if base == 'sobol' then shift = torch.rand(d) end                          -- a fresh Cranley-Patterson rotation per trial
  rec.map_seed = torch.random()
  hip.check(hip.C.b7_grid_trust_region(hip.ctx, hip.data(center), hip.data(lo), hip.data(hi), rec.prob, hip.data(shift),
                                       ffi.new('uint64_t', rec.map_seed), 0))
  local grid = hip.resident_only(M, d)
  -- the existing nominations, unchanged: the window as the observations, the hyper samples above as their draws
  local obs0, resp0, handed = self.observed, self.responses, 0
  self.observed, self.responses = X_win, Y_win
  model.sample_hypers = function() return nil end
  model.parse_hypers  = function() handed = handed % S + 1; return tabs[handed] end
  local ok, idx = pcall(function() return self:nominate_batch(q, grid) end)
  model.sample_hypers, model.parse_hypers = nil, nil                         -- the class's methods again
  self.observed, self.responses = obs0, resp0
  if not ok then error(idx, 2) end
  rec.kind, rec.index, rec.center, rec.lo, rec.hi, rec.shift, rec.hyps = 'model', idx, center, lo, hi, shift, tabs
  return tr_rows(idx, d), rec
end

-- bots/abstract.lua:112-152 with the candidates made per trial inside the trust region: nothing is stolen, the q nominees are
-- evaluated and observed (:124-144), their responses resize the region (b7_tr_update), and a restart moves the model's window
-- (self.tr_start) -- observed / responses / best stay the run's record.  self.tr_trace keeps a record per trial.
function bot:run_trial_trust_region()
  self.nTrials = self.nTrials + 1                                            -- :114
  local rows, rec = self:nominate_trust_region()                             -- :117
  local q, ys = rows:size(1), nil
  for k = 1, q do
    local y = self.objective(rows:select(1, k))                              -- :124
    if not torch.isTensor(y) then                                            -- :127-133
      if type(y) == 'number' then y = torch.Tensor{{y}} elseif type(y) == 'table' then y = torch.Tensor(y) end
    end
    if y:dim() == 1 then y:resize(y:nElement(), 1) end                       -- :134
    if ys == nil then ys = y else ys = ys:cat(y, 1) end
  end
  if self.responses == nil then self.responses = ys else self.responses = self.responses:cat(ys, 1) end   -- :137-141
  if self.observed == nil then self.observed = rows else self.observed = self.observed:cat(rows, 1) end   -- :143-144
  self.tr_since = self.tr_since + 1
  if self.model and self.tr_since == self.config.bot.nInitial then           -- :147-149, on the window
    local n = self.observed:size(1) - self.tr_start
    self.model:init(self.observed:narrow(1, self.tr_start + 1, n), self.responses:narrow(1, self.tr_start + 1, n))
  end
  local yq = hip.pin(ys:select(2, 1))
  local restart = ffi.new('int[1]')
  assert(hip.C.b7_tr_update(self.tr_state, hip.data(yq), q, restart) == 0, 'run_trial_trust_region: b7_tr_update refused the responses')
  if restart[0] == 1 then self.tr_start, self.tr_since = self.observed:size(1), 0 end
  rec.length_after, rec.restart, rec.x, rec.y = self.tr_state[0].length, restart[0] == 1, rows, ys
  self.tr_trace[#self.tr_trace + 1] = rec
  local col, at, low = ys:select(2, 1), 1, math.huge
  for k = 1, q do
    if col[k] < low then at, low = k, col[k] end
  end
  return rows:select(1, at), ys:narrow(1, at, 1)
end

-- bots/abstract.lua:112-152 for candidates sharded one process per GPU.  Only line 118 differs: `idx` is 1-based in the
-- union of the shards, so it must not index this rank's shard; dist_hip.commit returns the nominee on every rank and
-- deletes the row where it lives.  With one rank (or a group) the parent's code is right as it stands.
function bot:run_trial()
  if self.config.bot.trust_region then return self:run_trial_trust_region() end   -- trust-region nomination: above
  if D.world == 1 then return parent.run_trial(self) end
  local utils = require('bot7.utils')
  self.nTrials = self.nTrials + 1                                            -- :114
  local idx = self:nominate()                                                -- :117, an index into the UNION
  local g   = torch.isTensor(idx) and idx:view(-1)[1] or idx
  local row, loc = D.commit(g, self.candidates and self.candidates:size(2) or nil)   -- :118 across ranks
  self.pending = utils.tensor.append(self.pending, row:view(1, -1))
  if loc > 0 then   -- this rank held it: the host copy of the shard follows the device (same stable deletion)
    self.candidates = utils.tensor.remove(self.candidates, torch.LongTensor{loc})
    if self.candidates ~= nil then hip.set_resident(self.candidates) else hip.forget_resident() end
  end
  idx = self.pending:size(1)                                                 -- :120
  local nominee = self.pending:select(1, idx)                                -- :121
  local y = self.objective(nominee)                                          -- :124 (every rank: lock step)
  if not torch.isTensor(y) then                                              -- :127-133
    if type(y) == 'number' then y = torch.Tensor{{y}} elseif type(y) == 'table' then y = torch.Tensor(y) end
  end
  if y:dim() == 1 then y:resize(y:nElement(), 1) end                         -- :134
  if self.nTrials == 1 then self.responses = y else self.responses = self.responses:cat(y, 1) end   -- :137-141
  self.observed, self.pending = utils.tensor.steal(self.observed, self.pending, torch.LongTensor{idx})   -- :143-144
  if self.model and self.nTrials == self.config.bot.nInitial then            -- :147-149
    self.model:init(self.observed, self.responses)
  end
  return nominee, y
end

return bot
