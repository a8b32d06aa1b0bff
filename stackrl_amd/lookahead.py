"""One-step physics lookahead: what reward would each of k actions give, without taking any of them.

`Lookahead(env, k)` holds a scratch `VecStackEnv` of B x k envs with `env`'s pool and configuration.  `evaluate(actions [B, k])`
(after following a `set_pool` of the env: the scratch env loads the new pool too) gathers env's B state records (csrc/state.hip), writes each k-fold into the scratch handle and runs one `step` there; `env`
itself is not touched.  Randomness belongs to the slot (stackrl_amd/state.py): a forked record continues bit for bit until
its slot's next reset, so the result does not depend on the slot as long as the step is not the auto-reset — `evaluate`
raises there.

`LookaheadPolicy(base, lookahead)` has the signature `compare.run` gives a policy.  Its candidates are the base policy's own
action and the best other entries of the base's value map; it returns the one with the highest simulated reward."""
import torch

from stackrl_amd.env import VecStackEnv


def candidates(action, values, k, n_valid=None, n_actions=None):
  """int64 [B, k]: candidate 0 is `action` [B]; candidates 1 .. k-1 are the other entries of `values` [B, N] in the order of
  their value, descending, ties to the lower index.  With `n_valid` (and `n_actions`, the entries per map) only the entries
  of the first `n_valid` maps are considered."""
  action = action.to(torch.int64).reshape(-1)
  v = values.reshape(action.shape[0], -1)
  if n_valid is not None:
    v = v[:, :int(n_valid) * int(n_actions)]
  k = int(k)
  if not 1 <= k <= v.shape[1]:
    raise ValueError('k must be in 1..{} (the entries considered), got {}'.format(v.shape[1], k))
  if k == 1:
    return action[:, None]
  top = torch.sort(v, dim=1, descending=True, stable=True).indices[:, :k]
  # the base's action leaves the list if it is in it, else the list's last entry does: a stable sort on "is the action"
  keep = torch.sort((top == action[:, None]).to(torch.int8), dim=1, stable=True).indices
  return torch.cat([action[:, None], top.gather(1, keep)[:, :k - 1]], dim=1)


def choose(cand, reward):
  """The candidate [B] with the highest reward [B, k], ties to the lower candidate rank."""
  best = torch.sort(reward, dim=1, descending=True, stable=True).indices[:, 0]
  return cand.gather(1, best[:, None])[:, 0]


def score(reward, distances, penalty):
  """reward - penalty * moved / nb per candidate [B, k]: the simulated reward less the share of the pile's rocks that a push
  moves beyond its tolerances (`PoseDistances.moved`, `nb`; an env without a body has none to move)."""
  return reward - float(penalty) * (distances.moved / torch.clamp(distances.nb, min=1.0)).to(reward.device)


class Lookahead(object):
  def __init__(self, env, k, **kwargs):
    """env: a `VecStackEnv` (or `PipelinedVecStackEnv` / `StartedVecStackEnv`) of B envs; k: actions evaluated per env.
    kwargs go to the scratch env's constructor (e.g. `side_stream`)."""
    self.env, self.k = env, int(k)
    if self.k < 1:
      raise ValueError('k must be at least 1')
    self.B = int(env.batch_size)
    c = env.config
    conf = {f: getattr(c, f) for f in c.__dataclass_fields__ if f not in ('n_envs', 'env_index_offset')}
    n = self.B * self.k
    kwargs.setdefault('concurrent_envs', n)
    self.scratch = VecStackEnv(n_parallel=n, block=True, seed=0, pool=env.pool, device=env._device, **conf, **kwargs)
    self._source = torch.arange(self.B, dtype=torch.int32, device=self.scratch._device).repeat_interleave(self.k)   # record of each scratch env
    self.signature = self.scratch.state_signature()
    if self.signature != env.state_signature():
      raise ValueError('the scratch env does not share the env\'s state signature')

  def close(self):
    self.scratch.close()

  def _follow_pool(self):
    """After `env.set_pool` the env's records name meshes of a table the scratch env does not have: the scratch env loads
    the env's pool too, and whatever else keeps the signatures apart is an error."""
    sig = self.env.state_signature()
    if sig != self.signature:
      if self.scratch.pool is not self.env.pool:
        self.scratch.set_pool(self.env.pool)
        self.signature = self.scratch.state_signature()
      if sig != self.signature:
        raise ValueError('the scratch env does not share the env\'s state signature')

  def fork(self):
    """Every scratch env takes its env's state record, k forks of each (csrc/state.hip); `env` is only read.  Returns the rocks
    the episode has left."""
    env = self.env
    first = env._envs[0] if hasattr(env, '_envs') else env
    first._require_reset('Lookahead.evaluate')
    self._follow_pool()
    left = first._left
    if hasattr(env, '_envs'):
      env.drain()
      records = torch.cat([e._get_records()[0] for e in env._envs])
    else:
      records = env._get_records()[0]
    s = self.scratch
    s._set_records(records, env.state_signature(), None, self._source)   # (the export refuses records of another signature)
    s._left = left
    s._needs_reset = False      # every scratch env now holds a record of the table the scratch has
    return left

  def evaluate(self, actions, observations=False, push=None):
    """actions int64 [B, k] -> (reward [B, k(, keys)], done [B, k]) of one step with each, plus with `observations`
    (obs_map [B, k, H, W, 2], obs_obj [B, k, ...]) in front.  `ValueError` at the auto-reset point (no rock left): there
    the step draws the next episode from the slot's stream.
    With `push`, a `stackrl_amd.push.PushSpec`, every stepped fork is then pushed in place (its state is disposable) and the
    `PoseDistances` [B, k, ...] of the push follow the reward and done: how far the pile with the new rock on it moves."""
    env = self.env
    first = env._envs[0] if hasattr(env, '_envs') else env
    first._require_reset('Lookahead.evaluate')
    if first._left == 0:
      raise ValueError('Lookahead.evaluate at the auto-reset point: the next step resets the envs and its result depends on the slot')
    actions = torch.as_tensor(actions).to(device=self.scratch._device, dtype=torch.int64)
    if tuple(actions.shape) != (self.B, self.k):
      raise ValueError('actions must have shape [{}, {}]'.format(self.B, self.k))
    self.fork()
    s = self.scratch
    (om, oo), r, d = s.step(actions.reshape(-1), block=True)
    shape = (self.B, self.k)
    out = (r.reshape(shape + tuple(r.shape[1:])), d.reshape(shape))
    if observations:
      out = ((om.reshape(shape + tuple(om.shape[1:])), oo.reshape(shape + tuple(oo.shape[1:]))),) + out
    if push is not None:
      dv = push.draw(self.B, self.k, s.config.episode_length, s._device)
      moved = s.push(dv.reshape((self.B * self.k,) + tuple(dv.shape[2:])), push.substeps, select=push.select, tol=push.tol)
      out = out + (moved.reshape(*shape),)
    return out


class LookaheadPolicy(object):
  """`(obs, n_valid=None) -> (actions, values)`: of the base policy's action (candidate 0) and the k - 1 best other entries
  of its value map (by value descending, ties to the lower index), the one whose step gives the highest reward (ties to the
  lower candidate rank).  `values` is the base's map; with k = 1 this is the base policy.  `lookahead`: a `Lookahead`, or
  anything with `k` and `evaluate(actions [B, k]) -> (reward [B, k], done)`.

  With an integer `radius` the candidates are spread (stackrl_amd/candidates.py, include/stackrl_candidates.h): every
  candidate strikes the entries of its map within `radius` pixels, and the next one is the best entry left; `last_count` [B]
  then says how many distinct candidates an env had (the slots beyond repeat candidate 0).  Radius 0 gives the candidates of
  `radius=None`, picked by the kernel; k is at most 32 there.

  With `push`, a `stackrl_amd.push.PushSpec`, every candidate's pile is pushed after its step (`Lookahead.evaluate(push=...)`)
  and a candidate's score is `reward - penalty * moved / nb` (`score`): the share of the pile's rocks the push moves beyond the
  spec's tolerances costs `penalty`.  The tie rule is the same; `last_push` holds the latest `PoseDistances`.  With
  `push=None` nothing changes."""

  def __init__(self, base, lookahead, radius=None, push=None, penalty=0.0):
    self.base, self.lookahead = base, lookahead
    self.radius = None if radius is None else int(radius)
    self.push, self.penalty = push, float(penalty)
    self.last_count = None
    if self.radius is not None:
      from stackrl_amd import candidates as _candidates
      if self.radius < 0:
        raise ValueError('radius must be at least 0, got {}'.format(radius))
      if int(lookahead.k) > _candidates.MAX_K:
        raise ValueError('a radius needs k <= {}, got {}'.format(_candidates.MAX_K, lookahead.k))

  def candidates(self, obs, n_valid=None):
    action, values = self.base(obs) if n_valid is None else self.base(obs, n_valid=n_valid)
    action = torch.as_tensor(action)
    values = torch.as_tensor(values, device=action.device)
    if self.radius is not None:
      from stackrl_amd import candidates as _candidates
      cand, self.last_count = _candidates.select(values.reshape(action.shape[0], -1), action, k=self.lookahead.k, radius=self.radius,
                                                 n_valid=n_valid, OH=int(obs[0].shape[1]) - int(obs[1].shape[-3]) + 1)
      return cand, values
    n_actions = None
    if n_valid is not None:
      n_actions = values.reshape(action.shape[0], -1).shape[1] // obs[1].shape[1]
    return candidates(action, values, self.lookahead.k, n_valid, n_actions), values

  def __call__(self, obs, n_valid=None):
    cand, values = self.candidates(obs, n_valid)
    if cand.shape[1] == 1:
      return cand[:, 0], values
    if self.push is None:
      reward = self.lookahead.evaluate(cand)[0]
    else:
      reward, _, self.last_push = self.lookahead.evaluate(cand, push=self.push)
    if reward.dim() != 2:
      raise ValueError('LookaheadPolicy needs one reward per env and action, got {}'.format(tuple(reward.shape)))
    self.last = (cand, reward)
    if self.push is not None:
      reward = score(reward, self.last_push, self.penalty)
    return choose(cand, reward.to(cand.device)), values
