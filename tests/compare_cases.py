"""Scripted envs and policies of the policy-comparison tests (tests/test_compare.py) and of the script that records what the
reference's `stackrl/test.py` makes of them (tests/golden/make_compare_golden.py): 16 x 16 maps and 8 x 8 object maps, so 81
actions; observations, rewards and episode ends are functions of (env, seed, episode, step, actions so far) alone, so a
one-env gym-style env driven by the reference and a vectorised env driven by `stackrl_amd.compare.run` see the same episodes.
The rewards are multiples of 1/4 and the value maps small integers: every sum the analysis takes of them is exact."""
import collections

import numpy as np

H, OBJ = 16, 8
VSHAPE = (H - OBJ + 1, H - OBJ + 1)
A = VSHAPE[0] * VSHAPE[1]
ENVS = ((0, 5), (1, 5), (2, 4))          # (env id, episode length): with 12 steps a policy, a partial episode ends two of them
NUM_STEPS = 12
SEED = 11
HOLD = -2
SALT = 0          # chosen so that no value of the scripted runs lies within 1e-3 of a threshold (tests/test_compare.py asserts it)
KEYS = ('taps', 'edge', 'mix')


def observation(env_id, seed, episode, t, acc):
  rs = np.random.RandomState([int(seed) % 2 ** 32, env_id, episode, t, acc % 9973, SALT])
  return rs.randint(0, 16, (H, H, 2)).astype(np.uint8), rs.randint(0, 16, (OBJ, OBJ, 1)).astype(np.uint8)


def reward(env_id, t, action):
  return np.float32(((int(action) * 7 + t * 3 + env_id) % 9) * 0.25 - 1.0)


class Core(object):
  """One env's episode machine."""

  def __init__(self, env_id, length):
    self.env_id, self.length = env_id, length
    self.seed(0)

  def seed(self, seed):
    self._seed, self.episode = seed, 0

  def reset(self):
    self.episode += 1
    self.t = self.acc = 0
    return observation(self.env_id, self._seed, self.episode, 0, 0)

  def step(self, action):
    self.t += 1
    self.acc += int(action)
    return (observation(self.env_id, self._seed, self.episode, self.t, self.acc), reward(self.env_id, self.t, action),
            self.t == self.length)


Space = collections.namedtuple('Space', 'shape dtype')
SPACES = (Space((H, H, 2), np.uint8), Space((OBJ, OBJ, 1), np.uint8))


class ScriptedEnv(object):
  """The gym interface the reference's `run` uses (test.py:204-212, :264-265, :322, :333)."""

  def __init__(self, env_id, length):
    self._core = Core(env_id, length)
    self.observation_space = SPACES
    self.action_space = Space((), np.int64)

  def seed(self, seed=None):
    self._core.seed(seed)
    return [seed]

  def reset(self):
    return self._core.reset()

  def step(self, action):
    o, r, d = self._core.step(action)
    return o, r, d, {}


class VecScriptedEnv(object):
  """The same envs side by side behind the interface of `VecStackEnv`, on CPU tensors: a call after an env's `done` resets
  that env (reward 0, done False), an env whose action is HOLD sits the call out."""

  def __init__(self, envs):
    import torch
    self._torch = torch
    self._cores = [Core(e, n) for e, n in envs]
    self.batch_size = len(self._cores)
    self.observation_spec = tuple(Space(s.shape, torch.uint8) for s in SPACES)
    self.n_actions = A
    self._done = [False] * self.batch_size
    self._obs = [None] * self.batch_size
    self.calls = 0

  def seed(self, seed):
    for c in self._cores:
      c.seed(seed)
    return [[seed]] * self.batch_size

  def _pack(self, r, d):
    t = self._torch
    return ((t.from_numpy(np.stack([o[0] for o in self._obs])), t.from_numpy(np.stack([o[1] for o in self._obs]))),
            t.tensor(r, dtype=t.float32), t.tensor(d, dtype=t.bool))

  def reset(self):
    self._obs = [c.reset() for c in self._cores]
    self._done = [False] * self.batch_size
    return self._pack([0.0] * self.batch_size, [False] * self.batch_size)

  def step(self, action):
    self.calls += 1
    r, d = [0.0] * self.batch_size, [False] * self.batch_size
    for b, c in enumerate(self._cores):
      a = int(action[b])
      if a == HOLD:
        continue
      if self._done[b]:
        self._obs[b], self._done[b] = c.reset(), False
        continue
      assert 0 <= a < A
      self._obs[b], r[b], d[b] = c.step(a)
      self._done[b] = d[b]
    step = self._pack(r, d)
    return lambda: step


# ---------------------------------------------------------------------------------------------------- policies
def _sure(v):
  """A map whose sum is a multiple of A has its mean on a grid point, where values sit exactly on the threshold: move it off."""
  if int(v.sum()) % A == 0:
    v[-1] += 1
  return v.astype(np.float32)


def taps(obs):
  m = obs[0][:, :, 0].astype(np.int64)
  return _sure((m[0:9, 0:9] + m[7:16, 7:16] + m[3:12, 4:13]).ravel())


def edge(obs):
  m = obs[0][:, :, 0].astype(np.int64)
  o = int(obs[1].astype(np.int64).sum()) % 5
  return _sure((2 * m[4:13, 4:13] - m[0:9, 7:16] + o).ravel())


def mix(obs):
  m = obs[0].astype(np.int64)
  return _sure((m[0:9, 0:9, 0] + m[7:16, 7:16, 0] + m[3:12, 4:13, 0] + m[0:9, 0:9, 1] % 4).ravel())


VALUE_FNS = dict(zip(KEYS, (taps, edge, mix)))


def single(fn):
  """A policy for the reference's `run`: one observation -> (action, values float32 [A])."""
  def policy(obs):
    v = fn(obs)
    return int(np.argmax(v)), v
  return policy


def batched(fn):
  """A policy for `stackrl_amd.compare.run`: batched observation tensors -> (actions int64 [B], values float32 [B, A])."""
  import torch

  def policy(obs):
    m, o = obs[0].numpy(), obs[1].numpy()
    v = np.stack([fn((m[b], o[b])) for b in range(m.shape[0])])
    return torch.from_numpy(np.argmax(v, axis=-1)), torch.from_numpy(v)
  return policy


# ---------------------------------------------------------------------------------------------------- write
def write_calls():
  """The call sequence of the `write` cases: (tag, file, kwargs, force).  After each call the file's text is recorded; a call
  that raises leaves its message."""
  k = lambda *names: np.array(names)
  f32 = lambda *x: np.array(x, dtype=np.float32)
  return [
    ('new', 'r', dict(keys=k('a', 'b', 'c'), **{'return': f32(1.5, -2.25, 0.125)}, return_std=f32(0.5, 0.25, 0.0), action_value=f32(3, 4, 5),
                      priority=12), False),
    ('append', 'r', dict(keys=k('d'), **{'return': f32(7.75)}, return_std=f32(1.0), action_value=f32(6), priority=12), False),
    ('replace', 'r', dict(keys=k('a'), **{'return': f32(-1.0)}, return_std=f32(2.0), action_value=f32(9), priority=12), False),
    ('higher_kept', 'r', dict(priority=5, keys=k('b', 'e'), action_value=f32(1, 2), **{'return': f32(0.5, 0.75)}, return_std=f32(0.0, 0.5)), False),
    ('mismatch', 'r', dict(keys=k('a'), other=f32(1.0)), False),
    ('mismatch_forced', 'r', dict(keys=k('a', 'z'), other=f32(1.0, 2.5)), True),
    ('plain_new', 'p', dict(x=np.array([1, 2]), some_name=3.5), False),
    ('plain_append', 'p', dict(some_name=np.array([0.25, 0.5]), x=7), False),
  ]
