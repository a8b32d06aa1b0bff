"""Env states as values: what `VecStackEnv.get_state` returns and `set_state` takes.

An `EnvState` holds, for n envs of one handle at one point of their episode:
  records          int32 [n, words]: one state record per env (include/stackrl_hip.h, csrc/state.hip) — header, blob, height
                   map, staged render records;
  obs, reward, done  the latest step's `((obs_map, obs_obj), reward, done)` of those envs.  They are kept, not rendered
                   again on `set_state`: the render kernel also advances the reward memory, so rendering twice is not neutral;
  left             rocks of the running episode not yet placed (the host mirror of the lock-step episode machine);
  seed, sample_counter  the handle's randomness (the episode counters are in the records);
  signature        what a handle must share with the one the state came from (`srl_state_signature`);
  extra            the host fields of `StartedVecStackEnv` (`since_reset`, `done_prev`, the episode-length generator).

Randomness belongs to the slot: the RNG key of env i is seed + env_index_offset + i, the counter is in the record.  A record
written into another slot continues bit for bit until that slot's next reset, which draws the slot's own stream.

`state_dict()` / `from_state_dict()` are plain tensors and numbers and survive `torch.save` / `torch.load`.  `layout` is the
record layout of a configuration (host arithmetic, no device)."""
import ctypes

import numpy as np
import torch

from stackrl_amd import config as _config
from stackrl_amd import lib as _lib

PARTS = ('header', 'blob', 'height_map', 'stage_records')


def layout(config):
  """(words per record, {part: word offset}) of a `StackConfig` (`srl_state_layout`)."""
  c = config.to_c()
  words = ctypes.c_int64()
  off = (ctypes.c_int64 * 4)()
  rc = _lib.load().srl_state_layout(ctypes.byref(c), ctypes.byref(words), off)
  if rc != _config.OK:
    raise ValueError(_lib.last_error())
  return int(words.value), dict(zip(PARTS, (int(o) for o in off)))


def _index_list(x, name):
  if x is None:
    return None
  if torch.is_tensor(x):
    x = x.detach().cpu()
  out = [int(i) for i in np.asarray(x).reshape(-1)]
  if not out:
    raise ValueError('{} must not be empty'.format(name))
  return out


class EnvState(object):
  def __init__(self, records, obs, reward, done, left, seed, sample_counter, signature, extra=None):
    self.records = records
    self.obs = tuple(obs)
    self.reward = reward
    self.done = done
    self.left = int(left)
    self.seed = int(seed)
    self.sample_counter = int(sample_counter)
    self.signature = int(signature)
    self.extra = dict(extra or {})

  def __len__(self):
    return int(self.records.shape[0])

  @property
  def _left(self):      # under the name the envs keep it
    return self.left

  @property
  def device(self):
    return self.records.device

  def step_tuple(self, source=None):
    """The stored `((obs_map, obs_obj), reward, done)`, of the records `source` (a list) or of all, as new tensors."""
    if source is None:
      return (self.obs[0].clone(), self.obs[1].clone()), self.reward.clone(), self.done.clone()
    i = torch.as_tensor(source, dtype=torch.int64, device=self.device)
    return (self.obs[0][i], self.obs[1][i]), self.reward[i], self.done[i]

  def to(self, device):
    def mv(t):
      return t.to(device) if torch.is_tensor(t) else t
    return EnvState(mv(self.records), (mv(self.obs[0]), mv(self.obs[1])), mv(self.reward), mv(self.done), self.left, self.seed,
                    self.sample_counter, self.signature, {k: mv(v) for k, v in self.extra.items()})

  def cpu(self):
    return self.to('cpu')

  def state_dict(self):
    d = {'records': self.records, 'obs_map': self.obs[0], 'obs_obj': self.obs[1], 'reward': self.reward, 'done': self.done,
         'left': self.left, 'seed': self.seed, 'sample_counter': self.sample_counter, 'signature': self.signature}
    d.update({'extra.' + k: v for k, v in self.extra.items()})
    return d

  @classmethod
  def from_state_dict(cls, d):
    extra = {k[len('extra.'):]: v for k, v in d.items() if k.startswith('extra.')}
    return cls(d['records'], (d['obs_map'], d['obs_obj']), d['reward'], d['done'], d['left'], d['seed'], d['sample_counter'],
               d['signature'], extra)


def plan_set(state, signature, left, batch_size, indexes=None, source=None):
  """The checks of `set_state`, on the host: -> (dst, src) as lists or None (None = in order), and whether the whole batch
  returns to the snapshot.  Raises ValueError for a foreign signature, repeated or out-of-range destinations, record indexes
  outside the state, counts that do not match, and a partial set at another point of the episode than the env's."""
  if int(state.signature) != int(signature):
    raise ValueError('the state was taken from an env with another record layout, mesh pool, configuration or library build '
                     '(signature {:#x}, this env {:#x})'.format(int(state.signature), int(signature)))
  dst, src = _index_list(indexes, 'indexes'), _index_list(source, 'source')
  n_state = len(state)
  if src is not None and not all(0 <= s < n_state for s in src):
    raise ValueError('source must index the {} records of the state'.format(n_state))
  n = len(src) if src is not None else n_state
  if dst is None:
    if n != batch_size:
      raise ValueError('without indexes the state (or source) must have one record per env: {} for {} envs'.format(n, batch_size))
    return None, src, True
  if len(set(dst)) != len(dst):
    raise ValueError('indexes must be distinct: an env takes one record')
  if not all(0 <= e < batch_size for e in dst):
    raise ValueError('indexes must be in [0, {})'.format(batch_size))
  if len(dst) != n:
    raise ValueError('{} indexes for {} records'.format(len(dst), n))
  if state.left != left:
    raise ValueError('a partial set_state needs the snapshot at the env\'s own point of the episode ({} rocks left in the '
                     'snapshot, {} in the env): the episode machine\'s host mirror is one number for the batch'.format(state.left, left))
  return dst, src, False
