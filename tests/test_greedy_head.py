"""CPU tests of the greedy head's definition (include/stackrl_greedy.h) as `dqn.greedy_head_reference` restates it, of the
greedy path of `DQN` on the module's own layers, and of the streaming evaluation of `Trainer(fused_eval=True)`."""
import collections
import ctypes
import os
import re

import pytest
import torch

from stackrl_amd import nets
from stackrl_amd.dqn import DQN, greedy_head_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23


def test_qnet_library_exports_the_greedy_head():
  from stackrl_amd import build
  build.build()
  with open(os.path.join(ROOT, 'include', 'stackrl_greedy.h')) as f:
    names = sorted(set(re.findall(r'\b(srl_[a-z0-9_]+)\s*\(', f.read())))
  assert 'srl_greedy_head' in names          # and srl_qnet_last_error, which the comment points to
  L = ctypes.CDLL(build.QLIB)
  for n in names:
    assert hasattr(L, n), 'missing export ' + n
  assert 'greedy.hip' in build.QSRC and any(d.endswith('stackrl_greedy.h') for d in build.deps('qnet'))


@pytest.mark.parametrize('B,G,n_valid,A', [(1, 1, 1, 1), (3, 1, 1, 7), (4, 2, 1, 33), (4, 2, 2, 33), (2, 8, 7, 300)])
def test_reference_against_the_float64_statement(B, G, n_valid, A):
  g = torch.Generator().manual_seed(1000 * B + 10 * G + A)
  adv = 3 * torch.randn(B, G, A, generator=g)
  v = torch.randn(B, generator=g)
  actions, stats, q = greedy_head_reference(adv, v, n_valid)
  a = adv.double()[:, :n_valid]
  q64 = (a - a.mean(-1, keepdim=True) + v.double()[:, None, None]).reshape(B, -1)      # the literal statement
  # one rounding of the mean plus the two float32 operations
  bound = EPS * (a.mean(-1).abs().amax(-1) + a.abs().amax(dim=(1, 2)) + v.double().abs())
  chosen = q64.gather(1, actions[:, None])[:, 0]
  assert bool((q64.amax(-1) - chosen <= bound).all())
  assert bool(((q[:, :n_valid].reshape(B, -1).double() - q64).abs() <= bound[:, None]).all())
  assert bool(torch.isneginf(q[:, n_valid:]).all())
  flat = q[:, :n_valid].reshape(B, -1)
  assert torch.equal(actions, torch.argmax(flat, dim=-1))
  assert torch.equal(stats[:, 0], flat.amax(-1).double()) and torch.equal(stats[:, 1], flat.amin(-1).double())
  assert torch.allclose(stats[:, 2], flat.double().sum(-1), rtol=0, atol=1e-12 * float(flat.double().abs().sum()))
  assert torch.allclose(stats[:, 3], (flat.double() ** 2).sum(-1), rtol=1e-12, atol=0)
  # [B, A] is G = 1
  a2, s2, q2 = greedy_head_reference(adv[:, 0], v)
  a1, s1, q1 = greedy_head_reference(adv[:, :1], v)
  assert torch.equal(a2, a1) and torch.equal(s2, s1) and torch.equal(q2, q1[:, 0])


def test_ties_go_to_the_lowest_flat_index():
  g = torch.Generator().manual_seed(5)
  row = torch.randn(1, 1, 50, generator=g)
  adv = row.expand(3, 2, 50).contiguous()                 # two identical rows: same mean, same q
  v = torch.randn(3, generator=g)
  actions, _, q = greedy_head_reference(adv, v)
  assert torch.equal(q[:, 0], q[:, 1])
  assert torch.equal(actions, torch.argmax(row[0, 0]).expand(3)) and int(actions.max()) < 50
  const = torch.full((2, 3, 17), 1.25)                    # a constant row: every q equals v
  actions, stats, q = greedy_head_reference(const, torch.tensor([0.5, -2.0]))
  assert torch.equal(actions, torch.zeros(2, dtype=torch.int64))
  assert torch.equal(q, torch.tensor([0.5, -2.0])[:, None, None].expand(2, 3, 17))
  assert torch.equal(stats[:, 0], stats[:, 1])


def test_rows_beyond_n_valid_are_never_read():
  g = torch.Generator().manual_seed(6)
  adv = torch.randn(3, 4, 20, generator=g)
  v = torch.randn(3, generator=g)
  ref = greedy_head_reference(adv, v, 2)
  for junk in (float('nan'), float('inf')):
    dirty = adv.clone()
    dirty[:, 2:] = junk
    got = greedy_head_reference(dirty, v, 2)
    assert all(torch.equal(x, y) for x, y in zip(got, ref))
  assert torch.equal(ref[0], greedy_head_reference(adv[:, :2].contiguous(), v)[0])
  with pytest.raises(ValueError):
    greedy_head_reference(adv, v, 0)
  with pytest.raises(ValueError):
    greedy_head_reference(adv, v, 5)


def test_nan_never_wins_and_nothing_winning_is_action_zero():
  inf = float('inf')
  for fill in (-inf, float('nan')):
    a, st, _ = greedy_head_reference(torch.full((2, 1, 9), fill), None)
    assert a.tolist() == [0, 0] and st[0, 0] == -inf
  adv = torch.full((1, 2, 9), float('nan'))
  adv[0, 1] = torch.arange(9.)
  a, st, _ = greedy_head_reference(adv, None)
  assert a.tolist() == [17] and st[0, 0] == 8.0 and st[0, 1] == 0.0 and torch.isnan(st[0, 2])


def test_without_a_value_q_is_the_advantage():
  adv = torch.randn(3, 2, 11, generator=torch.Generator().manual_seed(7))
  a, st, q = greedy_head_reference(adv, None)
  assert torch.equal(q, adv) and torch.equal(a, torch.argmax(adv.reshape(3, -1), dim=-1))
  assert torch.equal(st[:, 0], adv.amax(dim=(1, 2)).double())


# ---------------------------------------------------------------------------- DQN.greedy on the module's own layers
SPEC = ((16, 16, 2), (4, 4, 1))


def _net(seed, dueling=True):
  return nets.DeepQSiamFCN(SPEC, left_filters=4, left_depth=2, pos_filters=4, dueling_units=8, dueling=dueling, seed=seed)


def _agent(B, seed, dueling=True):
  return DQN(_net(seed, dueling), learning_rate=1e-3, minibatch_size=4, replay_memory_size=B * 8, collect_batch_size=B, seed=seed)


def _obs(B, g, G=None):
  o = (B,) if G is None else (B, G)
  return (torch.randint(0, 256, (B,) + SPEC[0], generator=g, dtype=torch.uint8),
          torch.randint(0, 256, o + SPEC[1], generator=g, dtype=torch.uint8))


def test_dqn_greedy_is_the_definition_on_the_nets_own_pieces():
  agent = _agent(5, seed=3)
  x = _obs(5, torch.Generator().manual_seed(1))
  a, st, q = agent.greedy(x, stats=True, values=True)
  _, qm = agent.policy(x, values=True)                     # the module: float32 mean; the definition: float64 sum, one rounding
  assert q.shape == qm.shape and float((q - qm).abs().max()) <= 4 * EPS * float(qm.abs().max() + 1)
  assert torch.equal(a, torch.argmax(q, dim=-1)) and torch.equal(agent.greedy(x), a)
  assert torch.equal(st[:, 0], q.amax(-1).double()) and torch.equal(st[:, 1], q.amin(-1).double())
  # a net without the dueling head: Q is the advantage, bit for bit what the module returns
  plain = _agent(5, seed=3, dueling=False)
  a, q = plain.greedy(x, values=True)
  pa, pq = plain.policy(x, values=True)
  assert torch.equal(q, pq) and torch.equal(a, pa)


def test_orientation_layout_matches_orientation_greedy():
  from stackrl_amd.policies import FusedOrientationGreedy, OrientationGreedy
  agent = _agent(3, seed=4)
  x = _obs(3, torch.Generator().manual_seed(2), G=4)
  for n_valid in (None, 4, 3, 1):
    a, q = FusedOrientationGreedy(agent, value=True)(x, n_valid=n_valid)
    ra, rq = OrientationGreedy(agent.q_net, value=True)(x, n_valid=n_valid)
    assert q.shape == rq.shape and torch.equal(torch.isneginf(q), torch.isneginf(rq))
    fin = ~torch.isneginf(rq)
    assert float((q[fin] - rq[fin]).abs().max()) <= 4 * EPS * float(rq[fin].abs().max() + 1)
    assert torch.equal(a, torch.argmax(q, dim=-1))
    assert torch.equal(FusedOrientationGreedy(agent)(x, n_valid=n_valid), a)
    assert bool((rq.gather(1, a[:, None])[:, 0] >= rq.amax(-1) - 8 * EPS * (rq[fin].abs().max() + 1)).all())
  with pytest.raises(TypeError):
    FusedOrientationGreedy(agent.q_net)


# ---------------------------------------------------------------------------- streaming evaluation
class _ToyEnv(object):
  """The env interface `Trainer` uses, on CPU tensors: episodes of `L` steps, done on the L-th step, the step after a done is
  the reset step (reward 0, done False)."""

  def __init__(self, B, L, spec, seed=0):
    self.batch_size, self.L, self.spec = B, L, spec
    TS = collections.namedtuple('TS', 'shape dtype')
    self.observation_spec = tuple(TS(tuple(s), torch.uint8) for s in spec)
    self.n_actions = (spec[0][0] - spec[1][0] + 1) ** 2
    self.seed(seed)

  def seed(self, seed=None):
    self._g = torch.Generator().manual_seed(int(seed or 0))
    self._t = 0
    return [seed]

  def _obs(self):
    return tuple(torch.randint(0, 256, (self.batch_size,) + tuple(s), generator=self._g, dtype=torch.uint8) for s in self.spec)

  def reset(self):
    self._t = 0
    return self._obs(), torch.zeros(self.batch_size), torch.zeros(self.batch_size, dtype=torch.bool)

  def step(self, action):
    assert action.shape == (self.batch_size,) and int(action.max()) < self.n_actions
    self._t += 1
    if self._t % (self.L + 1) == 0:      # auto-reset call
      step = (self._obs(), torch.zeros(self.batch_size), torch.zeros(self.batch_size, dtype=torch.bool))
    else:
      done = torch.full((self.batch_size,), self._t % (self.L + 1) == self.L)
      # the reward depends on the action: a different greedy action gives a different return
      step = (self._obs(), torch.rand(self.batch_size, generator=self._g) + action.float() / self.n_actions, done)
    return lambda: step


class _Recorder(object):
  """An agent seen through `policy(values=True)`, keeping every step's values."""

  def __init__(self, agent):
    self.agent, self.values = agent, []

  def __getattr__(self, name):
    return getattr(self.agent, name)

  def policy(self, inputs, values=False, **kw):
    a, q = self.agent.policy(inputs, values=True, **kw)
    self.values.append(q)
    return (a, q) if values else a


def _rel(x, y):
  return abs(x - y) / max(abs(y), 1e-300)


@pytest.mark.parametrize('dueling', [False, True])
def test_streaming_eval_row_equals_the_row_from_the_stacked_values(dueling):
  """The agent without the dueling head is the issue's case: both paths see the same float32 Q (q = adv), only the float64
  combination order differs, 1e-9.  With the dueling head `agent.policy` takes the module's float32 mean where the
  definition rounds the float64 mean once, so Q differs by a rounding of the mean and the comparison with the module's
  stacked values holds to that rounding only (measured with seeds 3, 4, 5: the five statistics differ from the module's by
  up to 2.1e-7 relative, the mean by up to 4.7e-8); the 1e-9 comparison is then made against the stacked `agent.greedy` values,
  and the one against the module's within four float32 roundings of the values' magnitude."""
  from stackrl_amd.training import Trainer
  B, L = 3, 4

  def trainer(agent, fused):
    return Trainer(_ToyEnv(B, L, SPEC, seed=1), agent, eval_env=_ToyEnv(B, L, SPEC, seed=2), directory=None, eval_seed=5,
                   eval_reward_buffer_length=6, fused_eval=fused)

  row = trainer(_agent(B, 3, dueling), True).eval()
  rec = _Recorder(_agent(B, 3, dueling))
  plain = trainer(rec, False).eval()                                       # the default: the existing formula
  values = torch.stack(rec.values)
  assert values.dim() == 3 and values.shape[0] >= 2 * L
  assert plain == (0, plain[1], float(values.amax(dim=-1).mean()), float(values.mean()), float(values.std(unbiased=False)),
                   float(values.min()), float(values.max()))
  if dueling:                          # the stacked values of the definition itself
    agent = _agent(B, 3, dueling)
    env = _ToyEnv(B, L, SPEC, seed=5)
    step, qs = env.reset(), []
    for _ in range(values.shape[0]):
      a, q = agent.greedy(step[0], values=True)
      qs.append(q)
      step = env.step(a)()
    values, tol = torch.stack(qs), 4 * EPS
  d = values.double()
  want = (float(d.amax(dim=-1).mean()), float(d.mean()), float(d.std(unbiased=False)), float(d.min()), float(d.max()))
  print('fused', row, 'float64 from stacked', want, 'plain', plain)
  assert row[0] == 0 and row[1] == plain[1]                               # the return: exactly
  for got, w in zip(row[2:], want):
    assert _rel(got, w) <= 1e-9, (got, w)
  if dueling:
    for got, w in zip(row[2:], plain[2:]):
      assert abs(got - w) <= tol * (abs(w) + float(values.abs().max())), (got, w)


def test_fused_eval_writes_the_same_file_format(tmp_path):
  from stackrl_amd.training import Trainer
  d = str(tmp_path / 'run')
  tr = Trainer(_ToyEnv(3, 4, SPEC, seed=1), _agent(3, 3), eval_env=_ToyEnv(2, 4, SPEC, seed=2), directory=d, eval_seed=5,
               eval_reward_buffer_length=4, fused_eval=True)
  row = tr.eval()
  rows = open(os.path.join(d, 'eval.csv')).read().strip().split('\n')
  assert rows[0] == 'Iter,Return,Value,MeanValue,StdValue,MinValue,MaxValue' and len(rows) == 2
  assert tuple(float(x) for x in rows[1].split(',')[1:]) == row[1:]
  assert row[5] <= row[3] <= row[2] <= row[6] and row[4] >= 0
